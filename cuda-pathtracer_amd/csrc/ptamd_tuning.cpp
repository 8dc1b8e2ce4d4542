// ptamd_tuning.cpp — the gate of every tuning knob and the table of those a context reads at ptamd_create (ptamd_tuning.h).
#include "ptamd_tuning.h"
#include "../host/ptamd_internal.h"

#include <cstdlib>
#include <cstring>

namespace ptamd {

const char* tuning_env(const char* name)
{
  const char* gate = std::getenv("PTAMD_TUNING");
  if (!gate || std::atoi(gate) != 1) return nullptr;
  return std::getenv(name);
}

int alloc_fill_byte()
{
  const char* e = tuning_env("PTAMD_ALLOC_FILL");
  if (!e || !*e) return -1;
  char* end = nullptr;
  const long v = std::strtol(e, &end, 10);
  if (*end || v < 0 || v > 255) return -1;   // (not clamped: a test that asks for a byte it cannot have runs unfilled, and says so)
  return (int)v;
}

namespace {

enum KnobKind {
  kSwitch,     // atoi != 0
  kClamped,    // atoi, clamped to lo..hi
  kKernel,     // atoi; values outside lo..hi are ignored, one inside also clears default_kernel_is_builtin
  kSkipWord,   // "root", "all", "0" (no node), anything else the default selection
  kOpenUnit,   // atof; accepted only strictly inside (lo, hi)
};

struct Knob {
  const char* name;
  KnobKind kind;
  bool TuningSettings::* flag;         // kSwitch
  uint32_t TuningSettings::* number;   // kClamped, kKernel, kSkipWord
  float TuningSettings::* real;        // kOpenUnit
  int lo, hi;
};

constexpr Knob on_off(const char* name, bool TuningSettings::* f) { return { name, kSwitch, f, nullptr, nullptr, 0, 1 }; }
constexpr Knob number(const char* name, KnobKind kind, uint32_t TuningSettings::* f, int lo, int hi) { return { name, kind, nullptr, f, nullptr, lo, hi }; }

using S = TuningSettings;
constexpr Knob kKnobs[] = {
  on_off("PTAMD_GAMMA_TABLE", &S::gamma_table),
  on_off("PTAMD_OVERLAP", &S::overlap),
  number("PTAMD_REFILL_MIN", kClamped, &S::refill_min, 1, 64),
  number("PTAMD_DEFAULT_KERNEL", kKernel, &S::default_kernel, 1, 6),
  number("PTAMD_ROUND_MIN", kClamped, &S::round_min, 1, 64),
  number("PTAMD_ROUND_DIV", kClamped, &S::round_div, 1, 64),
  number("PTAMD_WALK_MIN", kClamped, &S::walk_min, 1, 64),
  number("PTAMD_WALK_MIN4", kClamped, &S::walk_min4, 1, 64),
  number("PTAMD_LEAF_DEFER", kClamped, &S::leaf_defer, 0, 64),
  on_off("PTAMD_SHORT_RCP", &S::short_rcp),
  on_off("PTAMD_WIDE8", &S::wide8),
  on_off("PTAMD_WIDE4Q", &S::wide4q),
  on_off("PTAMD_RS_GENERIC", &S::generic_round),
  on_off("PTAMD_RS_FLAT", &S::flat_round),
  on_off("PTAMD_RS_TIGHT", &S::tight_round),
  number("PTAMD_SKIP", kSkipWord, &S::skip_mode, 0, 0),
  { "PTAMD_SKIP_THRESHOLD", kOpenUnit, nullptr, nullptr, &S::skip_threshold, 0, 1 },
  on_off("PTAMD_POOL_LDS", &S::pool_in_lds),
  on_off("PTAMD_POOL_LDS_WIDE", &S::pool_in_lds_wide),
  number("PTAMD_TREELET", kClamped, &S::treelet_nodes, 0, 1024),
  number("PTAMD_XCD_REGIONS", kClamped, &S::xcd_regions, 0, 2),
  number("PTAMD_TILES_PER_TICKET", kClamped, &S::tiles_per_ticket, 1, 1024),
};

} // namespace

void read_tuning_knobs(TuningSettings& s)
{
  s = TuningSettings();
  for (const Knob& k : kKnobs) {
    const char* e = tuning_env(k.name);
    if (!e) continue;
    const int v = std::atoi(e);
    switch (k.kind) {
      case kSwitch: s.*k.flag = v != 0; break;
      case kClamped: s.*k.number = (uint32_t)(v < k.lo ? k.lo : (v > k.hi ? k.hi : v)); break;
      case kKernel:
        if (v >= k.lo && v <= k.hi) { s.*k.number = (uint32_t)v; s.default_kernel_is_builtin = false; }
        break;
      case kSkipWord:
        s.*k.number = !std::strcmp(e, "root") ? PTAMD_SKIP_ROOT : (!std::strcmp(e, "all") ? PTAMD_SKIP_ALL : (!std::strcmp(e, "0") ? PTAMD_SKIP_SET : PTAMD_SKIP_DEFAULT));
        break;
      case kOpenUnit: {
        const float f = (float)std::atof(e);
        if (f > (float)k.lo && f < (float)k.hi) s.*k.real = f;
        break;
      }
    }
  }
}

} // namespace ptamd
