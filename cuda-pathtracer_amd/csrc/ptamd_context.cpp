// ptamd_context.cpp — the device context of libptamd.so (include/ptamd.h): the last error, ptamd_create / ptamd_destroy, the
// device allocation, copy and synchronisation utilities, the frame counter, counters, the gamma self-test and the time stamps.
#include "ptamd_host.h"
#include "pt_refit.h"
#include "pt_refit_device.h"
#include "pt_reface.h"
#include "pt_rematerial.h"
#include "pt_relink.h"
#include "pt_morph.h"
#include "pt_query.h"
#include "pt_radiance.h"
#include "pt_gather.h"

#include <cstring>
#include <memory>
#include <new>

namespace ptamd {

static thread_local std::string g_last_error;

void set_error(const std::string& msg) { g_last_error = msg; }

int hip_fail(const char* what, hipError_t e)
{
  set_error(std::string(what) + ": " + hipGetErrorString(e));
  return PTAMD_ERR_HIP;
}

// The first operation of a new stream, issued and waited for at once: it brings the stream's queue up (~6 ms on this runtime),
// which would otherwise land in a frame
int bring_up(ptamd_context* ctx, hipStream_t s)
{
  PT_HIP(hipMemsetAsync(ctx->d_stats.get() + 13, 0, sizeof(unsigned long long), s));   // (word 13: read by no one)
  PT_HIP(hipStreamSynchronize(s));
  return PTAMD_OK;
}

bool stream_is_capturing(hipStream_t stream)
{
  if (stream == nullptr) return false;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone;
}

} // namespace ptamd

using namespace ptamd;

extern "C" {

const char* ptamd_get_last_error(void) { return g_last_error.c_str(); }
#ifndef PTAMD_BUILD_ID
#define PTAMD_BUILD_ID "unknown"
#endif
const char* ptamd_version(void) { return "ptamd 0.3 (gfx950) device code " PTAMD_BUILD_ID; }
const char* ptamd_build_id(void) { return PTAMD_BUILD_ID; }

uint32_t ptamd_interleaved_rows(uint32_t height, uint32_t ranks, uint32_t rank, uint32_t band_rows)
{
  if (ranks == 0 || rank >= ranks || band_rows == 0) return 0;
  uint32_t rows = 0;
  for (uint64_t y0 = (uint64_t)rank * band_rows; y0 < height; y0 += (uint64_t)ranks * band_rows)
    rows += (uint32_t)(y0 + band_rows <= height ? band_rows : height - y0);
  return rows;
}

uint32_t ptamd_wang_hash(uint32_t a)
{
  a = (a ^ 61u) ^ (a >> 16);
  a = a + (a << 3);
  a = a ^ (a >> 4);
  a = a * 0x27d4eb2du;
  a = a ^ (a >> 15);
  return a;
}

int ptamd_create(int32_t device_ordinal, ptamd_context** out)
{
  if (!out) { set_error("ptamd_create: null out"); return PTAMD_ERR_ARG; }
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0) {
    set_error(std::string("ptamd_create: no HIP device (") + (e != hipSuccess ? hipGetErrorString(e) : "count = 0") +
              "); this library has no CPU fallback");
    return PTAMD_ERR_HIP;
  }
  if (device_ordinal < 0 || device_ordinal >= n) { set_error("ptamd_create: device ordinal out of range"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(device_ordinal));
  std::unique_ptr<ptamd_context> ctx(new (std::nothrow) ptamd_context());
  if (!ctx) { set_error("ptamd_create: out of memory"); return PTAMD_ERR_ARG; }
  ctx->device = device_ordinal;
  read_tuning_knobs(ctx->knobs);
  // (a failure below deletes the context, and with it everything allocated so far)
  PT_HIP(ctx->d_stats.alloc(32 * sizeof(unsigned long long)));
  PT_HIP(hipMemset(ctx->d_stats.get(), 0, 32 * sizeof(unsigned long long)));
  PT_HIP(ctx->d_tickets.alloc(kTicketRing * sizeof(uint32_t)));
  PT_HIP(ctx->d_heads.alloc((size_t)kTicketRing * 8u * PT_HEAD_STRIDE * sizeof(uint32_t)));
  PT_HIP(hipMemset(ctx->d_heads.get(), 0, (size_t)kTicketRing * 8u * PT_HEAD_STRIDE * sizeof(uint32_t)));
  ctx->heads_clean.assign(kTicketRing, true);
  ctx->slot_pinned.assign(kTicketRing, false);
  if (ctx->knobs.gamma_table) {
    PT_HIP(ctx->d_gamma.alloc(258 * sizeof(float)));
    hipError_t ge = build_gamma_table(ctx->d_gamma.get(), nullptr);
    if (ge == hipSuccess) ge = hipDeviceSynchronize();
    if (ge != hipSuccess) return hip_fail("ptamd_create: gamma table", ge);
  }
  hipDeviceProp_t prop;
  PT_HIP(hipGetDeviceProperties(&prop, device_ordinal));
  ctx->n_cus = prop.multiProcessorCount;
  if (ctx->knobs.overlap) {
    // the two internal streams of the launch pipeline (null-stream callers), with their queues brought up now
    for (Stream& is : ctx->internal) {
      PT_HIP(is.create_non_blocking());
      const int brc = bring_up(ctx.get(), is.get());
      if (brc != PTAMD_OK) return brc;
    }
  }
  *out = ctx.release();
  return PTAMD_OK;
}

void ptamd_destroy(ptamd_context* ctx)
{
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  // before anything is released: megakernels may still be running on the lanes and internal streams (they read the scene tables and
  // the ticket heads), resolve passes on the callers' streams
  (void)hipDeviceSynchronize();
  delete ctx;
}

int ptamd_setup_function_tables(ptamd_context* ctx)
{
  if (!ctx) { set_error("ptamd_setup_function_tables: null context"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  // resolves every kernel entry point in the gfx950 code object (hipFuncGetAttributes loads it on first use), so a
  // missing or mismatched device image fails here, as the reference's cudaMemcpyFromSymbol calls would (raytrace.cu:362-374)
  hipError_t e = resolve_kernels();
  if (e == hipSuccess) e = resolve_refit_kernels();
  if (e == hipSuccess) e = resolve_refit_device_kernels();
  if (e == hipSuccess) e = resolve_reface_kernels();
  if (e == hipSuccess) e = resolve_rematerial_kernels();
  if (e == hipSuccess) e = resolve_rig_kernels();
  if (e == hipSuccess) e = resolve_relink_kernel();
  if (e == hipSuccess) e = resolve_query_kernels();
  if (e == hipSuccess) e = resolve_radiance_kernels();
  if (e == hipSuccess) e = resolve_gather_kernels();
  if (e != hipSuccess) return hip_fail("ptamd_setup_function_tables: device code object", e);
  return PTAMD_OK;
}

int ptamd_reset_frame_counter(ptamd_context* ctx)
{
  if (!ctx) { set_error("ptamd_reset_frame_counter: null context"); return PTAMD_ERR_ARG; }
  ctx->frame_counter = 0;
  return PTAMD_OK;
}

int ptamd_phase_cycles(ptamd_context* ctx, uint64_t out[12])
{
  if (!ctx || !out) { set_error("ptamd_phase_cycles: null argument"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  PT_HIP(hipDeviceSynchronize());
  PT_HIP(hipMemcpy(out, ctx->d_stats.get() + 16, 12 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return PTAMD_OK;
}

int ptamd_device_error_count(ptamd_context* ctx, uint64_t* out)
{
  if (!ctx || !out) { set_error("ptamd_device_error_count: null argument"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  PT_HIP(hipDeviceSynchronize());
  unsigned long long v = 0;
  PT_HIP(hipMemcpy(&v, ctx->d_stats.get() + 15, sizeof v, hipMemcpyDeviceToHost));
  *out = v;
  return PTAMD_OK;
}

int ptamd_gamma_table_selftest(ptamd_context* ctx, uint64_t* out_checked, uint64_t* out_mismatches)
{
  if (!ctx || !out_checked || !out_mismatches) { set_error("ptamd_gamma_table_selftest: null argument"); return PTAMD_ERR_ARG; }
  *out_checked = 0; *out_mismatches = 0;
  if (!ctx->d_gamma) return PTAMD_OK;   // no table in use
  PT_HIP(hipSetDevice(ctx->device));
  float limit = 0.0f;                   // T[256]: the table form is used below it
  PT_HIP(hipMemcpy(&limit, ctx->d_gamma.get() + 256, sizeof limit, hipMemcpyDeviceToHost));
  uint32_t limit_bits;
  std::memcpy(&limit_bits, &limit, 4);
  // every positive value below the limit, plus the 2^20 patterns from the limit on (those take the pt_powf form: must agree
  // trivially), plus the negative half's first 2^20 and the NaN patterns' first 2^20
  PT_HIP(hipMemsetAsync(ctx->d_stats.get() + 14, 0, sizeof(unsigned long long), nullptr));
  const uint32_t ranges[3][2] = { { 0u, limit_bits + (1u << 20) }, { 0x80000000u, 1u << 20 }, { 0x7F800000u, 1u << 20 } };
  for (const auto& r : ranges) {
    hipError_t e = launch_gamma_selftest(ctx->d_gamma.get(), r[0], r[1], ctx->d_stats.get() + 14, nullptr);
    if (e != hipSuccess) return hip_fail("ptamd_gamma_table_selftest", e);
    *out_checked += r[1];
  }
  PT_HIP(hipDeviceSynchronize());
  unsigned long long bad = 0;
  PT_HIP(hipMemcpy(&bad, ctx->d_stats.get() + 14, sizeof bad, hipMemcpyDeviceToHost));
  *out_mismatches = bad;
  return PTAMD_OK;
}

int ptamd_probe_layout(uint32_t what, uint32_t arg, uint32_t* out_in_words, uint32_t* out_out_words)
{
  // {input words (with `active`), output words (with the sentinel)} per PTAMD_PROBE_* number; XORWOW's output grows by its draws
  static const uint32_t kWords[PTAMD_PROBE_COUNT][2] = {
    { 21, 5 }, { 21, 5 }, { 21, 5 }, { 21, 5 }, { 11, 3 }, { 6, 6 }, { 2, 7 }, { 2, 3 }, { 3, 2 }, { 2, 2 }, { 2, 7 }, { 6, 2 }, { 4, 4 }, { 5, 2 }, { 2, 2 },
    { 2, 8 }, { 2, 8 }, { 2, 8 },
  };
  if (!out_in_words || !out_out_words || what >= PTAMD_PROBE_COUNT) { set_error("ptamd_probe_layout: bad argument"); return PTAMD_ERR_ARG; }
  const bool arg_ok = what == PTAMD_PROBE_XORWOW ? (arg >= 1u && arg <= 8192u) : (what == PTAMD_PROBE_OUTPUT ? arg <= 1u : (what == PTAMD_PROBE_ENV || arg == 0u));
  if (!arg_ok) { set_error("ptamd_probe_layout: bad arg for this probe"); return PTAMD_ERR_ARG; }
  *out_in_words = kWords[what][0];
  *out_out_words = kWords[what][1] + (what == PTAMD_PROBE_XORWOW ? arg : 0u);
  return PTAMD_OK;
}

int ptamd_probe(ptamd_context* ctx, uint32_t what, const void* in_dev, uint32_t n, void* out_dev, uint32_t arg)
{
  if (!ctx || !in_dev || !out_dev) { set_error("ptamd_probe: null argument"); return PTAMD_ERR_ARG; }
  uint32_t in_words = 0, out_words = 0;
  if (ptamd_probe_layout(what, arg, &in_words, &out_words) != PTAMD_OK) { set_error("ptamd_probe: bad what or arg"); return PTAMD_ERR_ARG; }
  const bool sweep = what >= PTAMD_PROBE_SWEEP_RCP;
  if (n == 0 || n > (1u << 24) || (sweep && n != 1u)) { set_error("ptamd_probe: n out of range"); return PTAMD_ERR_ARG; }
  if ((uintptr_t)in_dev % 4u || (uintptr_t)out_dev % (sweep ? 8u : 4u)) { set_error("ptamd_probe: misaligned pointer"); return PTAMD_ERR_ARG; }
  if (what == PTAMD_PROBE_ENV && arg >= ctx->cubemaps.size()) { set_error("ptamd_probe: cubemap id out of range"); return PTAMD_ERR_ARG; }
  if (what == PTAMD_PROBE_OUTPUT && arg == 1u && !ctx->d_gamma) { set_error("ptamd_probe: the context has no gamma table"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  KParams p = {};
  p.gamma_table = ctx->d_gamma.get();
  if (what == PTAMD_PROBE_ENV) {
    const DeviceCubemap& cm = ctx->cubemaps[arg];
    p.cubemap = cm.faces.get(); p.cubemap_size = cm.size;
    p.env_uniform = cm.uniform ? 1u : 0u; p.env_r = cm.color[0]; p.env_g = cm.color[1]; p.env_b = cm.color[2];
  }
  if (sweep) {   // counts of 0, "first" words of 0xFFFFFFFF, which the kernel lowers with atomicMin
    PT_HIP(hipMemsetAsync(out_dev, 0, 8 * sizeof(uint32_t), nullptr));
    PT_HIP(hipMemsetAsync(static_cast<uint32_t*>(out_dev) + 4, 0xFF, 2 * sizeof(uint32_t), nullptr));
  }
  const hipError_t e = launch_probe(p, what, static_cast<const uint32_t*>(in_dev), n, static_cast<uint32_t*>(out_dev), in_words, out_words, arg, nullptr);
  if (e != hipSuccess) return hip_fail("ptamd_probe", e);
  PT_HIP(hipDeviceSynchronize());
  return PTAMD_OK;
}

int ptamd_set_timeline(ptamd_context* ctx, uint32_t max_waves)
{
  if (!ctx) { set_error("ptamd_set_timeline: null context"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  PT_HIP(hipDeviceSynchronize());
  ctx->d_timeline.reset();
  ctx->timeline_waves = 0;
  if (max_waves == 0) return PTAMD_OK;
  PT_HIP(ctx->d_timeline.alloc((size_t)max_waves * 4u * sizeof(unsigned long long)));
  PT_HIP(hipMemset(ctx->d_timeline.get(), 0, (size_t)max_waves * 4u * sizeof(unsigned long long)));
  ctx->timeline_waves = max_waves;
  return PTAMD_OK;
}

int ptamd_read_timeline(ptamd_context* ctx, uint64_t* out, uint32_t n_waves, uint32_t* clock_khz)
{
  if (!ctx || !out || n_waves > ctx->timeline_waves) { set_error("ptamd_read_timeline: bad argument"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  PT_HIP(hipDeviceSynchronize());
  PT_HIP(hipMemcpy(out, ctx->d_timeline.get(), (size_t)n_waves * 4u * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  PT_HIP(hipMemset(ctx->d_timeline.get(), 0, (size_t)ctx->timeline_waves * 4u * sizeof(unsigned long long)));
  if (clock_khz) {
    int khz = 0;
    PT_HIP(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device));
    *clock_khz = (uint32_t)khz;
  }
  return PTAMD_OK;
}

int ptamd_device_alloc(ptamd_context* ctx, size_t bytes, void** out)
{
  if (!ctx || !out) { set_error("ptamd_device_alloc: null argument"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  PT_HIP(hipMalloc(out, bytes ? bytes : 16));
  const int fill = alloc_fill_byte();   // tuning knob PTAMD_ALLOC_FILL: the one place a test reads the fill back
  if (fill >= 0) PT_HIP(fill_new(*out, fill, bytes ? bytes : 16, false));
  return PTAMD_OK;
}

int ptamd_device_free(ptamd_context* ctx, void* p)
{
  if (!ctx) { set_error("ptamd_device_free: null context"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  PT_HIP(hipFree(p));
  return PTAMD_OK;
}

int ptamd_device_memset(ptamd_context* ctx, void* p, int value, size_t bytes, void* stream)
{
  if (!ctx || !p) { set_error("ptamd_device_memset: null argument"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  PT_HIP(hipMemsetAsync(p, value, bytes, static_cast<hipStream_t>(stream)));
  return PTAMD_OK;
}

int ptamd_device_to_host(ptamd_context* ctx, void* dst_host, const void* src_dev, size_t bytes, void* stream)
{
  if (!ctx || !dst_host || !src_dev) { set_error("ptamd_device_to_host: null argument"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  PT_HIP(hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream)));
  PT_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
  return PTAMD_OK;
}

int ptamd_host_to_device(ptamd_context* ctx, void* dst_dev, const void* src_host, size_t bytes, void* stream)
{
  if (!ctx || !dst_dev || !src_host) { set_error("ptamd_host_to_device: null argument"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  PT_HIP(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, static_cast<hipStream_t>(stream)));
  PT_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
  return PTAMD_OK;
}

int ptamd_stream_synchronize(ptamd_context* ctx, void* stream)
{
  if (!ctx) { set_error("ptamd_stream_synchronize: null context"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  PT_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
  return PTAMD_OK;
}

int ptamd_get_frame_counter(ptamd_context* ctx, uint32_t* out)
{
  if (!ctx || !out) { set_error("ptamd_get_frame_counter: null argument"); return PTAMD_ERR_ARG; }
  *out = ctx->frame_counter;
  return PTAMD_OK;
}

} // extern "C"
