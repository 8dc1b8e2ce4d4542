#!/usr/bin/env python3
"""Static instruction counts of the restart kernel per source region: compiles a scratch copy of pt_kernels.hip with
assembler-comment markers at the region boundaries and counts VALU / SALU / LDS / scratch / lane-spill instructions between
them in the ISA listing (block placement follows the source closely enough for this to be a useful map; the markers are
scheduling barriers, so the listing differs slightly from the shipped code).   python3 scripts/isa_regions.py [--dump REGION]
VARIANT=6 counts the generic instantiation of a resident scene (PT_RS_GENERIC) instead of the shipped one (0), VARIANT=8 the flat
one (PT_RS_FLAT: flat scenes under a uniform environment), VARIANT=9 / 10 the skip forms of the flat and the shipped one
(PT_RS_FLAT_SKIP, PT_RS_PLAIN_SKIP), VARIANT=11 the flat deferring form (PT_RS_FLAT_SKIP_DEFER) and VARIANT=14 its tight copy
(PT_RS_FLAT_SKIP_TIGHT), which is compiled in a unit of its own, pt_kernels_tight.hip: its counts come from that unit's listing.
The tight form's kernel body is its own (pt_tight_body.h, an explicit specialisation): its regions carry the same names, from
anchors in that header (TIGHT_MARKS), and one more, restart_begin, which parts the restart step and the refill from the staging
in front of them; so is its shading half (pt_tight_shade.h), whose regions carry path_post's names, from anchors of its own
(TIGHT_SHADE_MARKS)."""
import os, re, sys, collections
from kernel_listing import CSRC, listing
SRC = os.path.join(CSRC, "pt_kernels.hip")
MARKS = [  # (unique source anchor, marker name) — the marker goes in front of the anchor
    ("    if (!idle) {\n      if (!walking) {\n        best.t = PT_MAX_DIST;", "round_begin"),
    ("      } else if (WIDE) {\n        traverse_round4<STATS, FORM.wide>", "traverse_begin"),
    ("      if (node == WALK_OVER) {\n        // the iteration's first variate", "traverse_end"),
    ("        if (path_post<STATS, FIXED, FLAT>(p, st, r1, n, cnt)) {\n          path_finish_sample(p, st);", "lights_end"),
    ("          path_finish_sample(p, st);\n          idle = true;\n          if (STATS) samples++;", "post_end"),
    ("  if (!STATIC && !p.is_static) {\n    st.acc = found ? inter.diffuse_col : env_lookup<FLAT>(p, st.d);", "resolve_end"),
    ("  const f3 d = st.d;\n  const float cos_theta = dot(inter.normal, d);", "miss_end"),
    ("  const float pmax = __builtin_fmaxf(st.throughput.x, __builtin_fmaxf(st.throughput.y, st.throughput.z));\n  if (r1 > pmax && st.b() > 1u) return true;\n  st.throughput = st.throughput * rcp_hot(pmax);\n  ++st.bk;\n  return", "bsdf_end"),
]


TIGHT_UNIT = "pt_kernels_tight.hip"   # compiles pt_kernels.hip once more, for the tight forms alone
TIGHT_VARIANTS = ("14",)
TIGHT_BODY = "pt_tight_body.h"        # the tight form's own kernel body, included by pt_kernels.hip in that unit only
TIGHT_MARKS = [
    ("    unsigned long long need = __ballot(st.xy == PT_TIGHT_IDLE);\n    while (need) {", "restart_begin"),
    ("    if (st.xy != PT_TIGHT_IDLE) {\n      if (node == 0xFFFFu) {", "round_begin"),
    ("      traverse_round_tight(s_nodes, s_tris, reinterpret_cast<const uint32_t*>(s_mem)", "traverse_begin"),
    ("      if (node == 0xFFFFu) {\n        // the iteration's first variate", "traverse_end"),
    ("          tight_park(p, st.xy, st.acc);\n          st.xy = PT_TIGHT_IDLE;", "post_end"),
]
TIGHT_SHADE = "pt_tight_shade.h"      # the tight form's own shading half, included by its body: path_post's regions, from anchors of its own.
# A region is named for what the shared function holds under that name: lights_end the hit's decode, resolve_end the misses' tail,
# miss_end the BSDF sample, bsdf_end the roulette.  The tail stands in front of the decode in this source, so resolve_end comes first
# (regions() takes the markers in the listing's order), and traverse_end, the light loop, runs up to it.
TIGHT_SHADE_MARKS = [
    ("  if (!found) {\n    const f3 env = mk3(", "resolve_end"),
    ("  f3 normal, direct_light;", "lights_end"),
    # (this marker holds the normal: without it the compiler starts the BSDF sample's reflection, 18 VALU, inside the decode's region)
    ("  // the BSDF sample (raytrace.cu:88-120), ior 1\n", "miss_end", '"+v"(normal.x), "+v"(normal.y), "+v"(normal.z)'),
    ("  // the roulette (raytrace.cu:183-192)\n", "bsdf_end"),
]


def mark(s, marks):
    for anchor, name, *held in marks:   # held: output operands the marker pins, so that what is computed from them stays behind it
        assert s.count(anchor) == 1, (name, s.count(anchor))
        s = s.replace(anchor, 'asm volatile("; PT_MARK %s" : %s :: "memory");\n' % (name, held[0] if held else "") + anchor)
    return s


def marked_listing(tight=False):
    """The ISA listing (lines) of pt_kernels.hip compiled with a marker in front of every anchor of MARKS.  tight: of
    pt_kernels_tight.hip, the same marked text behind that unit's own lines."""
    s = mark(open(SRC).read(), MARKS)
    if not tight:
        return listing("pt_kernels.hip", s).split("\n")
    unit = open(os.path.join(CSRC, TIGHT_UNIT)).read()
    body = '#include "%s"\n' % TIGHT_BODY
    assert s.count(body) == 1
    tight = mark(open(os.path.join(CSRC, TIGHT_BODY)).read(), TIGHT_MARKS)
    shade = '#include "%s"\n' % TIGHT_SHADE
    assert tight.count(shade) == 1
    s = s.replace(body, tight.replace(shade, mark(open(os.path.join(CSRC, TIGHT_SHADE)).read(), TIGHT_SHADE_MARKS)))
    include = '#include "pt_kernels.hip"\n'
    assert unit.count(include) == 1
    return listing(TIGHT_UNIT, unit.replace(include, s)).split("\n")


def regions(lines, variant):
    """[(region name, Counter, (first line, end line))] of pt_megakernel_restart<true, variant> in a marked listing."""
    start = [i for i, l in enumerate(lines) if re.match(r"_ZN\d+ptamd\w*21pt_megakernel_restartILb1ELi%sEEEvNS_7KParamsE:" % variant, l)][0]
    end = [i for i, l in enumerate(lines) if i > start and re.match(r"\.Lfunc_end\d+:", l)][0]
    marks = [(i, re.search(r"; PT_MARK (\w+)", lines[i]).group(1)) for i in range(start, end) if "; PT_MARK" in lines[i]]
    bounds = [(start, "prologue")] + marks + [(end, "end")]
    out = []
    for (a, n), (b, _) in zip(bounds, bounds[1:]):
        c = collections.Counter()
        for l in lines[a:b]:
            t = l.strip().split()[0] if l.strip() else ""
            if t.startswith("v_readlane") or t.startswith("v_writelane"): c["lane-spill"] += 1
            elif t.startswith("v_mov"): c["v_mov"] += 1; c["VALU"] += 1
            elif t.startswith("v_"): c["VALU"] += 1
            elif t.startswith("s_") and not t.startswith(("s_waitcnt", "s_nop")): c["SALU"] += 1
            elif t.startswith("ds_"): c["LDS"] += 1
            elif t.startswith("scratch_"): c["scratch"] += 1
            elif t.startswith(("global_", "flat_", "buffer_")): c["VMEM"] += 1
        out.append((n, c, (a, b)))
    return out


if __name__ == "__main__":
    lines = marked_listing(tight=os.environ.get("VARIANT", "0") in TIGHT_VARIANTS)
    dump = sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == "--dump" else None
    for n, c, (a, b) in regions(lines, os.environ.get("VARIANT", "0")):
        print("%-16s %s" % (n, dict(c)))
        if dump == n:
            print("\n".join(l for l in lines[a:b] if l.strip() and not l.strip().startswith((";", "."))))
