// pt_tight_shade.h — the shading half of the restart kernel's tight form (PT_RS_FLAT_SKIP_TIGHT), its own: what the round does with a
// lane whose walk is over, between the light loop and the park.  Included by pt_tight_body.h, and by the host harness that compares
// the misses' tail with the shared one (tests/san/tight_miss_host.cpp), which sees the first half alone.
//
// It is compiled for what the form's launches are (pt_device.h: restart_select, round_form_tight): a flat scene (the 64-byte compact
// record, ior bitwise 1, no normal map, 1x1 maps), a one-colour environment, a static camera, Path::bk the bounce index alone.  Every
// floating-point operation of a path is path_post<false, true, true>'s (resolve_hit, miss_tail_finish, the BSDF sample, the roulette):
// the same operation on the same values in the same order.  What differs is integer, address, control and data-movement work:
//   * the hit's record is addressed as a 32-bit byte offset (64 * face; include/ptamd.h keeps a resident scene below 2048 records)
//     from a scalar base the kernel forms once, in front of its persistent loop; a light's two float4 likewise from KParams::lights;
//   * a lane is decoded only where it has a hit, and the decoded hit holds what the flat case uses: normal, colour, specular; a
//     light's emission is added where the light is decoded;
//   * BOTH variates of an iteration are drawn where the first one was, after the walk, by every lane: the generator's state then moves
//     by the same two places in every lane, and the copies that kept a missing lane's state one place behind a hit lane's are gone.
//     A lane that misses does not use the second variate; the rare lane that runs the literal iterations of the misses' loop steps
//     the generator back by that one draw first (xorwow_undraw), so it draws what it drew before;
//   * the misses' tail: a wave whose missing lanes are all at a maximum of exactly 1 (every primary miss, nearly every later one)
//     runs the adds alone, on the accumulator in place; throughput, bounce index, r1 and the generator are not written, so nothing of
//     them is copied where the missing lanes meet the others.  Any other wave runs miss_tail_finish as it is, on copies.
#pragma once

// ---------------------------------------------------------------- the misses' tail, one lane's arithmetic (host and device)

// The generator's state one draw back: xorwow_uniform moves v1..v4 one place down and adds its step to d; v0_before is the word the
// draw consumed.
PT_HD Xorwow xorwow_undraw(const Xorwow& now, uint32_t v0_before)
{
  Xorwow r;
  r.v0 = v0_before; r.v1 = now.v0; r.v2 = now.v1; r.v3 = now.v2; r.v4 = now.v3; r.d = now.d - 362437u;
  return r;
}

// The tail of a lane that missed: miss_tail_finish restated, with its first loop (the literal iterations of a lane whose maximum is not
// 1 yet) behind one test the caller makes for the whole wave, skip_literal: true only where no lane of the wave would run a pass of
// it.  b: the bounce index (Path::bk of the tight form); drawn: the generator behind the iteration's SECOND variate, v0_before: the
// word that draw consumed (the literal iterations draw on from behind the first one, as they always did).  Writes acc alone: the
// literal iterations run on copies.  (Run on the path's own throughput, which is dead behind a miss, they cost the lanes with a hit
// three copies where the two meet.)
template <class Rcp>
PT_HD void tight_miss_tail(bool skip_literal, f3 env, int max_bounces, f3& acc, f3 thr, uint32_t b, float r1, const Xorwow& drawn, uint32_t v0_before, Rcp rcp)
{
  if (!skip_literal) {
    Xorwow rng = xorwow_undraw(drawn, v0_before);
    while (!miss_tail_is_closed(thr))
      if (miss_tail_iteration(env, max_bounces, acc, thr, b, r1, rng, rcp)) return;
  }
  const f3 e = env * thr;
  const uint32_t n = miss_tail_count(b, max_bounces);
  for (uint32_t i = 0; i < n; ++i) acc = acc + e;
}

#ifdef PT_TIGHT_BUILD
// ---------------------------------------------------------------- the shading half (device)

// the base of a flat scene's compact records, which lie behind the general ones (KParams::shade): wave-uniform, formed once
PT_DEV const char* tight_records(const KParams& p)
{
  return reinterpret_cast<const char*>(p.shade + (size_t)PT_KARG(p, n_faces) * 7);
}

PT_DEV float4 tight_load4(const char* base, uint32_t offset) { return *reinterpret_cast<const float4*>(base + offset); }

// One iteration of radiance()'s loop behind the nearest-hit search, for a lane of the tight form.  r1, r2: the iteration's two
// variates, drawn in this order; v0_before: the generator's first word in front of the second draw.  Returns true when the path is
// complete (st.acc is final).
PT_DEV bool tight_shade(const KParams& p, const char* records, Path& st, float r1, float r2, uint32_t v0_before, Nearest nearest)
{
  const int max_bounces = p.bounces;
  // resolve_hit's `found`: a winner, and nearer than PT_MAX_DIST (a NaN distance is no hit)
  const bool found = nearest.idx != PT_END && nearest.t < PT_MAX_DIST;
  if (!found) {
    const f3 env = mk3(PT_KARG(p, env_r), PT_KARG(p, env_g), PT_KARG(p, env_b));
    tight_miss_tail(wave_all(miss_tail_is_closed(st.throughput)), env, max_bounces, st.acc, st.throughput, st.bk, r1, st.rng, v0_before, [](float x) { return rcp_hot(x); });
    return true;
  }

  f3 normal, direct_light;   // direct_light: brdf_lambert / pdf_lambert (brdf.cuh:14-31), the colour over 0.5, formed where the colour is loaded
  float specular = st.specular_col;   // a light leaves it as the last mesh hit set it
  const f3 d = st.d;
  if (nearest.idx & PT_LIGHT) {
    const char* lights = reinterpret_cast<const char*>(p.lights);
    const uint32_t at = (nearest.idx & ~PT_LIGHT) << 5;
    const float4 la = tight_load4(lights, at), lb = tight_load4(lights, at + 16u);
    const f3 col = mk3(la.x, la.y, la.z);
    direct_light = col / 0.5f;
    normal = normalize_hot(mk3(la.w, lb.x, lb.y) - (nearest.t * d)); // intersection.cuh:208: origin ignored
    // raytrace.cu:86: (light colour * emission) * throughput
    st.acc = st.acc + (col * lb.z) * st.throughput;
  } else {
    const uint32_t at = nearest.idx << 6;
    const float4 s0 = tight_load4(records, at), s1 = tight_load4(records, at + 16u), s2 = tight_load4(records, at + 32u);
    specular = *reinterpret_cast<const float*>(records + (at + 48u));
    const f3 n0 = mk3(s0.x, s0.y, s0.z), n1 = mk3(s1.x, s1.y, s1.z), n2 = mk3(s2.x, s2.y, s2.z);
    const float u = nearest.u, v = nearest.v;
    const float w = 1.0f - u - v;
    normal = w * n0 + u * n1 + v * n2;
    direct_light = mk3(s0.w, s1.w, s2.w) / 0.5f;
    // (formed here, on this side of the join: the compiler otherwise carries the colour across it, through three copies)
    asm volatile("" : "+v"(direct_light.x), "+v"(direct_light.y), "+v"(direct_light.z));
  }
  st.specular_col = specular;

  // the BSDF sample (raytrace.cu:88-120), ior 1
  const f3 spec = normalize_hot(reflect(d, normal));
  const float phi = (float)((double)2.0f * 3.14159265358979323846 * (double)r2);
  // r1 is a uniform variate in (0, 1]: both arguments are 0 or >= 2^-33
  const float sin_t = sqrt_hot(r1);
  const float cos_t = sqrt_hot(1.f - r1);
  const f3 axis = (__builtin_fabsf(normal.x) >= 0.1f) ? mk3(0.0f, 1.0f, 0.0f) : mk3(1.0f, 0.0f, 0.0f);
  const f3 u = normalize_hot(cross(axis, normal));
  const f3 v = cross(normal, u);
  float sphi, cphi;
  pt_sincosf(phi, sphi, cphi);
  const f3 dd = normalize_hot(v * sin_t * cphi + u * sphi * sin_t + normal * cos_t);
  st.o = st.o + d * nearest.t;
  st.d = mix(dd, spec, specular);
  st.o = st.o + st.d * 0.03f;
  st.throughput = st.throughput * direct_light;

  // the roulette (raytrace.cu:183-192)
  const float pmax = max3(st.throughput);
  if (r1 > pmax && st.bk > 1u) return true;
  st.throughput = st.throughput * rcp_hot(pmax);
  ++st.bk;
  return (int)st.bk >= max_bounces;
}
#endif
