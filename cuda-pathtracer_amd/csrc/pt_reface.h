// pt_reface.h — the material half of a face's shading record, written once for the upload (host/scene_tables.cpp:
// make_scene_tables) and for ptamd_scene_replace's kernels (pt_reface.hip): DESIGN.md §13 "Another number of faces".
//
// A shading record is 28 floats.  Floats 0..17 follow the face's geometry and are the refit's (pt_refit.h); words 18..27 follow its
// material_id alone and are formed here:
//   18      the id; bit 31: the diffuse+specular map is 1x1 and the record carries its texel; bit 30: the material has a normal map
//   19      ior
//   20..23  the one RGBA texel of a 1x1 map, or the map's descriptor {w, h, nb_chan, offset}
//   24..27  the normal map's descriptor, or zeros
// and, for flat scenes, the four texel words of the compact record {n0, r} {n1, g} {n2, b} {specular, 0, 0, 0} behind the general
// ones.  Everything is moved as 32-bit words: no float is interpreted, so host and device leave the same bytes whatever the texels
// hold.  The header includes nothing of HIP; the host half compiles with a plain C++ compiler.
#pragma once

#include "pt_refit.h"

#include <stddef.h>

namespace ptamd {

// The tables as both sides hold them: ptamd_material / the device's int4 {diffuse_spec_map, normal_map, bits(ior), 0}, and
// ptamd_texture_desc / TexDesc
struct RfcMaterial { int32_t diffuse_spec_map, normal_map; uint32_t ior_bits; int32_t pad; };
struct RfcTexture { int32_t w, h, nb_chan; uint32_t pad; uint64_t offset; };

constexpr uint32_t kRfcConstantMap = 0x80000000u;   // bit 31 of word 18
constexpr uint32_t kRfcNormalMap = 0x40000000u;     // bit 30 of word 18
constexpr uint32_t kRfcNoBadFace = 0xFFFFFFFFu;     // the minimum over "no face has a bad id"

// What a face's material_id decides: words 18..27 of its shading record, the compact record's texel words {r, g, b, specular}, and
// whether the face lets its scene be flat
struct RfcWords {
  uint32_t shade[10];
  uint32_t texel[4];
  bool flat;
};

// The id check.  Every caller makes it BEFORE it indexes a table with the id.
PT_RF_HD bool rfc_id_ok(uint32_t material_id, uint32_t n_materials) { return material_id < n_materials; }

// scene_is_flat's rule for one face: a 1x1 diffuse+specular map, no normal map, ior bitwise 1.0f (path_post tests ior == 1.0f, and
// a NaN ior is not flat)
PT_RF_HD bool rfc_flat(const RfcMaterial& m, const RfcTexture& dt)
{
  return dt.w == 1 && dt.h == 1 && m.normal_map < 0 && m.ior_bits == 0x3F800000u;
}

// The two tables come as bytes and are copied out record by record: the host's are ptamd_material (16 bytes, 16-byte records) and
// ptamd_texture_desc (24 bytes), the device's int4 and TexDesc, of the same layout.
PT_RF_HD RfcMaterial rfc_material(const void* materials, uint32_t id)
{
  RfcMaterial m;
  __builtin_memcpy(&m, static_cast<const char*>(__builtin_assume_aligned(materials, 4)) + (size_t)id * sizeof(RfcMaterial), sizeof m);
  return m;
}
PT_RF_HD RfcTexture rfc_texture(const void* textures, int32_t id)
{
  RfcTexture t;
  __builtin_memcpy(&t, static_cast<const char*>(__builtin_assume_aligned(textures, 8)) + (size_t)id * sizeof(RfcTexture), sizeof t);
  return t;
}

// `material_id` has passed rfc_id_ok; the material's texture ids are valid (validate_scene_desc at the upload)
PT_RF_HD void rfc_words(uint32_t material_id, const void* materials, const void* textures, const float* texels, RfcWords& out)
{
  const RfcMaterial m = rfc_material(materials, material_id);
  const RfcTexture dt = rfc_texture(textures, m.diffuse_spec_map);
  const float* texel = texels + dt.offset;
  for (int k = 0; k < 4; ++k) out.texel[k] = rf_float_to_bits(texel[k]);   // (a diffuse+specular map has four channels)
  uint32_t word = material_id;
  out.shade[1] = m.ior_bits;
  if (dt.w == 1 && dt.h == 1) {
    // a 1x1 diffuse+specular map (every material of indoor.obj as the reference loads it on Linux): sampleTexture can only ever
    // return texel 0 (intersection.cuh:20-26: x = int(uv.x * 0)), so the record carries the texel itself and the kernel skips the
    // dependent texel load
    for (int k = 0; k < 4; ++k) out.shade[2 + k] = out.texel[k];
    word |= kRfcConstantMap;
  } else {
    out.shade[2] = (uint32_t)dt.w; out.shade[3] = (uint32_t)dt.h; out.shade[4] = (uint32_t)dt.nb_chan; out.shade[5] = (uint32_t)dt.offset;
  }
  if (m.normal_map >= 0) {
    const RfcTexture nt = rfc_texture(textures, m.normal_map);
    out.shade[6] = (uint32_t)nt.w; out.shade[7] = (uint32_t)nt.h; out.shade[8] = (uint32_t)nt.nb_chan; out.shade[9] = (uint32_t)nt.offset;
    word |= kRfcNormalMap;               // the record's 7th float4 (normal map) is in use
  } else {
    out.shade[6] = 0u; out.shade[7] = 0u; out.shade[8] = 0u; out.shade[9] = 0u;
  }
  out.shade[0] = word;
  out.flat = rfc_flat(m, dt);
}

// The result words of the device pass, and what it reads and writes (pt_reface.hip)
constexpr uint32_t kRefaceResultWords = 4;   // {1 when some face is not flat, the lowest face with a bad id or kRfcNoBadFace, 0, 0}
inline uint32_t reface_groups(uint32_t n_faces) { return (n_faces + kRefitThreads - 1u) / kRefitThreads; }

struct RefaceParams {
  const float* faces;            // the caller's records, kFaceFloats floats each: word 27 is the id
  const void* materials;         // 16 bytes each {diffuse_spec_map, normal_map, bits(ior), 0}
  const void* textures;          // 24 bytes each {w, h, nb_chan, pad, offset}
  const float* texels;
  float* shade;                  // n_faces general records, then n_faces compact ones: every byte is written
  uint32_t* ids;                 // one word per face: its id, for the host's copy
  uint32_t* partials;            // two words per workgroup {not flat, lowest bad face}
  uint32_t* result;              // kRefaceResultWords
  uint32_t n_faces, n_materials;
};

} // namespace ptamd

#if defined(__HIPCC__)
namespace ptamd {
// Two kernels in stream order: the faces (one thread each), then one workgroup that folds the partials into `result`
hipError_t launch_reface(const RefaceParams& r, hipStream_t stream);
// ... the second of them alone, for another face pass that leaves the same partials (pt_rematerial.hip)
hipError_t launch_reface_fold(const uint32_t* partials, uint32_t n_groups, uint32_t* result, hipStream_t stream);
hipError_t resolve_reface_kernels();

// the workgroup's OR of `not_flat` and minimum of `bad`, valid in thread 0: the one fold of every kernel that forms these two words
__device__ __forceinline__ void rfc_fold_words(uint32_t (&so)[kRefitThreads], uint32_t (&sm)[kRefitThreads], uint32_t& not_flat, uint32_t& bad)
{
  so[threadIdx.x] = not_flat;
  sm[threadIdx.x] = bad;
  __syncthreads();
  for (uint32_t h = kRefitThreads / 2u; h > 0u; h >>= 1) {
    if (threadIdx.x < h) {
      so[threadIdx.x] |= so[threadIdx.x + h];
      const uint32_t other = sm[threadIdx.x + h];
      if (other < sm[threadIdx.x]) sm[threadIdx.x] = other;
    }
    __syncthreads();
  }
  not_flat = so[0];
  bad = sm[0];
}
}
#endif
