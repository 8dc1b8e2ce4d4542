// pt_launch.h — host-callable launchers of the device code in pt_kernels.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ptamd.h"

namespace ptamd {

struct KParams;
struct DenoiseParams;
struct TemporalParams;

// One form of a megakernel: a compiled instantiation and what a launch has to know about it (pt_kernels.hip: launchers)
struct KernelForm {
  const void* fn;            // what is launched
  const void* occupancy_fn;  // whose residency sizes the grid: the plain instantiation of the form's family
  uint32_t threads;          // workgroup size
  uint32_t ticket_waves;     // waves per workgroup that take tile tickets; 0: the tile kernels' 2-D grid of one thread per pixel
  size_t lds_bytes;          // dynamic LDS of the launch
  uint32_t cache_slot;       // index into ptamd_context::occupancy (kFormSlot*)
  const char* name;          // the family, for error text
  int restart_form = -1;     // the restart kernel: the PT_RS_* number of `fn` (pt_device.h: kRestartForms); -1: another family
};
enum : uint32_t { kFormSlotTile, kFormSlotPersistent, kFormSlotBlockwise, kFormSlotSplit, kFormSlotRestart, kFormSlotRestartContracted, kFormSlotRestartList, kFormSlots };
// kernel: PTAMD_KERNEL_* with AUTO resolved.  lds_bytes: of the scene's copy; for the restart kernel the launch's dynamic LDS
// (ptamd_launch.cpp: lay_out_lds).  list: the list form of adaptive sampling (pt_adaptive.h; KParams::adaptive names the state's device
// block).  p: the launch, whose fields choose among the restart kernel's forms (pt_device.h: restart_select, kRestartForms), or nullptr before it is
// known: everything but `fn` is then already final.
KernelForm megakernel_form(uint32_t kernel, bool lds_resident, bool stats, bool list, size_t lds_bytes, const KParams* p);
hipError_t form_blocks_per_cu(const KernelForm& f, int* out);
// n_blocks: the grid of every form that takes tickets (the tile kernels' follows from the launch's rows).  Nothing to do: hipSuccess
hipError_t launch_form(const KernelForm& f, const KParams& p, uint32_t n_blocks, hipStream_t stream);
uint32_t restart_threads(bool lds_resident);
// the wide walk's LDS treelet: chunk-major in a region of this size whenever a node is staged (pt_kernels.hip: PT_TREELET_STRIDE)
constexpr uint32_t kRestartTreeletRegionBytes = 64u * 1024u;
uint32_t restart_wide_blocks_per_cu();
hipError_t launch_resolve(const KParams& p, hipStream_t stream);
// gamma step of the tonemap as a table (pt_kernels.hip: gamma_byte): 258 floats, and its exhaustive check
hipError_t build_gamma_table(float* table_dev, hipStream_t stream);
hipError_t launch_gamma_selftest(const float* table_dev, uint32_t first, uint32_t count, unsigned long long* out_dev, hipStream_t stream);
// the probe of the device functions (pt_kernels.hip: pt_probe_kernel; ptamd_probe): rows of in_words words in, rows of out_words words out
hipError_t launch_probe(const KParams& p, uint32_t what, const uint32_t* in_dev, uint32_t n, uint32_t* out_dev, uint32_t in_words, uint32_t out_words,
                        uint32_t arg, hipStream_t stream);
// Resolves every kernel entry point of the code object (setupFunctionTables' role: fail early when the device image is unusable).
hipError_t resolve_kernels();
// walk-only kernel fed from a ray queue (pt_kernels.hip: pt_trace_queue_kernel): shape of a configuration, launch
void trace_queue_shape(uint32_t config, uint32_t* threads, uint32_t* plane_nodes, uint32_t* blocks_per_cu);
hipError_t launch_trace_queue(const KParams& p, uint32_t config, size_t lds_bytes, uint32_t n_blocks, const float* rays_dev, uint32_t n, int4* out_dev,
                              uint32_t* head_dev, int* resident_blocks_per_cu, hipStream_t stream);
hipError_t launch_trace_rays(const KParams& p, int kind, const float* rays_dev, uint32_t n, int4* out_dev,
                             hipStream_t stream);
// denoiser (pt_denoise.h): the feature pass (kind 1 every face, 2 the binary tree from L2) and one pass of the filter
// (0 prepare, 1 variance, 2 a-trous level, 3 plain output), full frames
hipError_t launch_features(const KParams& p, int kind, float4* feat_dev, float* rays_dev, hipStream_t stream);
hipError_t launch_denoise_pass(const DenoiseParams& q, int pass, hipStream_t stream);
// adaptive sampling (pt_adaptive.hip): select (mask, scan, scatter), the resolve of the list form, the full-frame resolve
struct AdaptiveParams;
hipError_t launch_adaptive_select(const AdaptiveParams& a, hipStream_t stream);
hipError_t launch_adaptive_resolve_list(const AdaptiveParams& a, hipStream_t stream);
hipError_t launch_adaptive_resolve(const AdaptiveParams& a, hipStream_t stream);
// temporal half (pt_denoise_temporal.hip): 0 reproject and blend, 1 temporal variance, 2 capture, 3 plain output
hipError_t launch_temporal_pass(const DenoiseParams& q, const TemporalParams& t, int pass, hipStream_t stream);
// ... and pass 0 in its motion form (pt_denoise_motion.hip): reproject along the faces' motion since the previous call, and blend
struct MotionParams;
hipError_t launch_motion_reproject(const DenoiseParams& q, const TemporalParams& t, const MotionParams& m, hipStream_t stream);
// guided upsample (pt_upsample.hip): 0 prepare the low frame's geometry records, 1 upsample to the full frame
struct UpsampleParams;
hipError_t launch_upsample_pass(const UpsampleParams& u, int pass, hipStream_t stream);

} // namespace ptamd

// the contracted instantiation of the restart kernel (pt_kernels_fma.hip) exports its form of a launch; megakernel_form asks it
extern "C" void ptamd_fma_restart_form(int lds_resident, size_t lds_bytes, const ptamd::KParams* p, ptamd::KernelForm* out);
// the unit of the restart kernel's tight forms (pt_kernels_tight.hip) exports their entries (nullptr: none compiled); restart_entry_of asks it
extern "C" const void* ptamd_tight_restart_entry(int variant, int lds_resident);
