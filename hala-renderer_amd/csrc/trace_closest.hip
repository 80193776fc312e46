// trace_closest.hip — the closest-hit traversal kernels of the wavefront path tracer (what the reference gets from `trace_rays(width,
// height, 1)`, src/rt_renderer.rs:458-464): camera rays generated in place at depth 0, a compact ray queue after that.  One update() =
// one sample per pixel = for each bounce { traverse_closest -> shade (shade.hip) -> traverse_shadow (trace_shadow.hip) } -> resolve
// (resolve.hip).  All queue sizes live in a device control block; nothing returns to the host inside a frame.
#include <algorithm>

#include "trace_loop.h"
#include "variants.h"

namespace rt {
// ---------------------------------------------------------------------------------------------------------
// K5a: persistent closest-hit traversal over a compact ray queue (coalesced 32-B ray reads, 16-B hit writes)
// ---------------------------------------------------------------------------------------------------------
template <bool ANY, bool COUNT, bool STAGED, bool ALPHA, bool INST>
__global__ void __launch_bounds__(kTraverseThreads, STAGED ? kTraverseWavesPerSimdStaged : kTraverseWavesPerSimd)
k_trace_batch(SceneView sv, const hala_ray* __restrict__ rays, hala_hit* __restrict__ hits, const uint32_t* __restrict__ n_ptr,
              uint32_t n_imm, WorkCounters* __restrict__ work, uint2* __restrict__ spill_base, Control* __restrict__ ctl, int account,
              uint32_t refill) {
  const TraverseLds lds = stage_bvh<STAGED, INST>(sv, g_smem);
  const uint32_t n = n_ptr ? *n_ptr : n_imm;
  uint2* spill = lane_spill(spill_base);
  StepCounters sc;
  if (account && blockIdx.x == 0 && threadIdx.x == 0) {
    if (ANY) ctl->totals.rays_shadow += n; else ctl->totals.rays_closest += n;
  }
  BatchSource src{rays, hits, ANY, account != 0, STAGED && refill == 64u};
  persistent_trace<ANY, COUNT, STAGED, ALPHA, INST>(sv, lds, spill, work, n, refill, src, sc);
  if (COUNT) flush_counters(ctl, ANY ? 1 : 0, sc);
}

// K5a at depth 0: the camera rays are generated in the lanes that trace them (RENDER_SPEC §5) — no ray-generation kernel,
// no primary-ray queue in HBM; entry i of the hit queue belongs to path slot i.  `n_account` = real (non-padding) paths.  VIEWS: fc.views > 1.
template <bool COUNT, bool STAGED, bool INST, bool VIEWS, bool FAR>
__global__ void __launch_bounds__(kTraverseThreads, STAGED ? kTraverseWavesPerSimdStaged : kTraverseWavesPerSimd)
k_trace_primary(SceneView sv, FrameConst fc, hala_hit* __restrict__ hits, WorkCounters* __restrict__ work, uint2* __restrict__ spill_base,
                Control* __restrict__ ctl, uint32_t n_account, uint32_t refill) {
  const TraverseLds lds = stage_bvh<STAGED, INST>(sv, g_smem);
  uint2* spill = lane_spill(spill_base);
  StepCounters sc;
  if (blockIdx.x == 0 && threadIdx.x == 0) ctl->totals.rays_closest += n_account;
  CameraSource<VIEWS, FAR> src{fc, sv, hits, STAGED && refill == 64u};
  persistent_trace<false, COUNT, STAGED, false, INST>(sv, lds, spill, work, fc.slot_count, refill, src, sc);
  if (COUNT) flush_counters(ctl, 0, sc);
}
uint32_t traverse_stack_lds_levels(TreeForm tree) {
  return tree == TreeForm::Staged ? kStackLdsStaged : (tree == TreeForm::TwoLevel ? kStackLdsInst : kStackLdsGlobal);
}
size_t traverse_fixed_lds_bytes(TreeForm tree) {  // per-lane stacks (+ the waves' leaf work lists and merge slots of the large-scene variants)
  const size_t stacks = (size_t)traverse_stack_lds_levels(tree) * kTraverseThreads * 8;
  return tree == TreeForm::Staged ? stacks : stacks + (kTraverseThreads / 64) * kCoopBytesPerWave;
}
uint32_t traverse_stack_spill_levels() { return kStackSpill; }
uint32_t traverse_max_leaf(TreeForm tree) { return tree == TreeForm::Staged ? 8u : (uint32_t)kLeafSlots; }
uint32_t traverse_blocks_per_cu(size_t dynamic_lds_bytes, TreeForm tree) {  // each traversal unit answers for a kernel of its own: the launches share one grid
  const uint32_t closest = tree_blocks_per_cu([](auto STAGED, auto INST) { return k_trace_batch<false, false, STAGED, false, INST>; }, tree, kTraverseThreads, dynamic_lds_bytes);
  const uint32_t shadow = trace_shadow_blocks_per_cu(dynamic_lds_bytes, tree);
  return closest < shadow ? closest : shadow;
}

// The traversal kernels are compiled per (any-hit, counting, tree form) and, for the any-hit ones, per "the scene has translucent
// materials" (RENDER_SPEC 7.1d: the ALPHA variants carry the texture fetch that decides whether a flagged triangle blocks); all
// launch-time constants
void launch_trace_batch(const LaunchCfg& lc, const SceneView& sv, const hala_ray* rays, hala_hit* hits, const uint32_t* n_ptr,
                        uint32_t n_imm, WorkCounters* work, Control* ctl, bool any, bool count, bool account, hipStream_t s) {
  SceneView sva = sv;
  if (any) sva.tris = sv.tris_any;  // RENDER_SPEC 7.1d
  const TreeForm tree = tree_form(sv);
  dispatch<kFamilyTraceBatch>([&](auto ANY, auto COUNT, auto ALPHA, auto STAGED, auto INST) {
    hipLaunchKernelGGL((k_trace_batch<ANY, COUNT, STAGED, ALPHA, INST>), dim3(lc.persistent_blocks), dim3(kTraverseThreads), lc.smem, s, sva, rays,
                       hits, n_ptr, n_imm, work, lc.spill, ctl, account ? 1 : 0, lc.refill);
  }, any, count, any && sv.any_translucent, tree == TreeForm::Staged, tree == TreeForm::TwoLevel);
}
void launch_trace_primary(const LaunchCfg& lc, const SceneView& sv, const FrameConst& fc, hala_hit* hits, WorkCounters* work, Control* ctl,
                          uint32_t n_account, bool count, bool far_camera, hipStream_t s) {
  const TreeForm tree = tree_form(sv);
  // camera rays of neighbouring pixels are about equally long: larger refills (40 idle lanes instead of 24) keep the 8 x 8 pixel blocks together
  const uint32_t refill = tree == TreeForm::Staged ? lc.refill : std::max(lc.refill, 40u);
  dispatch<kFamilyTracePrimary>([&](auto COUNT, auto STAGED, auto INST, auto VIEWS, auto FAR) {
    hipLaunchKernelGGL((k_trace_primary<COUNT, STAGED, INST, VIEWS, FAR>), dim3(lc.persistent_blocks), dim3(kTraverseThreads), lc.smem, s, sv, fc, hits, work,
                       lc.spill, ctl, n_account, refill);
  }, count, tree == TreeForm::Staged, tree == TreeForm::TwoLevel, fc.views > 1u, far_camera);
}

// ---------------------------------------------------------------------------------------------------------
// RENDER_SPEC 4.2, far origins, for a caller's ray batch: the rule runs at the batch's entry and exit, around the traversal launch, not
// inside it.  Entry: a copy of the batch with every far origin re-based, and per ray the distance it was moved; exit (closest hit):
// that distance back on the hit's t.  A batch without far origins is copied as it is and gets +0 on every t: the same bits.
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_rebase_batch(SceneView sv, const hala_ray* __restrict__ rays, hala_ray* __restrict__ out, float* __restrict__ moved, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4* rp = reinterpret_cast<const float4*>(rays + i);
  const float4 ro = rp[0], rd = rp[1];
  f3 o = mk3(ro.x, ro.y, ro.z);
  const f3 d = mk3(rd.x, rd.y, rd.z);
  float tmin = ro.w, tmax = rd.w;
  moved[i] = rebase_ray(sv, o, d, tmin, tmax);
  float4* op = reinterpret_cast<float4*>(out + i);
  op[0] = make_float4(o.x, o.y, o.z, tmin); op[1] = make_float4(rd.x, rd.y, rd.z, tmax);
}
__global__ void __launch_bounds__(256) k_unbase_hits(hala_hit* __restrict__ hits, const float* __restrict__ moved, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float* t = reinterpret_cast<float*>(hits + i);
  if (reinterpret_cast<const uint32_t*>(t)[3] != kAbsent) *t = *t + moved[i];
}
void launch_rebase_batch(const SceneView& sv, const hala_ray* rays, hala_ray* out, float* moved, uint32_t n, hipStream_t s) {
  hipLaunchKernelGGL(k_rebase_batch, dim3(blocks_for(n, 256)), dim3(256), 0, s, sv, rays, out, moved, n);
}
void launch_unbase_hits(hala_hit* hits, const float* moved, uint32_t n, hipStream_t s) {
  hipLaunchKernelGGL(k_unbase_hits, dim3(blocks_for(n, 256)), dim3(256), 0, s, hits, moved, n);
}

}  // namespace rt
