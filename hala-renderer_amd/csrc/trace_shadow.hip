// trace_shadow.hip — the any-hit traversal of the wavefront path tracer's NEE connections, alone and fused with the next bounce's
// closest-hit pass (trace_closest.hip has the frame's kernel sequence).
#include "trace_loop.h"
#include "variants.h"

namespace rt {
// ---------------------------------------------------------------------------------------------------------
// K5c: shadow traversal of the NEE connections of one bounce; unoccluded contributions are added to the
// path's radiance in the fixed order light, environment (RENDER_SPEC §6)
// ---------------------------------------------------------------------------------------------------------
template <bool COUNT, bool STAGED, bool ALPHA, bool INST, bool GROUPS>
__global__ void __launch_bounds__(kTraverseThreads, STAGED ? kTraverseWavesPerSimdStaged : kTraverseWavesPerSimd)
k_trace_shadow(SceneView sv, Queues q, PathState ps, Control* __restrict__ ctl, uint32_t depth, uint32_t kind, uint2* __restrict__ spill_base,
               uint32_t refill) {
  const TraverseLds lds = stage_bvh<STAGED, INST>(sv, g_smem);
  const uint32_t n = ctl->sizes.n_shadow[kind][depth];
  uint2* spill = lane_spill(spill_base);
  StepCounters sc;
  auto src = shadow_source<ALPHA, GROUPS>(q, ps, kind);
  persistent_trace<true, COUNT, STAGED, ALPHA, INST>(sv, lds, spill, &ctl->work_shadow[kind], n, refill, src, sc);
  if (COUNT) flush_counters(ctl, 1, sc);
}

// ---------------------------------------------------------------------------------------------------------
// K5c + K5a in one launch: the shadow passes of bounce d and the closest-hit traversal of bounce d + 1.  They are independent (a light
// connection only adds to its path's L, an environment connection to its Le, the closest-hit pass only reads the ray queue shade(d)
// wrote) and every persistent launch ends in a tail of a few long rays during which most of the chip idles — a fixed cost that weighs
// more the smaller the launch (late bounces, a rank's share of a strong-scaled frame; 10-20 % of the wave slots of a configs[3] launch).
// Here a wave that finds one queue dry moves straight on to the next: one tail instead of three.  (Launches side by side on two streams
// do not achieve this: each takes the chip from the other all the time, profiles/r02_experiments.txt.)  Not used by updates that carry
// per-launch timing events or counting kernels.
// Roles: a wave leaves a queue only when its last ray has ended, so when all workgroups walk the queues in one order every wave of the
// grid drains at the moment a queue runs dry, twice in mid-launch, with ever fewer live lanes.  The queues are independent and handed
// out from shared counters, so any workgroup may take them in any order: a workgroup STARTS on the queue of its role (light, environment
// or closest hit; own stage first, then the others) and the roles are dealt in proportion to the work each queue holds, so that the
// three queues run dry together near the launch's end and most waves never drain before its tail.  configs[3]: fused launch 4.57 ->
// 4.29 ms per frame, frame 7.56 -> 7.35 ms; two roles (any hit / closest hit) gain about half of that (profiles/fused_roles.txt).
// ---------------------------------------------------------------------------------------------------------
#ifndef RT_FUSED_ROLES
#define RT_FUSED_ROLES 3  // tuning builds: 0 = every workgroup takes the queues in the order light, environment, closest; 2 = two roles (any hit, closest hit)
#endif
// What a ray of each kind costs the chip, in ps: the time of the launches that trace only that kind, each with the chip to itself, divided
// by their rays (bench.py on configs[3] with every workgroup on one order, its two frames with one launch per pass: roofline.unfused_kernels,
// 1000 / grays_per_s_in_kernel: batch 152.3 and 153.7, shadow 128.4 and 129.7 in two runs).  Only the ratio (1.19) matters: the frame is the same to
// 0.01 ms from 0.89 to 1.3, 0.02 - 0.06 ms shorter near 1.6 and 0.09 ms longer at 2.0 (profiles/fused_roles.txt): kept as measured, not fitted.
#ifndef RT_ROLE_COST_CLOSEST
#define RT_ROLE_COST_CLOSEST 153.0f
#endif
#ifndef RT_ROLE_COST_ANY
#define RT_ROLE_COST_ANY 129.0f
#endif
constexpr uint32_t kRoleGroup = 16;  // consecutive workgroups that share a role: one per work shard (work_begin), two per XCD
// The stage a workgroup starts on: 0 light connections, 1 environment connections, 2 closest hit.  Groups of kRoleGroup workgroups take
// the roles in proportion to the work each queue holds (rays x cost), every role spread evenly over the grid: a share f of the groups
// is those g at which round(g f) steps.  An empty or absent queue (n == 0) gets no group: role 2 implies a closest-hit queue.  A grid of
// fewer than kRoleGroup workgroups is one group: closest hit if that is half the work or more, else the larger connection queue.
// Wave-uniform; nothing a frame computes depends on the roles: every workgroup visits every stage, and a stage whose queue is dry
// returns through the dry mask.
RT_DI uint32_t fused_role(uint32_t n_light, uint32_t n_env, uint32_t n_closest) {
  const float wl = (float)n_light * RT_ROLE_COST_ANY, we = (float)n_env * RT_ROLE_COST_ANY, wc = (float)n_closest * RT_ROLE_COST_CLOSEST;
  const float wa = wl + we;
  if (!(wa + wc > 0.0f)) return 0u;
  const uint32_t g = blockIdx.x / kRoleGroup;
  const float fc = wc / (wa + wc);
  const uint32_t c0 = (uint32_t)((float)g * fc + 0.5f), c1 = (uint32_t)((float)(g + 1u) * fc + 0.5f);
  if (c1 != c0) return 2u;
  if (RT_FUSED_ROLES == 2 || !(wa > 0.0f)) return 0u;
  const uint32_t a = g - c0;  // this group's rank among the any-hit groups
  const float fl = wl / wa;
  return (uint32_t)((float)(a + 1u) * fl + 0.5f) != (uint32_t)((float)a * fl + 0.5f) ? 0u : 1u;
}

template <bool STAGED, bool ALPHA, bool INST, bool GROUPS>
__global__ void __launch_bounds__(kTraverseThreads, STAGED ? kTraverseWavesPerSimdStaged : kTraverseWavesPerSimd)
k_trace_shadow_then_batch(SceneView sv, const Tri* __restrict__ tris_any, Queues q, PathState ps, Control* __restrict__ ctl, uint32_t depth,
                          uint32_t kinds, const hala_ray* __restrict__ rays, hala_hit* __restrict__ hits, uint2* __restrict__ spill_base, uint32_t refill) {
  const TraverseLds lds = stage_bvh<STAGED, INST>(sv, g_smem);
  uint2* spill = lane_spill(spill_base);
  StepCounters sc;
#if RT_FUSED_ROLES
  const uint32_t n_light = (kinds & 1u) ? ctl->sizes.n_shadow[0][depth] : 0u, n_env = (kinds & 2u) ? ctl->sizes.n_shadow[1][depth] : 0u;
  const uint32_t n_closest = rays != nullptr ? ctl->sizes.n_active[depth + 1u] : 0u;
  const uint32_t role = lane0_u32(fused_role(n_light, n_env, n_closest));
  auto closest = [&]() {
    const uint32_t n = ctl->sizes.n_active[depth + 1u];
    if (blockIdx.x == 0 && threadIdx.x == 0) ctl->totals.rays_closest += n;
    BatchSource src{rays, hits, false, true, STAGED && refill == 64u};
    persistent_trace<false, false, STAGED, false, INST>(sv, lds, spill, &ctl->work_closest, n, refill, src, sc);
  };
  if (role == 2u) closest();  // three inlined wave loops, one after the other: a loop over the stages keeps registers live across them (scratch in the ALPHA variants)
  {
    SceneView sva = sv;
    sva.tris = tris_any;  // RENDER_SPEC 7.1d (STAGED: the launcher only fuses when both passes traverse the same triangles)
    for (uint32_t i = 0; i < 2u; ++i) {
      const uint32_t kind = i ^ (role & 1u);  // bit 0 of kinds: light connections, bit 1: environment connections
      if (!((kinds >> kind) & 1u)) continue;
      auto src = shadow_source<ALPHA, GROUPS>(q, ps, kind);
      persistent_trace<true, false, STAGED, ALPHA, INST>(sva, lds, spill, &ctl->work_shadow[kind], ctl->sizes.n_shadow[kind][depth], refill, src, sc);
    }
  }
  if (role != 2u && rays != nullptr) closest();
#else
  {
    SceneView sva = sv;
    sva.tris = tris_any;  // RENDER_SPEC 7.1d (STAGED: the launcher only fuses when both passes traverse the same triangles)
    for (uint32_t kind = 0; kind < 2u; ++kind) {  // bit 0: light connections, bit 1: environment connections
      if (!((kinds >> kind) & 1u)) continue;
      auto src = shadow_source<ALPHA, GROUPS>(q, ps, kind);
      persistent_trace<true, false, STAGED, ALPHA, INST>(sva, lds, spill, &ctl->work_shadow[kind], ctl->sizes.n_shadow[kind][depth], refill, src, sc);
    }
  }
  if (rays == nullptr) return;  // the last bounce: its two shadow passes share the launch, no closest-hit pass follows
  const uint32_t n = ctl->sizes.n_active[depth + 1u];
  if (blockIdx.x == 0 && threadIdx.x == 0) ctl->totals.rays_closest += n;
  BatchSource src{rays, hits, false, true, STAGED && refill == 64u};
  persistent_trace<false, false, STAGED, false, INST>(sv, lds, spill, &ctl->work_closest, n, refill, src, sc);
#endif
}
uint32_t trace_shadow_blocks_per_cu(size_t dynamic_lds_bytes, TreeForm tree) {
  return tree_blocks_per_cu([](auto STAGED, auto INST) { return k_trace_shadow<false, STAGED, false, INST, false>; }, tree, kTraverseThreads, dynamic_lds_bytes);
}

void launch_trace_shadow(const LaunchCfg& lc, const SceneView& sv0, const Queues& q, const PathState& ps, Control* ctl, uint32_t depth,
                         uint32_t kind, bool count, hipStream_t s) {
  SceneView sv = sv0;
  sv.tris = sv0.tris_any;  // RENDER_SPEC 7.1d: shadow rays traverse the copy in which invisible surfaces are degenerate and translucent ones flagged
  const TreeForm tree = tree_form(sv);
  // light groups (RENDER_SPEC §14): only the light connections carry a group
  dispatch<kFamilyTraceShadow>([&](auto COUNT, auto ALPHA, auto STAGED, auto INST, auto GROUPS) {
    hipLaunchKernelGGL((k_trace_shadow<COUNT, STAGED, ALPHA, INST, GROUPS>), dim3(lc.persistent_blocks), dim3(kTraverseThreads), lc.smem, s, sv, q, ps,
                       ctl, depth, kind, lc.spill, lc.refill);
  }, count, sv.any_translucent != 0u, tree == TreeForm::Staged, tree == TreeForm::TwoLevel, kind == 0u && ps.groups != nullptr);
}

// the fused launch; false: the caller must issue the two launches separately (an LDS-staged scene whose any-hit rays traverse a
// different triangle copy than its closest-hit rays: only one of them is staged)
bool launch_trace_shadow_then_batch(const LaunchCfg& lc, const SceneView& sv, const Queues& q, const PathState& ps, Control* ctl, uint32_t depth,
                                    uint32_t kinds, bool with_closest, hipStream_t s) {
  const TreeForm tree = tree_form(sv);
  if (tree == TreeForm::Staged && sv.tris_any != sv.tris) return false;
  const hala_ray* rays = with_closest ? q.rays[(depth + 1u) & 1u] : nullptr;
  dispatch<kFamilyTraceShadowThenBatch>([&](auto ALPHA, auto STAGED, auto INST, auto GROUPS) {
    hipLaunchKernelGGL((k_trace_shadow_then_batch<STAGED, ALPHA, INST, GROUPS>), dim3(lc.persistent_blocks), dim3(kTraverseThreads), lc.smem, s, sv,
                       sv.tris_any, q, ps, ctl, depth, kinds, rays, q.hits, lc.spill, lc.refill);
  }, sv.any_translucent != 0u, tree == TreeForm::Staged, tree == TreeForm::TwoLevel, (kinds & 1u) != 0u && ps.groups != nullptr);
  return true;
}

}  // namespace rt
