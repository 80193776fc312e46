// closest_point.hip — closest-point query batches (RENDER_SPEC 4.8): for every point of a batch, the nearest point of the scene's surface
// within the query's radius.  One persistent kernel in the two one-level tree forms (LDS-staged, large), over the dequeue of trace_loop.h
// (work_begin / work_take, ballot-rank refill) and the blocks of traverse.h that do not depend on a ray: the LDS layout (stage_bvh), the
// per-lane stack with its spill (LaneStack), the key sort (sort2kv, key_tn).  What a point needs instead of a ray is in point_query.h,
// shared with the distance grids of distance_grid.hip: the node dequantisation with the point-to-box squared distance as the key, and
// Ericson's closest point on a triangle in the pinned arithmetic of 4.8.  The limit a query culls with is its best squared distance so far, starting from radius * radius; every comparison of a box key
// with it carries the multiplicative slack of 4.8 (kCullSlack), which together with the builders' box pad makes the culling conservative
// with respect to the triangles' own rounded distances.  Leaves are tested by the lane itself in both forms.
// Not one of the flag-dispatched families of variants.h: launched like the multi-hit kernel (tree_form, tree_blocks_per_cu, with_flags).
#include <algorithm>

#include "point_query.h"
#include "variants.h"

namespace rt {

RT_DI void point_begin(PointTrav& t, float4 q, uint32_t idx) {
  t.p = mk3(q.x, q.y, q.z);
  t.r2 = q.w >= 0.0f ? q.w * q.w : -1.0f;  // a NaN or negative radius admits nothing (dd <= -1 never holds)
  t.limit = t.r2;
  t.best = ~0ull; t.u = 0.0f; t.v = 0.0f; t.qx = 0.0f; t.qy = 0.0f; t.qz = 0.0f; t.region = 0u;
  t.idx = idx; t.cur = 0u; t.sp = 0;
}
RT_DI void point_done(const PointTrav& t, float4* out) {
  const bool found = t.best != ~0ull;
  const float dd = __uint_as_float((uint32_t)(t.best >> 32));
  float4* o = out + (size_t)t.idx * 2;
  o[0] = found ? make_float4(sqrt_rn(dd), t.u, t.v, __uint_as_float((uint32_t)t.best)) : make_float4(-1.0f, 0.0f, 0.0f, __uint_as_float(kAbsent));
  o[1] = found ? make_float4(t.qx, t.qy, t.qz, __uint_as_float(t.region)) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// The persistent loop of trace_multi.hip around point_step: the sharded dequeue and the ballot-rank refill of trace_loop.h.  A finished
// query writes its 32-B record at once.  COUNT: node visits and triangle tests are summed per wave and added to counters[0], [1].
// (The counting large form spilled 6 registers to scratch at the 96 of 5 waves per SIMD: it is built for 4.  It counts, it is not timed.)
template <bool STAGED, bool COUNT>
__global__ void __launch_bounds__(kTraverseThreads, (STAGED || COUNT) ? kTraverseWavesPerSimdStaged : kTraverseWavesPerSimd)
k_closest_point(SceneView sv, const float4* __restrict__ queries, float4* __restrict__ out, uint32_t n, WorkCounters* __restrict__ work,
                uint2* __restrict__ spill_base, uint32_t refill, unsigned long long* __restrict__ counters) {
  const TraverseLds lds = stage_bvh<STAGED, false>(sv, g_smem);  // (the large form's leaf work lists are not used here and not allocated)
  uint2* spill = lane_spill(spill_base);
  WorkCursor cur = work_begin(n);
  bool more = n > 0u;  // wave-uniform
  bool has = false;
  uint32_t n_nodes = 0u, n_tris = 0u;
  PointTrav t;
  for (;;) {
    const unsigned long long idle = __ballot(!has);
    if (more && idle) {
      uint32_t got = 0;
      const uint32_t base = work_take(work, cur, n, (uint32_t)__popcll(idle), &got);
      if (base == kAbsent) more = false;
      else if (!has) {
        const uint32_t rank = (uint32_t)__popcll(idle & ((1ull << lane_id()) - 1ull));
        if (rank < got) {
          const uint32_t idx = base + rank;
          point_begin(t, queries[idx], idx);
          has = true;
        }
      }
    }
    if (__ballot(has) == 0ull) { if (!more) break; continue; }
    for (;;) {
      if (has && point_step<STAGED, COUNT>(sv, lds, spill, t, n_nodes, n_tris)) { point_done(t, out); has = false; }
      const uint32_t nidle = (uint32_t)__popcll(__ballot(!has));
      if (nidle == 64u || (more && nidle >= refill)) break;
    }
  }
  if (COUNT) {
    const uint32_t a = wave_sum(n_nodes), b = wave_sum(n_tris);
    if (lane_id() == 0u) { atomicAdd(&counters[0], (unsigned long long)a); atomicAdd(&counters[1], (unsigned long long)b); }
  }
}

bool launch_closest_point(const LaunchCfg& lc, const SceneView& sv, uint32_t cu_count, const hala_point_query* queries, hala_closest_point* out,
                          uint32_t n, WorkCounters* work, unsigned long long* counters, hipStream_t s) {
  const TreeForm tree = tree_form(sv);
  if (tree == TreeForm::TwoLevel) return false;
  const size_t smem = query_lds_bytes(sv, tree, kTraverseThreads);
  const uint32_t per_cu = counted_blocks_per_cu([](auto STAGED, auto COUNT) { return k_closest_point<STAGED, COUNT>; }, counters != nullptr, tree, kTraverseThreads, smem);
  if (per_cu == 0u) return false;
  const uint32_t blocks = query_blocks(lc, cu_count, per_cu);
  with_flags([&](auto STAGED, auto COUNT) {
    hipLaunchKernelGGL((k_closest_point<STAGED, COUNT>), dim3(blocks), dim3(kTraverseThreads), smem, s, sv, reinterpret_cast<const float4*>(queries),
                       reinterpret_cast<float4*>(out), n, work, lc.spill, lc.refill, counters);
  }, tree == TreeForm::Staged, counters != nullptr);
  return true;
}

}  // namespace rt
