// closest_point.hip — closest-point query batches (RENDER_SPEC 4.8): for every point of a batch, the nearest point of the scene's surface
// within the query's radius.  One persistent kernel in the two one-level tree forms (LDS-staged, large), over the dequeue of trace_loop.h
// (work_begin / work_take, ballot-rank refill) and the blocks of traverse.h that do not depend on a ray: the LDS layout (stage_bvh), the
// per-lane stack with its spill (LaneStack), the key sort (sort2kv, key_tn).  What a point needs instead of a ray is here: the node
// dequantisation with the point-to-box squared distance as the key, and Ericson's closest point on a triangle in the pinned arithmetic of
// 4.8.  The limit a query culls with is its best squared distance so far, starting from radius * radius; every comparison of a box key
// with it carries the multiplicative slack of 4.8 (kCullSlack), which together with the builders' box pad makes the culling conservative
// with respect to the triangles' own rounded distances.  Leaves are tested by the lane itself in both forms.
// Not one of the flag-dispatched families of variants.h: launched like the multi-hit kernel (tree_form, tree_blocks_per_cu, with_flags).
#include <algorithm>

#include "trace_loop.h"
#include "variants.h"

namespace rt {

// RENDER_SPEC 4.8, conservative culling: a box is in reach while key * (1 - 2^-16) <= limit
#ifndef RT_POINT_CULL_SLACK
#define RT_POINT_CULL_SLACK 0.9999847412109375f  // tuning builds: 1.0f = no slack (DESIGN.md 27 has the node visits it costs)
#endif
constexpr float kCullSlack = RT_POINT_CULL_SLACK;

struct PointTrav {
  f3 p;
  float r2;                 // radius * radius, or -1 for a radius that admits nothing: what a triangle's dd is accepted against
  float limit;              // what box keys are culled with: min(r2, the best dd so far)
  unsigned long long best;  // bits(dd) << 32 | id of the answer so far; all ones: none
  float u, v, qx, qy, qz;
  uint32_t region;
  uint32_t idx, cur;
  int sp;
};
RT_DI void point_begin(PointTrav& t, float4 q, uint32_t idx) {
  t.p = mk3(q.x, q.y, q.z);
  t.r2 = q.w >= 0.0f ? q.w * q.w : -1.0f;  // a NaN or negative radius admits nothing (dd <= -1 never holds)
  t.limit = t.r2;
  t.best = ~0ull; t.u = 0.0f; t.v = 0.0f; t.qx = 0.0f; t.qy = 0.0f; t.qz = 0.0f; t.region = 0u;
  t.idx = idx; t.cur = 0u; t.sp = 0;
}

// RENDER_SPEC 4.8, per triangle: Ericson's closest point, the region tests in the spec's order; every operation is a single IEEE one
// (the unit is compiled without contraction), the only fmas are those of dot (2.1) and of q.
RT_DI void point_offer(PointTrav& t, float4 a, float4 b, float4 c, uint32_t id) {
  const f3 v0 = mk3(a.x, a.y, a.z), e1 = mk3(b.x, b.y, b.z), e2 = mk3(c.x, c.y, c.z);
  const f3 ap = t.p - v0, bp = ap - e1, cp = ap - e2;
  const float d1 = dot3(e1, ap), d2 = dot3(e2, ap), d3 = dot3(e1, bp), d4 = dot3(e2, bp), d5 = dot3(e1, cp), d6 = dot3(e2, cp);
  const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  const float bc0 = d4 - d3, bc1 = d5 - d6;
  float u, v;
  uint32_t region;
  if (d1 <= 0.0f && d2 <= 0.0f) { u = 0.0f; v = 0.0f; region = 4u; }
  else if (d3 >= 0.0f && d4 <= d3) { u = 1.0f; v = 0.0f; region = 5u; }
  else if (d6 >= 0.0f && d5 <= d6) { u = 0.0f; v = 1.0f; region = 6u; }
  else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { u = d1 / (d1 - d3); v = 0.0f; region = 1u; }
  else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) { u = 0.0f; v = d2 / (d2 - d6); region = 2u; }
  else if (va <= 0.0f && bc0 >= 0.0f && bc1 >= 0.0f) { v = bc0 / (bc0 + bc1); u = 1.0f - v; region = 3u; }
  else { const float den = 1.0f / ((va + vb) + vc); u = vb * den; v = vc * den; region = 0u; }
  const float qx = __fmaf_rn(v, e2.x, __fmaf_rn(u, e1.x, v0.x)), qy = __fmaf_rn(v, e2.y, __fmaf_rn(u, e1.y, v0.y)),
              qz = __fmaf_rn(v, e2.z, __fmaf_rn(u, e1.z, v0.z));
  const f3 r = mk3(t.p.x - qx, t.p.y - qy, t.p.z - qz);
  const float dd = dot3(r, r);
  // dd >= +0 or NaN: the bits of an accepted dd order like dd; a NaN fails the first comparison
  const unsigned long long key = ((unsigned long long)__float_as_uint(dd) << 32) | (unsigned long long)id;
  if (dd <= t.r2 && key < t.best) {
    t.best = key; t.limit = dd; t.u = u; t.v = v; t.qx = qx; t.qy = qy; t.qz = qz; t.region = region;
  }
}
RT_DI void point_done(const PointTrav& t, float4* out) {
  const bool found = t.best != ~0ull;
  const float dd = __uint_as_float((uint32_t)(t.best >> 32));
  float4* o = out + (size_t)t.idx * 2;
  o[0] = found ? make_float4(sqrt_rn(dd), t.u, t.v, __uint_as_float((uint32_t)t.best)) : make_float4(-1.0f, 0.0f, 0.0f, __uint_as_float(kAbsent));
  o[1] = found ? make_float4(t.qx, t.qy, t.qz, __uint_as_float(t.region)) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// The child test of a point: the planes of the four children dequantised (4.1b: pmin + q * 2^e, one fma each), per axis the distance
// max(lo - p, p - hi, 0), the squared distance as the key.  ref / key come back sorted as test_children sorts them: the leaves in reach
// first, nearest first, then the inner children in reach, nearest first, then the rest (kMissKey).  A key is a non-negative float with
// the child slot in its two low mantissa bits (key_tn rounds it down: conservative) and the sign bit set for inner children.
template <bool STAGED>
RT_DI void point_children(const SceneView& sv, const TraverseLds& lds, const f3& p, uint32_t node, float limit, uint32_t (&ref)[4], uint32_t (&key)[4]) {
  float4 q0, q1, q2, q3;
  if (STAGED) { const RT_LDS f32x4* n = lds.nodes + (size_t)node * 4; q0 = ld4(n); q1 = ld4(n + 1); q2 = ld4(n + 2); q3 = ld4(n + 3); }
  else { const float4* n = reinterpret_cast<const float4*>(sv.nodes) + (size_t)node * 4; q0 = n[0]; q1 = n[1]; q2 = n[2]; q3 = n[3]; }
  const uint32_t ex = __float_as_uint(q0.w);
  const float sx = __uint_as_float((ex & 0xffu) << 23), sy = __uint_as_float(((ex >> 8) & 0xffu) << 23), sz = __uint_as_float(((ex >> 16) & 0xffu) << 23);
  const uint32_t lox = __float_as_uint(q1.x), loy = __float_as_uint(q1.y), loz = __float_as_uint(q1.z);
  const uint32_t hix = __float_as_uint(q1.w), hiy = __float_as_uint(q2.x), hiz = __float_as_uint(q2.y);
  ref[0] = __float_as_uint(q3.x); ref[1] = __float_as_uint(q3.y); ref[2] = __float_as_uint(q3.z); ref[3] = __float_as_uint(q3.w);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float dx = hw_maxf(hw_maxf(__fmaf_rn(ubyte_f32(lox, c), sx, q0.x) - p.x, p.x - __fmaf_rn(ubyte_f32(hix, c), sx, q0.x)), 0.0f);
    const float dy = hw_maxf(hw_maxf(__fmaf_rn(ubyte_f32(loy, c), sy, q0.y) - p.y, p.y - __fmaf_rn(ubyte_f32(hiy, c), sy, q0.y)), 0.0f);
    const float dz = hw_maxf(hw_maxf(__fmaf_rn(ubyte_f32(loz, c), sz, q0.z) - p.z, p.z - __fmaf_rn(ubyte_f32(hiz, c), sz, q0.z)), 0.0f);
    const float k = __fmaf_rn(dz, dz, __fmaf_rn(dy, dy, dx * dx));
    const bool hit = ref[c] != kAbsent && k * kCullSlack <= limit;
    key[c] = hit ? ((__float_as_uint(k) & 0x7ffffffcu) | (uint32_t)c | (~ref[c] & kInnerKey)) : kMissKey;
  }
  sort2kv(key[0], key[1], ref[0], ref[1]); sort2kv(key[2], key[3], ref[2], ref[3]); sort2kv(key[0], key[2], ref[0], ref[2]);
  sort2kv(key[1], key[3], ref[1], ref[3]); sort2kv(key[1], key[2], ref[1], ref[2]);
}
RT_DI bool in_reach(uint32_t key, float limit) { return key_tn(key) * kCullSlack <= limit; }

// One node visit of a lane that holds a query; true when the query is finished.  The order is that of the ray steppers: the leaves in
// reach are tested by the lane itself, nearest first, then the nearest inner child is visited and the others wait on the stack with
// their keys; pops are culled against the limit as it stands then.
template <bool STAGED, bool COUNT>
RT_DI bool point_step(const SceneView& sv, const TraverseLds& lds, uint2* spill, PointTrav& t, uint32_t& n_nodes, uint32_t& n_tris) {
  LaneStack<STAGED, false> st{lds.stack + threadIdx.x, spill, t.sp};
  uint32_t ref[4], key[4];
  point_children<STAGED>(sv, lds, t.p, t.cur, t.limit, ref, key);
  if (COUNT) ++n_nodes;
  bool in[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) in[c] = (int32_t)key[c] < -1;
#pragma unroll
  for (int c = 3; c >= 1; --c) {
    const bool left = c == 3 ? (in[0] | in[1] | in[2]) : (c == 2 ? (in[0] | in[1]) : in[0]);
    if (in[c] & left) st.push(key[c], ref[c]);
  }
  uint32_t next = in[0] ? ref[0] : (in[1] ? ref[1] : (in[2] ? ref[2] : (in[3] ? ref[3] : kAbsent)));
  const uint32_t next_key = in[0] ? key[0] : (in[1] ? key[1] : (in[2] ? key[2] : key[3]));
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    if ((int32_t)key[c] < 0) break;          // a sorted prefix: leaf keys have the sign bit clear
    if (!in_reach(key[c], t.limit)) break;  // a nearer leaf may have lowered the limit: everything behind is out of reach
    const uint32_t first = ref[c] & 0x0fffffffu, count = ((ref[c] >> 28) & 7u) + 1u;
    for (uint32_t i = 0; i < count; ++i) {
      float4 a, b, c2;
      if (STAGED) { const RT_LDS f32x4* tp = lds.tris + (size_t)(first + i) * 3; a = ld4(tp); b = ld4(tp + 1); c2 = ld4(tp + 2); }
      else { const float4* tp = reinterpret_cast<const float4*>(sv.tris) + (size_t)(first + i) * 3; a = tp[0]; b = tp[1]; c2 = tp[2]; }
      point_offer(t, a, b, c2, __float_as_uint(a.w));
    }
    if (COUNT) n_tris += count;
  }
  if (next != kAbsent && !in_reach(next_key, t.limit)) next = kAbsent;
  while (next == kAbsent) {
    if (st.sp == 0) return true;
    const uint2 e = st.pop();
    if (in_reach(e.x, t.limit)) next = e.y;
  }
  t.cur = next;
  t.sp = st.sp;
  return false;
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

// The kernel's own LDS: the per-lane stacks, and a staged tree behind them
static size_t point_lds_bytes(const SceneView& sv, TreeForm tree) {
  const size_t stacks = (size_t)traverse_stack_lds_levels(tree) * kTraverseThreads * 8;
  return tree == TreeForm::Staged ? stacks + (size_t)sv.lds_nodes * 64 + (size_t)sv.lds_tris * 48 : stacks;
}
bool launch_closest_point(const LaunchCfg& lc, const SceneView& sv, uint32_t cu_count, const hala_point_query* queries, hala_closest_point* out,
                          uint32_t n, WorkCounters* work, unsigned long long* counters, hipStream_t s) {
  const TreeForm tree = tree_form(sv);
  if (tree == TreeForm::TwoLevel) return false;
  const size_t smem = point_lds_bytes(sv, tree);
  const uint32_t per_cu = counters ? tree_blocks_per_cu([](auto STAGED, auto) { return k_closest_point<STAGED, true>; }, tree, kTraverseThreads, smem)
                                  : tree_blocks_per_cu([](auto STAGED, auto) { return k_closest_point<STAGED, false>; }, tree, kTraverseThreads, smem);
  if (per_cu == 0u) return false;
  // the spill area holds one slice per lane of lc.persistent_blocks workgroups: never a larger grid than that
  const uint32_t blocks = std::min(lc.persistent_blocks, cu_count * std::min(per_cu, 8u));
  with_flags([&](auto STAGED, auto COUNT) {
    hipLaunchKernelGGL((k_closest_point<STAGED, COUNT>), dim3(blocks), dim3(kTraverseThreads), smem, s, sv, reinterpret_cast<const float4*>(queries),
                       reinterpret_cast<float4*>(out), n, work, lc.spill, lc.refill, counters);
  }, tree == TreeForm::Staged, counters != nullptr);
  return true;
}

}  // namespace rt
