// point_query.h — what a point asks of the tree (RENDER_SPEC 4.8), shared by closest_point.hip and distance_grid.hip (4.9): the state of
// a query, Ericson's closest point on a triangle in the pinned arithmetic of 4.8, the child test with the point-to-box squared distance
// as the key, and the per-lane node visit.  Both units run these instructions, so a voxel of a distance grid and a query of a batch at
// the same point get the same bits.
#pragma once
#include "trace_loop.h"

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

}  // namespace rt
