// distance_grid.hip — signed distance grids (RENDER_SPEC 4.9): the scene's distance field on a voxel grid.  The distance of a voxel is
// the closest-point answer of 4.8 at the voxel's point with the grid's band as the radius, computed by the per-triangle and per-node
// instructions of point_query.h, the ones k_closest_point runs: the same bits.  Two distance kernels, both persistent, both in the two
// one-level tree forms (LDS-staged as stage_bvh lays the tree out, large from memory):
//   method 1, per lane — the loop of k_closest_point; the voxels are dequeued in 4 x 4 x 4 brick order, so a wave holds 64 neighbours;
//   method 2, per wave — one wave owns one brick and walks the tree ONCE for its 64 points: node and triangle records are fetched from
//     a wave-uniform address, every lane computes its own child keys, a child is entered if any lane is in reach (ballot), nearest
//     first by the wave-minimum key, one stack per wave in LDS; pops are culled with min key * slack <= max limit over the lanes that
//     hold a point; in a leaf every lane offers itself every triangle.  A lane is offered triangles it did not need, which cannot
//     change its answer (the order of (bits(dd), id) is total), and never misses one it needs (4.9: the wave test is implied by a
//     lane's own).
// The sign (flags bit 0) is the parity of the crossings of the voxel's row, a ray along +x from voxel (0, j, k): one lane owns one row,
// walks the tree with the ray steppers' node test under a limit that never shrinks, and toggles one bit per accepted hit in the row's
// (nx + 1)-bit array; when the row is done the lane turns the toggles into suffix parities, which the distance kernels read as they
// store.  Not one of the flag-dispatched families of variants.h: launched like the closest-point kernel.
#include <algorithm>

#include "point_query.h"
#include "variants.h"

namespace rt {

RT_DI f3 voxel_point(const GridView& g, uint32_t x, uint32_t y, uint32_t z) {  // 4.9: one fma per axis
  return mk3(__fmaf_rn((float)x, g.spacing, g.origin[0]), __fmaf_rn((float)y, g.spacing, g.origin[1]), __fmaf_rn((float)z, g.spacing, g.origin[2]));
}
// The query (p, band) of 4.8 at voxel (x, y, z); the lane keeps the voxel in t.idx, 10 bits per axis (dims <= 1024)
RT_DI void grid_begin(PointTrav& t, const GridView& g, uint32_t x, uint32_t y, uint32_t z) {
  t.p = voxel_point(g, x, y, z);
  t.r2 = g.band >= 0.0f ? g.band * g.band : -1.0f;
  t.limit = t.r2;
  t.best = ~0ull; t.u = 0.0f; t.v = 0.0f; t.qx = 0.0f; t.qy = 0.0f; t.qz = 0.0f; t.region = 0u;
  t.idx = x | (y << 10) | (z << 20); t.cur = 0u; t.sp = 0;
}
// 4.9: the distance of the answer, or the band where there is none; inside (bit x + 1 of the row's suffix parities) flips the sign bit
RT_DI void grid_store(const GridView& g, const PointTrav& t, float* distance, uint32_t* prim, const uint32_t* inside) {
  const uint32_t x = t.idx & 1023u, y = (t.idx >> 10) & 1023u, z = t.idx >> 20;
  const bool found = t.best != ~0ull;
  uint32_t d = __float_as_uint(found ? sqrt_rn(__uint_as_float((uint32_t)(t.best >> 32))) : g.band);
  const size_t row = (size_t)z * g.ny + y;
  if (inside) {
    const uint32_t b = x + 1u;
    d ^= ((inside[row * g.words + (b >> 5)] >> (b & 31u)) & 1u) << 31;
  }
  const size_t at = row * g.nx + x;
  distance[at] = __uint_as_float(d);
  if (prim) prim[at] = found ? (uint32_t)t.best : kAbsent;
}
RT_DI void grid_bricks(const GridView& g, uint32_t& nbx, uint32_t& nby, uint32_t& nbz) { nbx = (g.nx + 3u) >> 2; nby = (g.ny + 3u) >> 2; nbz = (g.nz + 3u) >> 2; }
// counting launches: one set of atomics per wave
RT_DI void grid_count(unsigned long long* counters, int at, uint32_t a, uint32_t b) {
  const uint32_t sa = wave_sum(a), sb = wave_sum(b);
  if (lane_id() == 0u) { atomicAdd(&counters[at], (unsigned long long)sa); atomicAdd(&counters[at + 1], (unsigned long long)sb); }
}

// ---- method 1: one voxel per lane ------------------------------------------------------------------------------------------------------
// The persistent loop of k_closest_point around point_step.  Queue entry i is lane i % 64 of brick i / 64 (x = lane & 3, y = (lane >> 2)
// & 3, z = lane >> 4): a wave's first fill is one brick, and what it refills with are the neighbours of what it holds.  An entry beyond
// the grid's dims holds no voxel.  COUNT: counters[0] += node visits, [1] += triangle tests, each of one lane.
template <bool STAGED, bool COUNT>
__global__ void __launch_bounds__(kTraverseThreads, (STAGED || COUNT) ? kTraverseWavesPerSimdStaged : kTraverseWavesPerSimd)
k_grid_lane(SceneView sv, GridView g, float* __restrict__ distance, uint32_t* __restrict__ prim, const uint32_t* __restrict__ inside,
            WorkCounters* __restrict__ work, uint2* __restrict__ spill_base, uint32_t refill, unsigned long long* __restrict__ counters) {
  const TraverseLds lds = stage_bvh<STAGED, false>(sv, g_smem);
  uint2* spill = lane_spill(spill_base);
  uint32_t nbx, nby, nbz;
  grid_bricks(g, nbx, nby, nbz);
  const uint32_t n = nbx * nby * nbz * 64u;  // <= 2^30
  WorkCursor cur = work_begin(n);
  bool more = true;  // wave-uniform
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
          const uint32_t idx = base + rank, brick = idx >> 6, l = idx & 63u;
          const uint32_t x = (brick % nbx) * 4u + (l & 3u), y = ((brick / nbx) % nby) * 4u + ((l >> 2) & 3u), z = (brick / (nbx * nby)) * 4u + (l >> 4);
          if (x < g.nx && y < g.ny && z < g.nz) { grid_begin(t, g, x, y, z); has = true; }
        }
      }
    }
    if (__ballot(has) == 0ull) { if (!more) break; continue; }
    for (;;) {
      if (has && point_step<STAGED, COUNT>(sv, lds, spill, t, n_nodes, n_tris)) { grid_store(g, t, distance, prim, inside); has = false; }
      const uint32_t nidle = (uint32_t)__popcll(__ballot(!has));
      if (nidle == 64u || (more && nidle >= refill)) break;
    }
  }
  if (COUNT) grid_count(counters, 0, n_nodes, n_tris);
}

// ---- method 2: one brick per wave ------------------------------------------------------------------------------------------------------
// Minimum / maximum of an unsigned value over the 64 lanes, wave-uniform (a scalar register).  Every lane of the wave must be active.
// The scan of the wave reductions LLVM emits for gfx9: four row shifts, then lane 15 of a row to the next row and lane 31 to the upper
// half (DPP; a lane without a source keeps its own value), the result in lane 63.
template <int CTRL, int ROWS> RT_DI uint32_t dpp_u32(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, ROWS, 0xf, false); }
template <bool MAX> RT_DI uint32_t wave_pick(uint32_t a, uint32_t b) { return MAX ? max(a, b) : min(a, b); }
template <bool MAX>
RT_DI uint32_t wave_reduce_u32(uint32_t v) {
  v = wave_pick<MAX>(v, dpp_u32<0x111, 0xf>(v));  // row_shr:1
  v = wave_pick<MAX>(v, dpp_u32<0x112, 0xf>(v));  // row_shr:2
  v = wave_pick<MAX>(v, dpp_u32<0x114, 0xf>(v));  // row_shr:4
  v = wave_pick<MAX>(v, dpp_u32<0x118, 0xf>(v));  // row_shr:8
  v = wave_pick<MAX>(v, dpp_u32<0x142, 0xa>(v));  // row_bcast:15 into rows 1 and 3
  v = wave_pick<MAX>(v, dpp_u32<0x143, 0xc>(v));  // row_bcast:31 into rows 2 and 3
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
// what a lane's limit counts in the wave's maximum: its bits (a limit is >= +0 and orders like them); a lane without a point (-1): 0
RT_DI uint32_t limit_bits(float limit) { return limit >= 0.0f ? __float_as_uint(limit) : 0u; }

// One wave, one brick, one walk.  The wave's stack is its quarter of the workgroup's stack area (64 x stack_lds() entries: a walk
// needs at most the tree's own stack need, which the per-lane kernels fit in 64).  Everything that steers the walk — node, keys, refs,
// depth — is wave-uniform and lives in scalar registers; the node index and the leaf's first triangle go through readfirstlane, so the
// fetches have a provably uniform address and are not waterfalled.
// COUNT: counters[0] += node visits x lanes that hold a point, [1] += triangle tests x lanes that hold a point (what method 1 counts:
// the arithmetic of one lane), [4] += nodes fetched by a wave, [5] += triangles fetched by a wave.
template <bool STAGED, bool COUNT>
__global__ void __launch_bounds__(kTraverseThreads, (STAGED || COUNT) ? kTraverseWavesPerSimdStaged : kTraverseWavesPerSimd)
k_grid_brick(SceneView sv, GridView g, float* __restrict__ distance, uint32_t* __restrict__ prim, const uint32_t* __restrict__ inside,
             WorkCounters* __restrict__ work, unsigned long long* __restrict__ counters) {
  const TraverseLds lds = stage_bvh<STAGED, false>(sv, g_smem);
  RT_LDS u32x2* stack = lds.stack + (size_t)(threadIdx.x >> 6) * (64u * (uint32_t)stack_lds<STAGED>());
  uint32_t nbx, nby, nbz;
  grid_bricks(g, nbx, nby, nbz);
  const uint32_t n = nbx * nby * nbz;
  WorkCursor cur = work_begin(n);
  const uint32_t lane = lane_id();
  uint32_t n_nodes = 0u, n_tris = 0u, w_nodes = 0u, w_tris = 0u;
  for (;;) {
    uint32_t got = 0;
    const uint32_t brick = work_take(work, cur, n, 1u, &got);  // wave-uniform
    if (brick == kAbsent) break;
    const uint32_t x = (brick % nbx) * 4u + (lane & 3u), y = ((brick / nbx) % nby) * 4u + ((lane >> 2) & 3u), z = (brick / (nbx * nby)) * 4u + (lane >> 4);
    const bool valid = x < g.nx && y < g.ny && z < g.nz;
    PointTrav t;
    grid_begin(t, g, x & 1023u, y & 1023u, z & 1023u);
    if (!valid) { t.r2 = -1.0f; t.limit = -1.0f; }  // holds no point: in reach of nothing, accepts nothing
    uint32_t maxlim = wave_reduce_u32<true>(limit_bits(t.limit));
    uint32_t node = 0u;
    int sp = 0;
    for (;;) {
      node = lane0_u32(node);
      // every present child with this lane's key (a limit of +inf culls nothing; a NaN key is a miss), then back into slot order
      uint32_t ref[4], key[4];
      point_children<STAGED>(sv, lds, t.p, node, __builtin_inff(), ref, key);
      float4 q3;
      if (STAGED) q3 = ld4(lds.nodes + (size_t)node * 4 + 3); else q3 = reinterpret_cast<const float4*>(sv.nodes)[(size_t)node * 4 + 3];
      uint32_t uref[4] = {lane0_u32(__float_as_uint(q3.x)), lane0_u32(__float_as_uint(q3.y)), lane0_u32(__float_as_uint(q3.z)), lane0_u32(__float_as_uint(q3.w))};
      uint32_t ukey[4];
      if (COUNT) { n_nodes += valid ? 1u : 0u; w_nodes += lane == 0u ? 1u : 0u; }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        uint32_t kb = ~0u;  // this lane's key of child c (key_tn's rounding: conservative); all ones: none, which no limit reaches
#pragma unroll
        for (int e = 0; e < 4; ++e) kb = (valid && key[e] != kMissKey && (key[e] & 3u) == (uint32_t)c) ? (key[e] & 0x7ffffffcu) : kb;
        const bool reach = __uint_as_float(kb) * kCullSlack <= t.limit;
        ukey[c] = kMissKey;
        if (__builtin_amdgcn_ballot_w64(reach) != 0ull) ukey[c] = wave_reduce_u32<false>(kb) | (uint32_t)c | (~uref[c] & kInnerKey);
      }
      sort2kv(ukey[0], ukey[1], uref[0], uref[1]); sort2kv(ukey[2], ukey[3], uref[2], uref[3]); sort2kv(ukey[0], ukey[2], uref[0], uref[2]);
      sort2kv(ukey[1], ukey[3], uref[1], uref[3]); sort2kv(ukey[1], ukey[2], uref[1], uref[2]);
      bool in[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) in[c] = (int32_t)ukey[c] < -1;
#pragma unroll
      for (int c = 3; c >= 1; --c) {
        const bool left = c == 3 ? (in[0] | in[1] | in[2]) : (c == 2 ? (in[0] | in[1]) : in[0]);
        if (in[c] & left) { stack[sp] = u32x2{ukey[c], uref[c]}; ++sp; }
      }
      uint32_t next = in[0] ? uref[0] : (in[1] ? uref[1] : (in[2] ? uref[2] : (in[3] ? uref[3] : kAbsent)));
      const uint32_t next_key = in[0] ? ukey[0] : (in[1] ? ukey[1] : (in[2] ? ukey[2] : ukey[3]));
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if ((int32_t)ukey[c] < 0) break;                              // a sorted prefix: leaf keys have the sign bit clear
        if (!in_reach(ukey[c], __uint_as_float(maxlim))) break;      // nearer leaves may have lowered every lane's limit
        const uint32_t first = lane0_u32(uref[c] & 0x0fffffffu), count = ((uref[c] >> 28) & 7u) + 1u;
        for (uint32_t i = 0; i < count; ++i) {
          float4 a, b, c2;
          if (STAGED) { const RT_LDS f32x4* tp = lds.tris + (size_t)(first + i) * 3; a = ld4(tp); b = ld4(tp + 1); c2 = ld4(tp + 2); }
          else { const float4* tp = reinterpret_cast<const float4*>(sv.tris) + (size_t)(first + i) * 3; a = tp[0]; b = tp[1]; c2 = tp[2]; }
          point_offer(t, a, b, c2, __float_as_uint(a.w));
        }
        if (COUNT) { n_tris += valid ? count : 0u; w_tris += lane == 0u ? count : 0u; }
        maxlim = wave_reduce_u32<true>(limit_bits(t.limit));
      }
      if (next != kAbsent && !in_reach(next_key, __uint_as_float(maxlim))) next = kAbsent;
      while (next == kAbsent && sp != 0) {
        --sp;
        const u32x2 e = stack[sp];
        if (in_reach(lane0_u32(e.x), __uint_as_float(maxlim))) next = lane0_u32(e.y);
      }
      if (next == kAbsent) break;
      node = next;
    }
    if (valid) grid_store(g, t, distance, prim, inside);
  }
  if (COUNT) { grid_count(counters, 0, n_nodes, n_tris); grid_count(counters, 4, w_nodes, w_tris); }
}

// ---- the rows: crossings of the ray along +x from voxel (0, j, k) ---------------------------------------------------------------------
struct RowTrav {
  RayPre r;
  float ts;        // 4.2: how far a far origin was moved; back on every hit's t
  uint32_t* bits;  // the row's (nx + 1)-bit array
  uint32_t cur;
  int sp;
};
// An accepted hit at distance t from the row's origin lies beyond the voxels with t_i = (float)i * spacing < t: it toggles bit
// m = #{i < nx : t_i < t}.  The t_i do not decrease with i, so those voxels are a prefix, and its length is found by bisection with the
// very products the definition compares: 11 steps cover nx <= 1024, a fixed count, so the lanes of a leaf test stay together (the
// estimate t / spacing with two fix-up loops kept 25 more scalar registers alive than the kernel has).  The row belongs to this lane: a
// plain read-modify-write.
RT_DI void row_toggle(const GridView& g, uint32_t* bits, float t) {
  uint32_t m = 0u, hi = g.nx;  // the answer lies in [m, hi]
  for (int step = 0; step < 11; ++step) {
    const uint32_t mid = (m + hi) >> 1;
    const bool below = m < hi && (float)mid * g.spacing < t;
    hi = (m < hi && !below) ? mid : hi;
    m = below ? mid + 1u : m;
  }
  bits[m >> 5] ^= 1u << (m & 31u);
}
// toggles -> suffix parities: bit b becomes the parity of the toggles at b and above, so voxel i is inside iff bit i + 1 is set
RT_DI void row_finish(const GridView& g, uint32_t* bits) {
  uint32_t carry = 0u;
  for (uint32_t w = g.words; w-- > 0u;) {
    uint32_t v = bits[w];
    v ^= v >> 1; v ^= v >> 2; v ^= v >> 4; v ^= v >> 8; v ^= v >> 16;
    v ^= carry;
    carry = (v & 1u) ? ~0u : 0u;
    bits[w] = v;
  }
}
// One node visit of a lane that holds a row; true when the row is finished.  multi_step's visit (trace_multi.hip) with a limit that
// never shrinks: every child the slab test accepts is entered, every triangle of 4.7's hit set S toggles its bit.
template <bool STAGED, bool COUNT>
RT_DI bool row_step(const SceneView& sv, const TraverseLds& lds, uint2* spill, const GridView& g, RowTrav& t, uint32_t& n_nodes, uint32_t& n_tris) {
  LaneStack<STAGED, false> st{lds.stack + threadIdx.x, spill, t.sp};
  const RayPre r = t.r;
  const float limit = __builtin_inff();  // tmax' = +inf - ts
  uint32_t ref[4], key[4];
  test_children<STAGED, false>(sv, lds, r, t.cur, limit, ref, key);
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
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    if ((int32_t)key[c] < 0) break;  // a sorted prefix: leaf keys have the sign bit clear
    const uint32_t first = ref[c] & 0x0fffffffu, count = ((ref[c] >> 28) & 7u) + 1u;
    if (COUNT) n_tris += count;
    if (STAGED) {
      leaf_walk_staged(lds, r, first, count, [&](float tt, float, float, float, uint32_t, uint32_t, uint32_t) -> bool {
        if (tt > r.tmin && tt < limit) row_toggle(g, t.bits, tt + t.ts);
        return false;
      });
    } else {
      const float4* tris = reinterpret_cast<const float4*>(sv.tris);
      for (uint32_t i = 0; i < count; ++i) {
        const float4* p = tris + (size_t)(first + i) * 3;
        const float4 a = p[0], b = p[1], c2 = p[2];
        float tt, tu, tv, det;
        if (tri_test_od(r.o, r.d, a, b, c2, &tt, &tu, &tv, &det) && tt > r.tmin && tt < limit) row_toggle(g, t.bits, tt + t.ts);
      }
    }
  }
  if (next == kAbsent) {
    if (st.sp == 0) return true;
    next = st.pop().y;
  }
  t.cur = next;
  t.sp = st.sp;
  return false;
}
// The persistent loop of k_trace_multi around row_step; queue entry i is row (j, k) = (i % ny, i / ny).  COUNT: counters[2] += node
// visits, [3] += triangle tests.
template <bool STAGED, bool COUNT>
__global__ void __launch_bounds__(kTraverseThreads, kTraverseWavesPerSimdStaged)
k_grid_rows(SceneView sv, GridView g, uint32_t* __restrict__ bits, WorkCounters* __restrict__ work, uint2* __restrict__ spill_base, uint32_t refill,
            unsigned long long* __restrict__ counters) {
  const TraverseLds lds = stage_bvh<STAGED, false>(sv, g_smem);
  uint2* spill = lane_spill(spill_base);
  const uint32_t n = g.ny * g.nz;
  WorkCursor cur = work_begin(n);
  bool more = true;  // wave-uniform
  bool has = false;
  uint32_t n_nodes = 0u, n_tris = 0u;
  RowTrav t;
  for (;;) {
    const unsigned long long idle = __ballot(!has);
    if (more && idle) {
      uint32_t got = 0;
      const uint32_t base = work_take(work, cur, n, (uint32_t)__popcll(idle), &got);
      if (base == kAbsent) more = false;
      else if (!has) {
        const uint32_t rank = (uint32_t)__popcll(idle & ((1ull << lane_id()) - 1ull));
        if (rank < got) {
          const uint32_t row = base + rank;
          f3 o = voxel_point(g, 0u, row % g.ny, row / g.ny);
          const f3 d = mk3(1.0f, 0.0f, 0.0f);
          float tmin = 0.0f, tmax = __builtin_inff();
          t.ts = rebase_ray(sv, o, d, tmin, tmax);  // a mode-0 ray: the far-origin rule of 4.2
          t.r = make_ray(o, d, tmin);
          t.bits = bits + (size_t)row * g.words;
          t.cur = 0u; t.sp = 0;
          has = true;
        }
      }
    }
    if (__ballot(has) == 0ull) { if (!more) break; continue; }
    for (;;) {
      if (has && row_step<STAGED, COUNT>(sv, lds, spill, g, t, n_nodes, n_tris)) { row_finish(g, t.bits); has = false; }
      const uint32_t nidle = (uint32_t)__popcll(__ballot(!has));
      if (nidle == 64u || (more && nidle >= refill)) break;
    }
  }
  if (COUNT) grid_count(counters, 2, n_nodes, n_tris);
}

bool launch_grid_rows(const LaunchCfg& lc, const SceneView& sv, uint32_t cu_count, const GridView& g, uint32_t* bits, WorkCounters* work,
                      unsigned long long* counters, hipStream_t s) {
  const TreeForm tree = tree_form(sv);
  if (tree == TreeForm::TwoLevel) return false;
  const size_t smem = query_lds_bytes(sv, tree, kTraverseThreads);
  const uint32_t per_cu = counted_blocks_per_cu([](auto STAGED, auto COUNT) { return k_grid_rows<STAGED, COUNT>; }, counters != nullptr, tree, kTraverseThreads, smem);
  if (per_cu == 0u) return false;
  with_flags([&](auto STAGED, auto COUNT) {
    hipLaunchKernelGGL((k_grid_rows<STAGED, COUNT>), dim3(query_blocks(lc, cu_count, per_cu)), dim3(kTraverseThreads), smem, s, sv, g, bits, work, lc.spill,
                       lc.refill, counters);
  }, tree == TreeForm::Staged, counters != nullptr);
  return true;
}
bool launch_distance_grid(const LaunchCfg& lc, const SceneView& sv, uint32_t cu_count, const GridView& g, uint32_t method, float* distance, uint32_t* prim,
                          const uint32_t* inside, WorkCounters* work, unsigned long long* counters, hipStream_t s) {
  const TreeForm tree = tree_form(sv);
  if (tree == TreeForm::TwoLevel) return false;
  const size_t smem = query_lds_bytes(sv, tree, kTraverseThreads);
  const uint32_t per_cu =
      method == 2u ? counted_blocks_per_cu([](auto STAGED, auto COUNT) { return k_grid_brick<STAGED, COUNT>; }, counters != nullptr, tree, kTraverseThreads, smem)
                   : counted_blocks_per_cu([](auto STAGED, auto COUNT) { return k_grid_lane<STAGED, COUNT>; }, counters != nullptr, tree, kTraverseThreads, smem);
  if (per_cu == 0u) return false;
  const uint32_t blocks = query_blocks(lc, cu_count, per_cu);
  with_flags([&](auto STAGED, auto COUNT) {
    if (method == 2u)
      hipLaunchKernelGGL((k_grid_brick<STAGED, COUNT>), dim3(blocks), dim3(kTraverseThreads), smem, s, sv, g, distance, prim, inside, work, counters);
    else
      hipLaunchKernelGGL((k_grid_lane<STAGED, COUNT>), dim3(blocks), dim3(kTraverseThreads), smem, s, sv, g, distance, prim, inside, work, lc.spill,
                         lc.refill, counters);
  }, tree == TreeForm::Staged, counters != nullptr);
  return true;
}

}  // namespace rt
