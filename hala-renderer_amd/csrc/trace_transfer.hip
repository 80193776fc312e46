// trace_transfer.hip — transfer bakes (RENDER_SPEC 4.13): every owned texel of a receiver's bake map is projected along its normal, from
// `front` ahead of the surface to `back` behind it, onto the triangles of a chosen set of instances (the targets); the nearest target hit
// by (t, triangle id) is the texel's record.  Two kernels.
// k_trace_transfer is a persistent closest-hit traversal of its own, written like the multi-hit kernel (trace_multi.hip) over the dequeue
// of trace_loop.h (work_begin / work_take) and the building blocks of traverse.h (stage_bvh, LaneStack, test_children, leaf_walk_staged,
// tri_test_od), in the two one-level tree forms (bakes are refused on two-level trees: no INST form).  What differs from the closest-hit
// traversal of the frame:
//   the ray comes from the receiver's sample buffer (bake.hip), generated in the lane that traces it, as the occlusion rays are
//   (occlusion.hip: OcclusionSourceT::load) — no ray queue in memory; a texel without a valid sample takes no ray and gets the miss record;
//   a triangle is admitted only if its global id lies in one of the target ranges (instances own contiguous id ranges: the host merges
//   the target set into sorted [lo, hi) ranges).  The filter sits behind the accepted triangle test and the range compare: it is asked
//   for the few triangles a ray really crosses nearer than its limit, not for every candidate of a leaf.  One or two ranges — one
//   target, or every instance but the receiver — are kernel arguments (scalar registers, two unsigned compares each); more are bisected
//   in a table in memory.  The 128-B shading record is never read to learn an instance;
//   the limit a ray culls with is its tmax until a TARGET hit is held: a triangle of another instance never shrinks it.  Box tests and
//   pops compare with <=, so a lower id at exactly the limit is still reached (RENDER_SPEC 4.7 at k = 1).
// The finishing lane writes (t, u, v, id) into the first half of the texel's 32-B record; k_transfer_resolve, one lane per texel, then
// reads that half back, fetches the hit triangle's vertex normals (64 B of its shading record, once per HIT), and writes whole records:
// the wave exchanges the halves so that each of its two store instructions writes 1 KiB without a gap (as k_bake_sample does).
#include <algorithm>

#include "trace_loop.h"
#include "variants.h"

namespace rt {

RT_DI bool is_target(const TransferTargets& tg, uint32_t id) {
  if (tg.count <= 2u) return (id - tg.lo0 < tg.hi0 - tg.lo0) | (id - tg.lo1 < tg.hi1 - tg.lo1);  // (an unused range is [0, 0): never)
  uint32_t a = 0u, b = tg.count;  // table[a].x <= id < table[b].x, or id below every range
  while (b - a > 1u) {
    const uint32_t mid = (a + b) >> 1;
    if (tg.table[mid].x <= id) a = mid; else b = mid;
  }
  const uint2 r = tg.table[a];
  return id - r.x < r.y - r.x;  // (id < r.x wraps: never)
}

struct TransferTrav {
  RayPre r;
  float limit;   // what the slab test and the pops cull with: tmax until a target hit is held, then its t
  float u, v, ts;
  uint32_t id;   // the held hit's triangle, kAbsent: none yet
  uint32_t idx, cur;
  int sp;
};
RT_DI void transfer_begin(TransferTrav& t, const RayPre& r, float tmax, float ts, uint32_t idx) {
  t.r = r;
  t.limit = tmax == tmax ? tmax : -1.0f;  // a NaN limit admits no hit (trav_begin)
  t.u = 0.0f; t.v = 0.0f; t.ts = ts; t.id = kAbsent; t.idx = idx;
  t.cur = 0u; t.sp = 0;
}
// RENDER_SPEC 4.2's range and the order of 4.7 at k = 1: tmin < t < tmax, below the held hit by (t, id); then the target filter
RT_DI void transfer_offer(TransferTrav& t, const TransferTargets& tg, float tt, float u, float v, uint32_t id) {
  const bool nearer = tt < t.limit || (tt == t.limit && t.id != kAbsent && id < t.id);  // (no hit held: limit is tmax, which t must stay below)
  if (tt > t.r.tmin && nearer && is_target(tg, id)) { t.limit = tt; t.u = u; t.v = v; t.id = id; }
}
RT_DI void transfer_done(const TransferTrav& t, float4* out) {
  out[(size_t)t.idx * 2u] = t.id != kAbsent ? make_float4(t.limit + t.ts, t.u, t.v, __uint_as_float(t.id)) : make_float4(-1.0f, 0.0f, 0.0f, __uint_as_float(kAbsent));
}

// One node visit of a lane that holds a ray; true when the ray is finished: multi_step (trace_multi.hip) with the one held hit in registers
template <bool STAGED>
RT_DI bool transfer_step(const SceneView& sv, const TraverseLds& lds, uint2* spill, const TransferTargets& tg, TransferTrav& t) {
  LaneStack<STAGED, false> st{lds.stack + threadIdx.x, spill, t.sp};
  const RayPre r = t.r;
  uint32_t ref[4], key[4];
  test_children<STAGED, false>(sv, lds, r, t.cur, t.limit, ref, key);
  // the inner children that were hit: the nearest is visited next, the others wait on the stack with their keys
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
  // the leaves in reach, nearest first (a sorted prefix: leaf keys have the sign bit clear, inner children and misses have it set)
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    if ((int32_t)key[c] < 0) break;
    if (!(key_tn(key[c]) <= t.limit)) break;  // a target hit in a nearer leaf may have drawn the limit in: everything behind is out of reach
    const uint32_t first = ref[c] & 0x0fffffffu, count = ((ref[c] >> 28) & 7u) + 1u;
    if (STAGED) {
      leaf_walk_staged(lds, r, first, count, [&](float tt, float uu, float vv, float, uint32_t id, uint32_t, uint32_t) -> bool {
        transfer_offer(t, tg, tt, uu, vv, id);
        return false;
      });
    } else {
      const float4* tris = reinterpret_cast<const float4*>(sv.tris);
      for (uint32_t i = 0; i < count; ++i) {
        const float4* p = tris + (size_t)(first + i) * 3;
        const float4 a = p[0], b = p[1], c2 = p[2];
        float tt, tu, tv, det;
        if (tri_test_od(r.o, r.d, a, b, c2, &tt, &tu, &tv, &det)) transfer_offer(t, tg, tt, tu, tv, __float_as_uint(a.w));
      }
    }
  }
  // go on with the nearest inner child if it is still in reach, else with the first stack entry that is
  if (next != kAbsent && !(key_tn(next_key) <= t.limit)) next = kAbsent;
  while (next == kAbsent) {
    if (st.sp == 0) return true;
    const uint2 e = st.pop();
    if (key_tn(e.x) <= t.limit) next = e.y;
  }
  t.cur = next;
  t.sp = st.sp;
  return false;
}

// RENDER_SPEC 4.13, the ray of texel idx: validity is 4.10's rule on (point, 0, normal); n = normal * (1 / sqrt(nn)), o = madd(n, front,
// point), d = -n, [0, tmax); set up as a mode-0 ray (the far-origin rule of 4.2: ts comes back on the hit's t).  false: no ray — an
// ownerless texel (the all-zero sample) or an invalid sample.
RT_DI bool transfer_load(const SceneView& sv, const float4* __restrict__ samples, uint32_t idx, float front, float tmax, TransferTrav& t) {
  constexpr float kInf = __builtin_huge_valf();
  const float4 pb = samples[(size_t)idx * 2u], nr = samples[(size_t)idx * 2u + 1u];
  const f3 nrm = mk3(nr.x, nr.y, nr.z);
  const float nn = dot3(nrm, nrm);
  if (!(nn > 0.0f && nn < kInf && fabsf(pb.x) < kInf && fabsf(pb.y) < kInf && fabsf(pb.z) < kInf)) return false;
  const f3 n = nrm * rcp_rn(sqrt_rn(nn));
  f3 o = madd3(n, front, mk3(pb.x, pb.y, pb.z));
  const f3 d = -n;
  float tmin = 0.0f;
  const float ts = rebase_ray(sv, o, d, tmin, tmax);
  transfer_begin(t, make_ray(o, d, tmin), tmax, ts, idx);
  return true;
}

// The persistent loop of trace_multi.hip (k_trace_multi) around transfer_step.  A finished ray writes its 16 B at once.
// (Both forms compile without scratch at their launch bounds; the staged form is built for kTraverseWavesPerSimdStaged like every
// staged traversal kernel: the packed leaf walk wants its 128 registers.)
template <bool STAGED>
__global__ void __launch_bounds__(kTraverseThreads, STAGED ? kTraverseWavesPerSimdStaged : kTraverseWavesPerSimd)
k_trace_transfer(SceneView sv, const float4* __restrict__ samples, float4* out, uint32_t n, float front, float tmax, TransferTargets tg,
                 WorkCounters* __restrict__ work, uint2* __restrict__ spill_base, uint32_t refill) {
  const TraverseLds lds = stage_bvh<STAGED, false>(sv, g_smem);  // (the large form's leaf work lists are not used here and not allocated)
  uint2* spill = lane_spill(spill_base);
  WorkCursor cur = work_begin(n);
  bool more = n > 0u;  // wave-uniform
  bool has = false;
  TransferTrav t;
  for (;;) {
    const unsigned long long idle = __ballot(!has);
    if (more && idle) {
      uint32_t got = 0;
      const uint32_t base = work_take(work, cur, n, (uint32_t)__popcll(idle), &got);
      if (base == kAbsent) more = false;
      else if (!has) {
        const uint32_t rank = (uint32_t)__popcll(idle & ((1ull << lane_id()) - 1ull));
        if (rank < got) {
          const uint32_t idx = base + rank;  // (< n: work_take grants entries of the queue only)
          if (transfer_load(sv, samples, idx, front, tmax, t)) has = true;
          else out[(size_t)idx * 2u] = make_float4(-1.0f, 0.0f, 0.0f, __uint_as_float(kAbsent));
        }
      }
    }
    if (__ballot(has) == 0ull) { if (!more) break; continue; }
    for (;;) {
      if (has && transfer_step<STAGED>(sv, lds, spill, tg, t)) { transfer_done(t, out); has = false; }
      const uint32_t nidle = (uint32_t)__popcll(__ballot(!has));
      if (nidle == 64u || (more && nidle >= refill)) break;
    }
  }
}

// One lane per texel, a wave per 64 consecutive texels: the first half of the record as the trace left it -> the whole record.
// normal: RENDER_SPEC 4.11's shading normal (make_surface's form, shading.h) of the HIT triangle at the hit's (u, v), through the hit
// instance's transform; not turned to the ray.  height = front - t.  A miss: (-1, 0, 0, ~0, 0, 0, 0, 0).
__global__ void __launch_bounds__(256) k_transfer_resolve(SceneView sv, float4* __restrict__ out, uint32_t count, float front) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, lane = lane_id();
  float4 h = make_float4(-1.0f, 0.0f, 0.0f, __uint_as_float(kAbsent)), nh = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (i < count) {
    const float4 got = out[(size_t)i * 2u];
    const uint32_t gid = __float_as_uint(got.w);
    if (gid != kAbsent) {
      h = got;
      const float4* sp = reinterpret_cast<const float4*>(sv.shade_tris + gid);
      const float4 s0 = sp[0], s1 = sp[1], s2 = sp[2], s3 = sp[3];
      const float u = got.y, v = got.z, w0 = 1.0f - u - v;
      const f3 nl = madd3(mk3(s3.x, s3.y, s3.z), v, madd3(mk3(s2.x, s2.y, s2.z), u, mk3(s1.x, s1.y, s1.z) * w0));
      const f3 nw = normalize3(transform_normal(sv.primitives[__float_as_uint(s0.w)].transform, nl));
      nh = make_float4(nw.x, nw.y, nw.z, front - got.x);
    }
  }
  // word j of the wave's 128 goes to lane j & 63 of store j >> 6: it is word j & 1 of the record of lane j >> 1.  (Every record of the
  // wave is read above before any is written below: the loads' values are needed for the exchange.)
  const size_t base = (size_t)(i - lane) * 2u;
#pragma unroll
  for (uint32_t k = 0; k < 2u; ++k) {
    const int src = (int)((lane >> 1) + 32u * k);
    const float4 a = make_float4(__shfl(h.x, src), __shfl(h.y, src), __shfl(h.z, src), __shfl(h.w, src));
    const float4 b = make_float4(__shfl(nh.x, src), __shfl(nh.y, src), __shfl(nh.z, src), __shfl(nh.w, src));
    const size_t j = base + 64u * k + lane;
    const bool odd = (lane & 1u) != 0u;  // (per component: a select between two float4 went through scratch, bake.hip)
    if (j < (size_t)count * 2u) out[j] = make_float4(odd ? b.x : a.x, odd ? b.y : a.y, odd ? b.z : a.z, odd ? b.w : a.w);
  }
}

bool launch_trace_transfer(const LaunchCfg& lc, const SceneView& sv, uint32_t cu_count, const hala_occlusion_sample* samples, const TransferTargets& targets,
                           float front, float tmax, hala_bake_transfer_hit* out, uint32_t count, WorkCounters* work, hipStream_t s) {
  const TreeForm tree = tree_form(sv);
  if (tree == TreeForm::TwoLevel) return false;
  const size_t smem = query_lds_bytes(sv, tree, kTraverseThreads);
  int n = 0;
  const hipError_t e = tree == TreeForm::Staged ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_trace_transfer<true>, kTraverseThreads, smem)
                                                : hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_trace_transfer<false>, kTraverseThreads, smem);
  if (e != hipSuccess || n <= 0) return false;
  const uint32_t blocks = query_blocks(lc, cu_count, (uint32_t)n);
  const float4* sp = reinterpret_cast<const float4*>(samples);
  float4* op = reinterpret_cast<float4*>(out);
  with_flags([&](auto STAGED) {
    hipLaunchKernelGGL((k_trace_transfer<STAGED>), dim3(blocks), dim3(kTraverseThreads), smem, s, sv, sp, op, count, front, tmax, targets, work, lc.spill, lc.refill);
  }, tree == TreeForm::Staged);
  hipLaunchKernelGGL(k_transfer_resolve, dim3(blocks_for(count, 256)), dim3(256), 0, s, sv, op, count, front);
  return true;
}

}  // namespace rt
