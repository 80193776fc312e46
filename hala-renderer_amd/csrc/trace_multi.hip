// trace_multi.hip — multi-hit ray batches (RENDER_SPEC 4.7): the k nearest hits of every ray of a batch, ordered by (t, triangle id).
// One persistent traversal kernel in the three tree forms of trace_closest.hip (LDS-staged, large one-level, two-level), over the dequeue
// of trace_loop.h (work_begin / work_take) and the building blocks of traverse.h: the LDS layout (stage_bvh), the per-lane stack with its
// spill (LaneStack), the instance transitions (enter_instance / leave_instance), the child test with the key order of 4.4b
// (test_children) and the triangle tests (leaf_walk_staged on staged trees, tri_test_od on the others).  What differs from the
// closest-hit traversal is the limit a ray culls with: the t of its k-th entry once it holds k hits, its tmax until then.
//
// Where the k entries live: in the ray's own slice of the output array, hits[i * k .. i * k + k), kept sorted while the ray is traced;
// the lane holds only the key of the worst entry and the count.  An insertion walks the slice from its end (one 16-B load and store per
// entry that moves; a lane reads back what it wrote itself, in program order).  No LDS beyond what the closest-hit kernels use, so the
// occupancy does not depend on k and a staged tree keeps its place.  The leaf tests are per lane in all three forms.
#include <algorithm>

#include "trace_loop.h"
#include "variants.h"

namespace rt {

struct MultiTrav {
  RayPre r;
  float tmax;
  float limit;               // what the slab test and the pops cull with: tmax until k hits are held, then the k-th entry's t
  unsigned long long worst;  // key (bits(t) << 32 | id) of the k-th entry; all ones until k hits are held
  float4* list;              // hits + i * k: the sorted entries [0, n)
  uint32_t n, idx;
  uint32_t cur;
  int sp;
  uint32_t gid_base;  // two-level trees: inside an instance the triangles' ids are local to the primitive (traverse.h: Trav)
};
RT_DI void multi_begin(MultiTrav& t, const RayPre& r, float tmax, float4* list, uint32_t idx) {
  t.r = r; t.tmax = tmax;
  t.limit = tmax == tmax ? tmax : -1.0f;  // a NaN limit admits no hit (trav_begin)
  t.worst = ~0ull; t.list = list; t.n = 0u; t.idx = idx;
  t.cur = 0u; t.sp = 0; t.gid_base = 0u;
}
// An accepted hit (its key is below the worst key) goes to its place in the sorted slice; with k entries held the worst one drops out.
RT_DI void multi_insert(MultiTrav& t, uint32_t k, unsigned long long key, float tt, float u, float v, uint32_t id) {
  const float4 rec = make_float4(tt, u, v, __uint_as_float(id));
  const uint32_t start = t.n < k ? t.n : k - 1u;  // the slot that opens: behind the list, or the worst entry's
  uint32_t j = start;
  float4 top = rec;  // what stands in slot `start` afterwards
  while (j > 0u) {
    const float4 e = t.list[j - 1u];
    const unsigned long long ek = ((unsigned long long)__float_as_uint(e.x) << 32) | (unsigned long long)__float_as_uint(e.w);
    if (ek < key) break;
    if (j == start) top = e;
    t.list[j] = e;
    --j;
  }
  t.list[j] = rec;
  if (t.n < k) ++t.n;
  if (t.n == k) {  // (then start == k - 1)
    t.worst = ((unsigned long long)__float_as_uint(top.x) << 32) | (unsigned long long)__float_as_uint(top.w);
    t.limit = top.x;
  }
}
// RENDER_SPEC 4.2's range and the order of 4.7: tmin < t < tmax, and below the k-th entry by (t, id) once k are held (t > 0: the bits
// of t order like t)
RT_DI void multi_offer(MultiTrav& t, uint32_t k, float tt, float u, float v, uint32_t id) {
  const unsigned long long key = ((unsigned long long)__float_as_uint(tt) << 32) | (unsigned long long)id;
  if (tt > t.r.tmin && tt < t.tmax && key < t.worst) multi_insert(t, k, key, tt, u, v, id);
}
RT_DI void multi_done(const MultiTrav& t, uint32_t k, uint32_t* counts) {
  for (uint32_t j = t.n; j < k; ++j) t.list[j] = make_float4(-1.0f, 0.0f, 0.0f, __uint_as_float(kAbsent));
  if (counts) counts[t.idx] = t.n;
}

// One node visit of a lane that holds a ray; true when the ray is finished.  The stack, the way into and out of an instance, the child
// test with its keys and order, and the paired leaf walk of staged trees are traverse.h's (LaneStack, enter_instance / leave_instance,
// test_children, leaf_walk_staged), with the list's limit where the closest-hit traversal culls with best.t; every leaf in reach is
// tested by the lane itself, nearest first, while it stays in reach of the limit.
template <bool STAGED, bool INST>
RT_DI bool multi_step(const SceneView& sv, const TraverseLds& lds, uint2* spill, MultiTrav& t, uint32_t k) {
  static_assert(!(INST && STAGED), "LDS-staged trees have no instance levels");
  LaneStack<STAGED, INST> st{lds.stack + threadIdx.x, spill, t.sp};
  uint32_t shade_base;  // (the records of 4.7 carry triangle ids only)
  const RayPre r = t.r;
  uint32_t ref[4], key[4];
  test_children<STAGED, INST>(sv, lds, r, t.cur, t.limit, ref, key);
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
    if (!(key_tn(key[c]) <= t.limit)) break;  // a hit in a nearer leaf may have filled the list: everything behind is out of reach
    const uint32_t first = ref[c] & 0x0fffffffu, count = ((ref[c] >> 28) & 7u) + 1u;
    if (STAGED) {
      leaf_walk_staged(lds, r, first, count, [&](float tt, float uu, float vv, float, uint32_t id, uint32_t, uint32_t) -> bool {
        multi_offer(t, k, tt, uu, vv, id);
        return false;
      });
    } else {
      const float4* tris = reinterpret_cast<const float4*>(sv.tris);
      for (uint32_t i = 0; i < count; ++i) {
        const float4* p = tris + (size_t)(first + i) * 3;
        const float4 a = p[0], b = p[1], c2 = p[2];
        float tt, tu, tv, det;
        if (tri_test_od(r.o, r.d, a, b, c2, &tt, &tu, &tv, &det)) multi_offer(t, k, tt, tu, tv, __float_as_uint(a.w) + t.gid_base);
      }
    }
  }
  // go on with the nearest inner child if it is still in reach, else with the first stack entry that is
  if (next != kAbsent && !(key_tn(next_key) <= t.limit)) next = kAbsent;
  for (;;) {
    if (next == kAbsent) {
      if (st.sp == 0) return true;
      const uint2 e = st.pop();
      if (INST && e.y == kExitRef) { leave_instance(st, t.r, t.gid_base, shade_base); continue; }  // the instance's tree is done
      if (key_tn(e.x) <= t.limit) next = e.y;
      continue;
    }
    if (INST && is_inst_leaf(next)) next = enter_instance(sv, st, t.r, t.gid_base, shade_base, next);
    break;
  }
  t.cur = next;
  t.sp = st.sp;
  return false;
}

// The persistent loop of trace_loop.h (persistent_trace) around multi_step, written out: the same sharded dequeue and ballot-rank refill
// (through persistent_trace's loop made generic, frame kernels came out with other machine code: profiles/traverse_shared.txt).  A
// finished ray pads its slice and writes its count at once: its records are in memory already.
// (The two-level form carries the instance transitions next to the list state: at the 96 registers of 5 waves per SIMD it spilled 8 of
// them to scratch, so it is built for 4 like the staged form.)
template <bool STAGED, bool INST>
__global__ void __launch_bounds__(kTraverseThreads, (STAGED || INST) ? kTraverseWavesPerSimdStaged : kTraverseWavesPerSimd)
k_trace_multi(SceneView sv, const hala_ray* __restrict__ rays, float4* hits, uint32_t* counts, uint32_t n, uint32_t k,
              WorkCounters* __restrict__ work, uint2* __restrict__ spill_base, uint32_t refill) {
  const TraverseLds lds = stage_bvh<STAGED, INST>(sv, g_smem);  // (the large forms' leaf work lists are not used here and not allocated)
  uint2* spill = lane_spill(spill_base);
  WorkCursor cur = work_begin(n);
  bool more = n > 0u;  // wave-uniform
  bool has = false;
  MultiTrav t;
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
          const float4* rp = reinterpret_cast<const float4*>(rays + idx);
          const float4 ro = rp[0], rd = rp[1];
          multi_begin(t, make_ray(mk3(ro.x, ro.y, ro.z), mk3(rd.x, rd.y, rd.z), ro.w), rd.w, hits + (size_t)idx * k, idx);
          has = true;
        }
      }
    }
    if (__ballot(has) == 0ull) { if (!more) break; continue; }
    for (;;) {
      if (has && multi_step<STAGED, INST>(sv, lds, spill, t, k)) { multi_done(t, k, counts); has = false; }
      const uint32_t nidle = (uint32_t)__popcll(__ballot(!has));
      if (nidle == 64u || (more && nidle >= refill)) break;
    }
  }
}

// RENDER_SPEC 4.7, far origins: the distance ray i was moved, back on the t of each of its records (miss records stay)
__global__ void __launch_bounds__(256) k_unbase_multi(float4* __restrict__ hits, const float* __restrict__ moved, uint64_t total, uint32_t k) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  float* t = reinterpret_cast<float*>(hits + i);
  if (reinterpret_cast<const uint32_t*>(t)[3] != kAbsent) *t = *t + moved[i / k];
}

bool launch_trace_multi(const LaunchCfg& lc, const SceneView& sv, uint32_t cu_count, const hala_ray* rays, hala_hit* hits, uint32_t* counts,
                        uint32_t n, uint32_t k, WorkCounters* work, hipStream_t s) {
  const TreeForm tree = tree_form(sv);
  const size_t smem = query_lds_bytes(sv, tree, kTraverseThreads);
  const uint32_t per_cu = tree_blocks_per_cu([](auto STAGED, auto INST) { return k_trace_multi<STAGED, INST>; }, tree, kTraverseThreads, smem);
  if (per_cu == 0u) return false;
  const uint32_t blocks = query_blocks(lc, cu_count, per_cu);
  with_flags([&](auto STAGED, auto INST) {
    if constexpr (!(STAGED && INST))
      hipLaunchKernelGGL((k_trace_multi<STAGED, INST>), dim3(blocks), dim3(kTraverseThreads), smem, s, sv, rays, reinterpret_cast<float4*>(hits), counts, n, k,
                         work, lc.spill, lc.refill);
  }, tree == TreeForm::Staged, tree == TreeForm::TwoLevel);
  return true;
}
void launch_unbase_multi(hala_hit* hits, const float* moved, uint32_t n, uint32_t k, hipStream_t s) {
  const uint64_t total = (uint64_t)n * k;
  hipLaunchKernelGGL(k_unbase_multi, dim3((uint32_t)((total + 255u) / 256u)), dim3(256), 0, s, reinterpret_cast<float4*>(hits), moved, total, k);
}

}  // namespace rt
