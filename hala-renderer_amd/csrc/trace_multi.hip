// trace_multi.hip — multi-hit ray batches (RENDER_SPEC 4.7): the k nearest hits of every ray of a batch, ordered by (t, triangle id).
// One persistent traversal kernel in the three tree forms of trace_closest.hip (LDS-staged, large one-level, two-level), over the same
// dequeue (trace_loop.h: work_begin / work_take), the same LDS layout and stack with its spill (stage_bvh, lane_spill), the same slab test
// and key order (4.4b) and the same triangle tests (tri_test2 on staged trees, tri_test_od on the others).  What differs from the
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

// One node visit of a lane that holds a ray (traverse.h: trav_step without the any-hit, counting and wave-cooperative parts); true when
// the ray is finished.  The children are tested, keyed and sorted exactly as there; every leaf in reach is tested by the lane itself,
// nearest first, while it stays in reach of the limit.
template <bool STAGED, bool INST>
RT_DI bool multi_step(const SceneView& sv, const TraverseLds& lds, uint2* spill, MultiTrav& t, uint32_t k) {
  static_assert(!(INST && STAGED), "LDS-staged trees have no instance levels");
  constexpr int kS = stack_lds<STAGED, INST>();
  RT_LDS u32x2* stack = lds.stack + threadIdx.x;
  int sp = t.sp;
  auto pop = [&]() -> uint2 {
    --sp;
    if (sp < kS) { const u32x2 v = stack[sp * kTraverseThreads]; return make_uint2(v.x, v.y); }
    return spill[sp - kS];
  };
  auto push = [&](uint32_t a, uint32_t b) {
    if (sp < kS) stack[sp * kTraverseThreads] = u32x2{a, b}; else spill[sp - kS] = make_uint2(a, b);
    ++sp;
  };
  // RENDER_SPEC 4.5, as in trav_step: the world-space ray is parked under an exit mark while the lane is inside an instance
  auto enter_instance = [&](uint32_t leaf) -> uint32_t {
    const float4* ip = reinterpret_cast<const float4*>(sv.inst_refs + (leaf & 0x0fffffffu));
    const float4 i0 = ip[0], i1 = ip[1], i2 = ip[2], i3 = ip[3];
    push(__float_as_uint(t.r.o.x), __float_as_uint(t.r.o.y));
    push(__float_as_uint(t.r.o.z), __float_as_uint(t.r.d.x));
    push(__float_as_uint(t.r.d.y), __float_as_uint(t.r.d.z));
    push(0u, kExitRef);
    const f3 r0 = mk3(i0.x, i0.y, i0.z), r1 = mk3(i0.w, i1.x, i1.y), r2 = mk3(i1.z, i1.w, i2.x), tr = mk3(i2.y, i2.z, i2.w);
    const f3 tv = t.r.o - tr, d = t.r.d;
    t.r = make_ray(mk3(dot3(r0, tv), dot3(r1, tv), dot3(r2, tv)), mk3(dot3(r0, d), dot3(r1, d), dot3(r2, d)), t.r.tmin);
    t.gid_base = __float_as_uint(i3.y);
    return __float_as_uint(i3.x);
  };
  auto leave_instance = [&]() {
    const uint2 c2 = pop(), c1 = pop(), c0 = pop();
    t.r = make_ray(mk3(__uint_as_float(c0.x), __uint_as_float(c0.y), __uint_as_float(c1.x)),
                   mk3(__uint_as_float(c1.y), __uint_as_float(c2.x), __uint_as_float(c2.y)), t.r.tmin);
    t.gid_base = 0u;
  };
  const RayPre r = t.r;
  uint32_t ref[4], key[4];
  {
    float4 q0, q1, q2, q3;
    if (STAGED) { const RT_LDS f32x4* p = lds.nodes + (size_t)t.cur * 4; q0 = ld4(p); q1 = ld4(p + 1); q2 = ld4(p + 2); q3 = ld4(p + 3); }
    else { const float4* p = reinterpret_cast<const float4*>(sv.nodes) + (size_t)t.cur * 4; q0 = p[0]; q1 = p[1]; q2 = p[2]; q3 = p[3]; }
    const uint32_t ex = __float_as_uint(q0.w);
    const float kx = __uint_as_float((ex & 0xffu) << 23) * r.idir.x, ky = __uint_as_float(((ex >> 8) & 0xffu) << 23) * r.idir.y,
                kz = __uint_as_float(((ex >> 16) & 0xffu) << 23) * r.idir.z;
    const float ax = __fmaf_rn(q0.x, r.idir.x, -r.ood.x), ay = __fmaf_rn(q0.y, r.idir.y, -r.ood.y), az = __fmaf_rn(q0.z, r.idir.z, -r.ood.z);
    const uint32_t lox = __float_as_uint(q1.x), loy = __float_as_uint(q1.y), loz = __float_as_uint(q1.z);
    const uint32_t hix = __float_as_uint(q1.w), hiy = __float_as_uint(q2.x), hiz = __float_as_uint(q2.y);
    ref[0] = __float_as_uint(q3.x); ref[1] = __float_as_uint(q3.y); ref[2] = __float_as_uint(q3.z); ref[3] = __float_as_uint(q3.w);
    const bool px = r.idir.x >= 0.0f, py = r.idir.y >= 0.0f, pz = r.idir.z >= 0.0f;
    const uint32_t nx = px ? lox : hix, fx = px ? hix : lox, ny = py ? loy : hiy, fy = py ? hiy : loy, nz = pz ? loz : hiz, fz = pz ? hiz : loz;
    const v2f kx2 = {kx, kx}, ky2 = {ky, ky}, kz2 = {kz, kz}, ax2 = {ax, ax}, ay2 = {ay, ay}, az2 = {az, az};
#pragma unroll
    for (int c = 0; c < 4; ++c) {  // the slab test of 4.3b with the list's limit where the closest-hit traversal has best.t
      const v2f tx = __builtin_elementwise_fma(v2f{ubyte_f32(nx, c), ubyte_f32(fx, c)}, kx2, ax2);
      const v2f ty = __builtin_elementwise_fma(v2f{ubyte_f32(ny, c), ubyte_f32(fy, c)}, ky2, ay2);
      const v2f tz = __builtin_elementwise_fma(v2f{ubyte_f32(nz, c), ubyte_f32(fz, c)}, kz2, az2);
      const float tn = hw_maxf(hw_maxf(tx.x, ty.x), hw_maxf(tz.x, r.tmin));
      const float tf = hw_minf(hw_minf(tx.y, ty.y), hw_minf(tz.y, t.limit));
      const bool hit = ref[c] != kAbsent && tn <= tf * 1.0000004f;
      const uint32_t inner_bit = INST ? ((!(ref[c] >> 31) || (ref[c] >> 28) == 0xFu) ? kInnerKey : 0u) : (~ref[c] & kInnerKey);
      const uint32_t kc = (__float_as_uint(tn) & 0xfffffffcu) | ((uint32_t)c | inner_bit);
      key[c] = hit ? kc : kMissKey;
    }
  }
  sort2kv(key[0], key[1], ref[0], ref[1]); sort2kv(key[2], key[3], ref[2], ref[3]); sort2kv(key[0], key[2], ref[0], ref[2]);
  sort2kv(key[1], key[3], ref[1], ref[3]); sort2kv(key[1], key[2], ref[1], ref[2]);
  // the inner children that were hit: the nearest is visited next, the others wait on the stack with their keys
  bool in[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) in[c] = (int32_t)key[c] < -1;
#pragma unroll
  for (int c = 3; c >= 1; --c) {
    const bool left = c == 3 ? (in[0] | in[1] | in[2]) : (c == 2 ? (in[0] | in[1]) : in[0]);
    if (in[c] & left) push(key[c], ref[c]);
  }
  uint32_t next = in[0] ? ref[0] : (in[1] ? ref[1] : (in[2] ? ref[2] : (in[3] ? ref[3] : kAbsent)));
  const uint32_t next_key = in[0] ? key[0] : (in[1] ? key[1] : (in[2] ? key[2] : key[3]));
  // the leaves in reach, nearest first (a sorted prefix: leaf keys have the sign bit clear, inner children and misses have it set)
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    if ((int32_t)key[c] < 0) break;
    if (!(key_tn(key[c]) <= t.limit)) break;  // a hit in a nearer leaf may have filled the list: everything behind is out of reach
    const uint32_t first = ref[c] & 0x0fffffffu, count = ((ref[c] >> 28) & 7u) + 1u;
    if (STAGED) {  // two triangles per packed test (leaf_test_staged)
      for (uint32_t i = 0; i < count; i += 2u) {
        const bool two = i + 1u < count;
        const RT_LDS f32x4* p = lds.tris + (size_t)(first + i) * 3;
        const float4 a0 = ld4(p), b0 = ld4(p + 1), c0 = ld4(p + 2);
        float4 a1 = a0, b1 = b0, c1 = c0;
        if (two) { a1 = ld4(p + 3); b1 = ld4(p + 4); c1 = ld4(p + 5); }
        bool ok[2]; float tt[2], uu[2], vv[2], dd[2];
        tri_test2(r, a0, b0, c0, a1, b1, c1, ok, tt, uu, vv, dd);
        if (ok[0]) multi_offer(t, k, tt[0], uu[0], vv[0], __float_as_uint(a0.w));
        if (two && ok[1]) multi_offer(t, k, tt[1], uu[1], vv[1], __float_as_uint(a1.w));
      }
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
      if (sp == 0) { t.sp = 0; return true; }
      const uint2 e = pop();
      if (INST && e.y == kExitRef) { leave_instance(); continue; }  // the instance's tree is done: back to the world-space ray
      if (key_tn(e.x) <= t.limit) next = e.y;
      continue;
    }
    if (INST && is_inst_leaf(next)) next = enter_instance(next);
    break;
  }
  t.cur = next;
  t.sp = sp;
  return false;
}

// The persistent loop of trace_loop.h (persistent_trace) around multi_step: the same sharded dequeue and ballot-rank refill.  A finished
// ray pads its slice and writes its count at once: its records are in memory already.
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

// The kernel's own LDS: the per-lane stacks, and a staged tree behind them
static size_t multi_lds_bytes(const SceneView& sv, TreeForm tree) {
  const size_t stacks = (size_t)traverse_stack_lds_levels(tree) * kTraverseThreads * 8;
  return tree == TreeForm::Staged ? stacks + (size_t)sv.lds_nodes * 64 + (size_t)sv.lds_tris * 48 : stacks;
}
bool launch_trace_multi(const LaunchCfg& lc, const SceneView& sv, uint32_t cu_count, const hala_ray* rays, hala_hit* hits, uint32_t* counts,
                        uint32_t n, uint32_t k, WorkCounters* work, hipStream_t s) {
  const TreeForm tree = tree_form(sv);
  const size_t smem = multi_lds_bytes(sv, tree);
  const uint32_t per_cu = tree_blocks_per_cu([](auto STAGED, auto INST) { return k_trace_multi<STAGED, INST>; }, tree, kTraverseThreads, smem);
  if (per_cu == 0u) return false;
  // the spill area holds one slice per lane of lc.persistent_blocks workgroups: never a larger grid than that
  const uint32_t blocks = std::min(lc.persistent_blocks, cu_count * std::min(per_cu, 8u));
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
