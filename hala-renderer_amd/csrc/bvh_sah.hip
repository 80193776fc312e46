// bvh_sah.hip — the full-sweep SAH hierarchy builder (top-down, one tree level per round): the default from 4096 triangles
// (hala_rt_build_options::builder = 1).
// The triangles are sorted ONCE along each axis by the centroid of their box; every open node owns the same range [first, last] of
// positions in all three orders.  A round, for all open nodes at once: per axis a segmented prefix and suffix union of the boxes
// (rocPRIM scan-by-key over the node ids; min / max are exactly associative, so the result does not depend on how the scan is cut up),
// the surface-area cost area(L)*|L| + area(R)*|R| of every split position, the cheapest (cost, axis, position) per node through a
// 64-bit atomic min, then a stable partition of the three orders by the side each triangle went to.  Needs no Morton order.  The
// contract is HierarchyJob's (bvh_build_impl.h).
#include <cstring>

#include <rocprim/rocprim.hpp>

#include <algorithm>

#include "bvh_build_impl.h"

namespace rt {

namespace {

struct BoxUnionOp {
  __host__ __device__ Box6 operator()(const Box6& a, const Box6& b) const { return box_union(a, b); }
};
struct Flag3 { uint32_t v[3]; };
struct Flag3Plus {
  __host__ __device__ Flag3 operator()(const Flag3& a, const Flag3& b) const { return Flag3{{a.v[0] + b.v[0], a.v[1] + b.v[1], a.v[2] + b.v[2]}}; }
};
constexpr unsigned long long kSahNoSplit = ~0ull;
constexpr int kSahQuant = 4;
constexpr uint32_t kSahPosMask = 0x0fffffffu;  // split position relative to the node's first position (n < 2^28); axis in bits 28-29

__global__ void __launch_bounds__(256) k_sah_keys(const Box6* __restrict__ tri_box, uint32_t n, int axis, uint32_t* __restrict__ keys,
                                                   uint32_t* __restrict__ ids) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  keys[i] = f2ord(tri_box[i].mn[axis] + tri_box[i].mx[axis]);  // twice the centroid; ties keep id order (stable sort)
  ids[i] = i;
}
__global__ void __launch_bounds__(256) k_sah_init(uint32_t n, uint32_t* __restrict__ node_of, uint32_t* __restrict__ first, uint32_t* __restrict__ last,
                                                   uint32_t* __restrict__ node_parent, uint32_t* __restrict__ act, unsigned long long* __restrict__ best) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) node_of[i] = 0u;
  if (i == 0u) { first[0] = 0u; last[0] = n - 1u; node_parent[0] = kAbsent; act[0] = 0u; best[0] = kSahNoSplit; }
}
__global__ void __launch_bounds__(256) k_sah_gather(const uint32_t* __restrict__ ord, const Box6* __restrict__ tri_box, uint32_t n, Box6* __restrict__ out) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < n) out[p] = tri_box[ord[p]];
}
// cost of splitting the node of position p between p - 1 and p along `axis`; axis 0 also leaves the node's fitted box
__global__ void __launch_bounds__(256) k_sah_cost(uint32_t n, uint32_t axis, const uint32_t* __restrict__ node_of, const uint32_t* __restrict__ first,
                                                   const uint32_t* __restrict__ last, const Box6* __restrict__ box_l, const Box6* __restrict__ box_r,
                                                   unsigned long long* __restrict__ best, Box6* __restrict__ node_box, float pad, uint32_t quant) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t node = kAbsent;
  unsigned long long key = kSahNoSplit;
  if (p < n) {
    node = node_of[p];
    if (node != kAbsent) {
      const uint32_t lo = first[node], hi = last[node] + 1u;
      if (p > lo) {
        // triangles are tested `quant` at a time (a leaf item of the cooperative pass occupies kLeafSlots lanes however full it is)
        const float cost = half_area(box_l[p - 1u]) * (float)((p - lo + quant - 1u) / quant) + half_area(box_r[p]) * (float)((hi - p + quant - 1u) / quant);
        // areas and counts are >= 0: the bits of the cost order like the cost (a NaN cannot arise from finite boxes; +inf sorts last)
        key = ((unsigned long long)__float_as_uint(cost) << 32) | ((unsigned long long)axis << 28) | (unsigned long long)(p - lo);
      }
      if (axis == 0u && p + 1u == hi) {
        node_box[node] = widen(box_l[p], pad);  // the inclusive scan's last box of the node: the union of its triangle boxes
      }
    }
  }
  // the positions of a node are contiguous: fold the wave's keys per run of equal nodes first, one atomic per run
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (uint32_t off = 1; off < 64u; off <<= 1) {
    const unsigned long long ok = __shfl_down(key, off);
    const uint32_t on = __shfl_down(node, off);
    if (lane + off < 64u && on == node && ok < key) key = ok;
  }
  const uint32_t prev = __shfl_up(node, 1u);
  if (node != kAbsent && (lane == 0u || prev != node) && key != kSahNoSplit) atomicMin(&best[node], key);
}
// per open node: the split it takes, and how many of its two children are inner nodes (>= 2 triangles)
__global__ void __launch_bounds__(256) k_sah_decide(const uint32_t* __restrict__ act, uint32_t count, const unsigned long long* __restrict__ best,
                                                     const uint32_t* __restrict__ first, const uint32_t* __restrict__ last, uint32_t force_median,
                                                     uint2* __restrict__ split, uint32_t* __restrict__ cnt) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count) return;
  const uint32_t node = act[j], lo = first[node], hi = last[node] + 1u;
  const unsigned long long key = best[node];
  uint32_t axis = (uint32_t)(key >> 28) & 3u, k = lo + ((uint32_t)key & kSahPosMask);
  if (force_median || key == kSahNoSplit || axis > 2u || k <= lo || k >= hi) { axis = 0u; k = lo + (hi - lo) / 2u; }  // very deep trees: halve
  split[node] = make_uint2(axis, k);
  cnt[j] = (k - lo >= 2u ? 1u : 0u) + (hi - k >= 2u ? 1u : 0u);
}
__global__ void __launch_bounds__(256) k_sah_children(const uint32_t* __restrict__ act, uint32_t count, const uint32_t* __restrict__ cnt,
                                                       const uint32_t* __restrict__ off, uint32_t next_id, const uint2* __restrict__ split,
                                                       BinaryTree tree, uint32_t* __restrict__ act_next, unsigned long long* __restrict__ best, uint32_t* __restrict__ made) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count) return;
  const BinaryTree& t = tree;
  const uint32_t node = act[j], lo = t.first[node], hi = t.last[node] + 1u, k = split[node].y;
  uint32_t slot = off[j];
  if (k - lo >= 2u) {
    const uint32_t id = next_id + slot;
    t.left[node] = id; t.first[id] = lo; t.last[id] = k - 1u; t.node_parent[id] = node; best[id] = kSahNoSplit; act_next[slot] = id;
    ++slot;
  } else { t.left[node] = kLeafBit | lo; t.leaf_parent[lo] = node; }
  if (hi - k >= 2u) {
    const uint32_t id = next_id + slot;
    t.right[node] = id; t.first[id] = k; t.last[id] = hi - 1u; t.node_parent[id] = node; best[id] = kSahNoSplit; act_next[slot] = id;
  } else { t.right[node] = kLeafBit | k; t.leaf_parent[k] = node; }
  if (j + 1u == count) made[0] = off[j] + cnt[j];
}
// side[triangle] = 1 when it goes to the left child of its node
__global__ void __launch_bounds__(256) k_sah_side(uint32_t n, const uint32_t* __restrict__ node_of, const uint2* __restrict__ split,
                                                   const uint32_t* __restrict__ ord0, const uint32_t* __restrict__ ord1, const uint32_t* __restrict__ ord2,
                                                   uint8_t* __restrict__ side) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const uint32_t node = node_of[p];
  if (node == kAbsent) return;
  const uint2 sp = split[node];
  const uint32_t id = sp.x == 0u ? ord0[p] : (sp.x == 1u ? ord1[p] : ord2[p]);
  side[id] = p < sp.y ? 1u : 0u;
}
__global__ void __launch_bounds__(256) k_sah_flags(uint32_t n, const uint32_t* __restrict__ node_of, const uint32_t* __restrict__ ord0,
                                                    const uint32_t* __restrict__ ord1, const uint32_t* __restrict__ ord2, const uint8_t* __restrict__ side,
                                                    Flag3* __restrict__ flags) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  Flag3 f{{0u, 0u, 0u}};
  if (node_of[p] != kAbsent) { f.v[0] = side[ord0[p]]; f.v[1] = side[ord1[p]]; f.v[2] = side[ord2[p]]; }
  flags[p] = f;
}
// stable partition of every open node's range in the three orders, and the node every position belongs to in the next round
__global__ void __launch_bounds__(256) k_sah_scatter(uint32_t n, uint32_t* __restrict__ node_of, const uint2* __restrict__ split,
                                                      const uint32_t* __restrict__ first, const uint32_t* __restrict__ left, const uint32_t* __restrict__ right,
                                                      const Flag3* __restrict__ flags, const Flag3* __restrict__ scan, const uint32_t* __restrict__ in0,
                                                      const uint32_t* __restrict__ in1, const uint32_t* __restrict__ in2, uint32_t* __restrict__ out0,
                                                      uint32_t* __restrict__ out1, uint32_t* __restrict__ out2) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const uint32_t node = node_of[p];
  const uint32_t id[3] = {in0[p], in1[p], in2[p]};
  uint32_t* const out[3] = {out0, out1, out2};
  if (node == kAbsent) {
#pragma unroll
    for (int b = 0; b < 3; ++b) out[b][p] = id[b];
    return;
  }
  const uint32_t lo = first[node], k = split[node].y;
  const Flag3 f = flags[p], sp = scan[p], s0 = scan[lo];
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    const uint32_t lefts = sp.v[b] - s0.v[b];  // left-going triangles before p in this node's range of order b
    out[b][f.v[b] ? lo + lefts : k + ((p - lo) - lefts)] = id[b];
  }
  const uint32_t child = p < k ? left[node] : right[node];
  node_of[p] = (child & kLeafBit) ? kAbsent : child;
}

constexpr uint32_t kSweepRounds = 64;  // below that depth every node is halved instead: at most 28 more rounds

struct SahScratch {
  Dev<uint32_t> keys_in, keys_out, ids_in, ord[3][2], node_of, act[2], cnt, off, made;
  Dev<Box6> box_in, box_l, box_r;
  Dev<unsigned long long> best;
  Dev<uint2> split;
  Dev<uint8_t> side;
  Dev<Flag3> flags, scan;
  Dev<char> tmp;  // rocPRIM's: the largest of its five uses
  DevList plan(uint32_t n) {
    const uint32_t* u = nullptr;
    uint32_t* uo = nullptr;
    Box6* bx = nullptr;
    Flag3* f3 = nullptr;
    size_t need[5] = {0, 0, 0, 0, 0};
    (void)rocprim::radix_sort_pairs(nullptr, need[0], uo, uo, uo, uo, n, 0, 32, 0);
    (void)rocprim::inclusive_scan_by_key(nullptr, need[1], u, bx, bx, n, BoxUnionOp(), rocprim::equal_to<uint32_t>(), 0);
    (void)rocprim::inclusive_scan_by_key(nullptr, need[2], rocprim::make_reverse_iterator(u), rocprim::make_reverse_iterator(bx),
                                         rocprim::make_reverse_iterator(bx), n, BoxUnionOp(), rocprim::equal_to<uint32_t>(), 0);
    (void)exclusive_sum(nullptr, need[3], uo, uo, n, 0);
    (void)rocprim::exclusive_scan(nullptr, need[4], f3, f3, Flag3{{0u, 0u, 0u}}, n, Flag3Plus(), 0);
    size_t tmp_bytes = 0;
    for (size_t v : need) tmp_bytes = std::max(tmp_bytes, v);
    return {keys_in.of(n), keys_out.of(n), ids_in.of(n), ord[0][0].of(n), ord[0][1].of(n), ord[1][0].of(n), ord[1][1].of(n), ord[2][0].of(n), ord[2][1].of(n),
            node_of.of(n), act[0].of(n), act[1].of(n), cnt.of(n), off.of(n), box_in.of(n), box_l.of(n), box_r.of(n), best.of(n - 1), split.of(n - 1),
            side.of(n), flags.of(n), scan.of(n), made.of(4), tmp.of(tmp_bytes)};
  }
};

}  // namespace

size_t sah_scratch_bytes(uint32_t n) { return arena_bytes(SahScratch().plan(n)); }

std::string sah_hierarchy(const HierarchyJob& job, hipStream_t s) {
  const uint32_t n = job.n, ni = n - 1;
  const BinaryTree& t = job.tree;
  SahScratch sc;
  std::string e = alloc_all(sc.plan(n));
  if (!e.empty()) return e;
  const uint32_t* nk = sc.node_of;
  auto rk = rocprim::make_reverse_iterator(nk + n);
  auto rin = rocprim::make_reverse_iterator(sc.box_in.get() + n);
  auto rout = rocprim::make_reverse_iterator(sc.box_r.get() + n);
  const size_t tmp_bytes = sc.tmp.bytes;
  size_t tb;
  for (int a = 0; a < 3; ++a) {
    hipLaunchKernelGGL(k_sah_keys, dim3(nblk(n)), dim3(256), 0, s, job.tri_box, n, a, sc.keys_in, sc.ids_in);
    HIP_TRY(rocprim::radix_sort_pairs(sc.tmp.raw, tb = tmp_bytes, sc.keys_in.get(), sc.keys_out.get(), sc.ids_in.get(), sc.ord[a][0].get(), n, 0, 32, s));
  }
  hipLaunchKernelGGL(k_sah_init, dim3(nblk(n)), dim3(256), 0, s, n, sc.node_of, t.first, t.last, t.node_parent, sc.act[0], sc.best);
  const uint32_t quant = (uint32_t)kSahQuant;  // = the leaf slots of the cooperative pass (traverse.h: RT_LEAF_SLOTS)
  uint32_t open = 1, next_id = 1, round = 0;
  int cur = 0, ac = 0;
  while (open > 0) {
    if (round > kSweepRounds + 32u) return "bvh_build: the SAH rounds do not terminate";
    const uint32_t* o[3] = {sc.ord[0][cur], sc.ord[1][cur], sc.ord[2][cur]};
    const uint32_t axes = round < kSweepRounds ? 3u : 1u;  // past the sweep rounds only the boxes are still needed: axis 0 leaves them
    for (uint32_t a = 0; a < axes; ++a) {
      hipLaunchKernelGGL(k_sah_gather, dim3(nblk(n)), dim3(256), 0, s, o[a], job.tri_box, n, sc.box_in);
      HIP_TRY(rocprim::inclusive_scan_by_key(sc.tmp.raw, tb = tmp_bytes, nk, sc.box_in.get(), sc.box_l.get(), n, BoxUnionOp(), rocprim::equal_to<uint32_t>(), s));
      HIP_TRY(rocprim::inclusive_scan_by_key(sc.tmp.raw, tb = tmp_bytes, rk, rin, rout, n, BoxUnionOp(), rocprim::equal_to<uint32_t>(), s));
      hipLaunchKernelGGL(k_sah_cost, dim3(nblk(n)), dim3(256), 0, s, n, a, nk, t.first, t.last, sc.box_l, sc.box_r, sc.best, t.node_box, job.pad, quant);
    }
    hipLaunchKernelGGL(k_sah_decide, dim3(nblk(open)), dim3(256), 0, s, sc.act[ac], open, sc.best, t.first, t.last, round >= kSweepRounds ? 1u : 0u, sc.split,
                       sc.cnt);
    HIP_TRY(exclusive_sum(sc.tmp.raw, tb = tmp_bytes, sc.cnt.get(), sc.off.get(), open, s));
    hipLaunchKernelGGL(k_sah_children, dim3(nblk(open)), dim3(256), 0, s, sc.act[ac], open, sc.cnt, sc.off, next_id, sc.split, t, sc.act[ac ^ 1], sc.best,
                       sc.made);
    hipLaunchKernelGGL(k_sah_side, dim3(nblk(n)), dim3(256), 0, s, n, nk, sc.split, o[0], o[1], o[2], sc.side);
    hipLaunchKernelGGL(k_sah_flags, dim3(nblk(n)), dim3(256), 0, s, n, nk, o[0], o[1], o[2], sc.side, sc.flags);
    HIP_TRY(rocprim::exclusive_scan(sc.tmp.raw, tb = tmp_bytes, sc.flags.get(), sc.scan.get(), Flag3{{0u, 0u, 0u}}, n, Flag3Plus(), s));
    hipLaunchKernelGGL(k_sah_scatter, dim3(nblk(n)), dim3(256), 0, s, n, sc.node_of, sc.split, t.first, t.left, t.right, sc.flags, sc.scan, o[0], o[1], o[2],
                       sc.ord[0][cur ^ 1], sc.ord[1][cur ^ 1], sc.ord[2][cur ^ 1]);
    uint32_t now = 0;
    HIP_TRY(hipMemcpyAsync(&now, sc.made, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    next_id += now;
    if (next_id > ni) return "bvh_build: the SAH rounds made more nodes than a binary tree has";
    open = now;
    cur ^= 1; ac ^= 1; ++round;
  }
  if (next_id != ni) return "bvh_build: the SAH rounds made " + std::to_string(next_id) + " of " + std::to_string(ni) + " nodes";
  HIP_TRY(hipMemcpyAsync(job.sorted_ids, sc.ord[0][cur], (size_t)n * 4, hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipGetLastError());
  return "";
}

}  // namespace rt
