// bvh_ploc.hip — PLOC (parallel locally-ordered clustering, Meister & Bittner 2018): the fast large-scene hierarchy builder
// (hala_rt_build_options::builder = 2).  Clusters (initially the triangles, in Morton order) repeatedly merge with their nearest
// neighbour — nearest = smallest surface area of the union, searched kPlocRadius positions to either side — whenever the choice is
// mutual.  Because merged clusters need not be adjacent, the triangles are re-ordered once at the end so that every subtree is a
// contiguous range again.  The contract is HierarchyJob's (bvh_build_impl.h).
#include "bvh_build_impl.h"

namespace rt {

namespace {

constexpr int kPlocRadius = 16;
constexpr uint32_t kPlocTail = 512;  // clusters the one-workgroup tail takes over at
RT_DI uint32_t ploc_size(uint32_t ref, const uint32_t* __restrict__ subtree) { return (ref & kLeafBit) ? 1u : subtree[ref]; }

// ---- one round, as three steps over accessors: the global kernels read device memory, the tail kernel LDS --------------------------
// the nearest of the m live clusters to cluster i, at most `radius` positions away
template <class BoxAt> RT_DI uint32_t ploc_nearest(uint32_t i, uint32_t m, uint32_t radius, BoxAt box) {
  const Box6 bi = box(i);
  const uint32_t lo = i > radius ? i - radius : 0u, hi = min(m - 1u, i + radius);
  float best = 3.402823466e+38f;
  uint32_t bj = i;
  for (uint32_t j = lo; j <= hi; ++j) {  // ascending j + strict '<': ties go to the lower index (guarantees a mutual pair)
    if (j == i) continue;
    const float a = half_area(box_union(bi, box(j)));
    if (a < best || bj == i) { best = a; bj = j; }
  }
  return bj;
}
// a mutual pair merges at its lower position; the upper one leaves the list
struct PlocFlags { uint32_t merge, keep; };
template <class NnAt> RT_DI PlocFlags ploc_flags(uint32_t i, NnAt nn) {
  const uint32_t j = nn(i);
  const bool mutual = j != i && nn(j) == i;
  return PlocFlags{(mutual && i < j) ? 1u : 0u, (mutual && i > j) ? 0u : 1u};
}
// node `id` over the clusters ra and rb: links, size and the fitted box (widen: no bottom-up pass); returns the new cluster's box
RT_DI Box6 ploc_merge(const BinaryTree& t, uint32_t* subtree, uint32_t id, uint32_t ra, uint32_t rb, uint32_t size, const Box6& ba, const Box6& bb,
                      float pad) {
  t.left[id] = ra; t.right[id] = rb;
  if (ra & kLeafBit) t.leaf_parent[ra & ~kLeafBit] = id; else t.node_parent[ra] = id;
  if (rb & kLeafBit) t.leaf_parent[rb & ~kLeafBit] = id; else t.node_parent[rb] = id;
  subtree[id] = size;
  const Box6 u = box_union(ba, bb);
  t.node_box[id] = widen(u, pad);
  return u;
}

__global__ void __launch_bounds__(256) k_ploc_init(const Box6* __restrict__ tri_box, const uint32_t* __restrict__ sorted_ids, uint32_t n,
                                                    uint32_t* __restrict__ cl_ref, Box6* __restrict__ cl_box) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  cl_ref[k] = kLeafBit | k;
  cl_box[k] = tri_box[sorted_ids[k]];
}
// The round kernels take the live cluster count m (and the nodes created so far) from device memory: the host only knows an upper
// bound of m (the grid), refreshed every few rounds, so that a round does not cost a host round trip (k_ploc_advance).
__global__ void __launch_bounds__(256) k_ploc_nearest(const Box6* __restrict__ cl_box, const uint32_t* __restrict__ state, uint32_t radius,
                                                       uint32_t* __restrict__ nn) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t m = state[0];
  if (i >= m) return;
  nn[i] = ploc_nearest(i, m, radius, [&](uint32_t j) { return cl_box[j]; });
}
__global__ void __launch_bounds__(256) k_ploc_flags(const uint32_t* __restrict__ nn, const uint32_t* __restrict__ state, uint32_t bound,
                                                     uint32_t* __restrict__ merge, uint32_t* __restrict__ keepc) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= bound) return;
  const uint32_t m = state[0];
  if (i >= m) { merge[i] = 0u; keepc[i] = 0u; return; }  // the scans run over the host's bound
  const PlocFlags f = ploc_flags(i, [&](uint32_t j) { return nn[j]; });
  merge[i] = f.merge;
  keepc[i] = f.keep;
}
__global__ void __launch_bounds__(256) k_ploc_apply(const uint32_t* __restrict__ nn, const uint32_t* __restrict__ merge,
                                                     const uint32_t* __restrict__ keepc, const uint32_t* __restrict__ merge_scan,
                                                     const uint32_t* __restrict__ keep_scan, const uint32_t* __restrict__ state, uint32_t last_id,
                                                     const uint32_t* __restrict__ cl_ref, const Box6* __restrict__ cl_box,
                                                     uint32_t* __restrict__ cl_ref_out, Box6* __restrict__ cl_box_out, BinaryTree tree,
                                                     uint32_t* __restrict__ subtree, float pad) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t m = state[0], next_id = last_id - state[1];  // last_id = n - 2: ids count down from it as nodes are created
  if (i >= m || !keepc[i]) return;
  const uint32_t pos = keep_scan[i];
  if (!merge[i]) { cl_ref_out[pos] = cl_ref[i]; cl_box_out[pos] = cl_box[i]; return; }
  const uint32_t j = nn[i], id = next_id - merge_scan[i];  // ids count down: the last merge of all creates node 0, the root
  const uint32_t ra = cl_ref[i], rb = cl_ref[j];
  cl_ref_out[pos] = id;
  cl_box_out[pos] = ploc_merge(tree, subtree, id, ra, rb, ploc_size(ra, subtree) + ploc_size(rb, subtree), cl_box[i], cl_box[j], pad);
}
// closes a round: state = {m - merged, created + merged}
__global__ void k_ploc_advance(const uint32_t* __restrict__ merge, const uint32_t* __restrict__ merge_scan, uint32_t* __restrict__ state) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const uint32_t m = state[0];
  if (m == 0u) return;
  const uint32_t merged = merge_scan[m - 1u] + merge[m - 1u];
  state[0] = m - merged;
  state[1] += merged;
}
// The last rounds in ONE workgroup: once kPlocTail or fewer clusters are left (27 of the ~60 rounds of a million-triangle build)
// a round is far shorter than its six launches and two host round trips.  The same three steps over LDS, the same ids (next_id -
// exclusive scan of the merge flags) as the global kernels: the tree is bit for bit the same.
__global__ void __launch_bounds__(kPlocTail) k_ploc_tail(uint32_t m, uint32_t radius, uint32_t next_id, const uint32_t* __restrict__ cl_ref_in,
                                                          const Box6* __restrict__ cl_box_in, BinaryTree tree, uint32_t* subtree, float pad) {
  __shared__ uint32_t s_ref[2][kPlocTail], s_size[2][kPlocTail];  // s_size: triangles below the cluster (subtree[] of this kernel's own
  __shared__ Box6 s_box[2][kPlocTail];                            // nodes is only written, never read back through the caches)
  __shared__ uint32_t s_nn[kPlocTail];
  __shared__ uint32_t s_wave[kPlocTail / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  int cur = 0;
  if (tid < m) { const uint32_t r = cl_ref_in[tid]; s_ref[0][tid] = r; s_size[0][tid] = ploc_size(r, subtree); s_box[0][tid] = cl_box_in[tid]; }
  __syncthreads();
  while (m > 1u) {
    if (tid < m) s_nn[tid] = ploc_nearest(tid, m, radius, [&](uint32_t j) { return s_box[cur][j]; });
    __syncthreads();
    PlocFlags f{0u, 0u};
    if (tid < m) f = ploc_flags(tid, [&](uint32_t j) { return s_nn[j]; });
    // one block-wide scan for both flags: merge count in the high half, keep count in the low half (<= 512 each)
    const uint32_t packed = (f.merge << 16) | f.keep;
    uint32_t incl = packed;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
      if (lane >= (uint32_t)d) incl += up;
    }
    if (lane == 63u) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t w = 0; w < kPlocTail / 64; ++w) { const uint32_t v = s_wave[w]; if (w < wave) before += v; total += v; }
    const uint32_t excl = before + incl - packed;
    const uint32_t merge_scan = excl >> 16, keep_scan = excl & 0xffffu;
    if (tid < m && f.keep) {
      if (!f.merge) { s_ref[cur ^ 1][keep_scan] = s_ref[cur][tid]; s_size[cur ^ 1][keep_scan] = s_size[cur][tid]; s_box[cur ^ 1][keep_scan] = s_box[cur][tid]; }
      else {
        const uint32_t j = s_nn[tid], id = next_id - merge_scan, size = s_size[cur][tid] + s_size[cur][j];
        s_ref[cur ^ 1][keep_scan] = id; s_size[cur ^ 1][keep_scan] = size;
        s_box[cur ^ 1][keep_scan] = ploc_merge(tree, subtree, id, s_ref[cur][tid], s_ref[cur][j], size, s_box[cur][tid], s_box[cur][j], pad);
      }
    }
    __syncthreads();
    next_id -= total >> 16;
    m = total & 0xffffu;
    cur ^= 1;
  }
}
// position of leaf k / first position of node i in the depth-first order of the finished tree: the sizes of all left
// siblings passed on the way up
RT_DI uint32_t ploc_offset(uint32_t ref, uint32_t p, const BinaryTree& t, const uint32_t* __restrict__ subtree) {
  uint32_t pos = 0;
  while (p != kAbsent) {
    if (t.right[p] == ref) pos += ploc_size(t.left[p], subtree);
    ref = p;
    p = t.node_parent[p];
  }
  return pos;
}
__global__ void __launch_bounds__(256) k_ploc_leaf_order(BinaryTree tree, const uint32_t* __restrict__ subtree, const uint32_t* __restrict__ sorted_ids,
                                                          uint32_t n, uint32_t* __restrict__ new_pos, uint32_t* __restrict__ sorted_ids_out,
                                                          uint32_t* __restrict__ leaf_parent_out) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const uint32_t pos = ploc_offset(kLeafBit | k, tree.leaf_parent[k], tree, subtree);
  new_pos[k] = pos;
  sorted_ids_out[pos] = sorted_ids[k];
  leaf_parent_out[pos] = tree.leaf_parent[k];
}
__global__ void __launch_bounds__(256) k_ploc_node_ranges(BinaryTree tree, const uint32_t* __restrict__ subtree, uint32_t n_internal) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_internal) return;
  const uint32_t off = ploc_offset(i, tree.node_parent[i], tree, subtree);
  tree.first[i] = off;
  tree.last[i] = off + subtree[i] - 1u;
}
__global__ void __launch_bounds__(256) k_ploc_renumber(BinaryTree tree, const uint32_t* __restrict__ new_pos, uint32_t n_internal) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_internal) return;
  const uint32_t l = tree.left[i], r = tree.right[i];
  if (l & kLeafBit) tree.left[i] = kLeafBit | new_pos[l & ~kLeafBit];
  if (r & kLeafBit) tree.right[i] = kLeafBit | new_pos[r & ~kLeafBit];
}

struct PlocScratch {
  Dev<uint32_t> ref[2], nn, merge, keepc, merge_scan, keep_scan, subtree, new_pos, ids2, lp2, state;
  Dev<Box6> box[2];
  Dev<char> tmp;  // rocPRIM's
  DevList plan(uint32_t n) {
    size_t tmp_bytes = 0;
    (void)exclusive_sum(nullptr, tmp_bytes, nullptr, nullptr, n, 0);
    return {ref[0].of(n), box[0].of(n), ref[1].of(n), box[1].of(n), nn.of(n), merge.of(n), keepc.of(n), merge_scan.of(n), keep_scan.of(n),
            new_pos.of(n), ids2.of(n), lp2.of(n), subtree.of(n - 1), tmp.of(tmp_bytes), state.of(2)};
  }
};

}  // namespace

size_t ploc_scratch_bytes(uint32_t n) { return arena_bytes(PlocScratch().plan(n)); }

std::string ploc_hierarchy(const HierarchyJob& job, hipStream_t s) {
  const uint32_t n = job.n, ni = n - 1;
  const BinaryTree& t = job.tree;
  PlocScratch sc;
  std::string e = alloc_all(sc.plan(n));
  if (!e.empty()) return e;
  hipLaunchKernelGGL(k_ploc_init, dim3(nblk(n)), dim3(256), 0, s, job.tri_box, job.sorted_ids, n, sc.ref[0], sc.box[0]);
  uint32_t m = n, created = 0;
  int cur = 0;
  const uint32_t radius = kPlocRadius;
  const bool tail = job.opt.ploc_tail != 2u;  // 2: every round as separate launches
  // rounds between two looks at the device's counters: a look is a host round trip (~50 us, as long as a late round itself); the
  // grid of the rounds in between is sized for the count of the last look (clusters only get fewer).  Same tree for any value.
  const uint32_t look_every = job.opt.ploc_look_every ? job.opt.ploc_look_every : 6u;
  const uint32_t init_state[2] = {n, 0u};
  HIP_TRY(hipMemcpyAsync(sc.state, init_state, 8, hipMemcpyHostToDevice, s));
  while (m > 1) {
    if (tail && m <= kPlocTail) {
      hipLaunchKernelGGL(k_ploc_tail, dim3(1), dim3(kPlocTail), 0, s, m, radius, (ni - 1u) - created, sc.ref[cur], sc.box[cur], t, sc.subtree, job.pad);
      break;
    }
    const uint32_t bound = m;
    for (uint32_t round = 0; round < look_every; ++round) {
      hipLaunchKernelGGL(k_ploc_nearest, dim3(nblk(bound)), dim3(256), 0, s, sc.box[cur], sc.state, radius, sc.nn);
      hipLaunchKernelGGL(k_ploc_flags, dim3(nblk(bound)), dim3(256), 0, s, sc.nn, sc.state, bound, sc.merge, sc.keepc);
      size_t tb = sc.tmp.bytes;
      HIP_TRY(exclusive_sum(sc.tmp.raw, tb, sc.merge.get(), sc.merge_scan.get(), bound, s));
      tb = sc.tmp.bytes;
      HIP_TRY(exclusive_sum(sc.tmp.raw, tb, sc.keepc.get(), sc.keep_scan.get(), bound, s));
      hipLaunchKernelGGL(k_ploc_apply, dim3(nblk(bound)), dim3(256), 0, s, sc.nn, sc.merge, sc.keepc, sc.merge_scan, sc.keep_scan, sc.state, ni - 1u,
                         sc.ref[cur], sc.box[cur], sc.ref[cur ^ 1], sc.box[cur ^ 1], t, sc.subtree, job.pad);
      hipLaunchKernelGGL(k_ploc_advance, dim3(1), dim3(64), 0, s, sc.merge, sc.merge_scan, sc.state);
      cur ^= 1;
    }
    uint32_t now[2] = {0u, 0u};
    HIP_TRY(hipMemcpyAsync(now, sc.state, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (now[0] >= m) return "bvh_build: PLOC made no progress";  // cannot happen: the closest pair is always mutual
    m = now[0];
    created = now[1];
  }
  static const uint32_t absent = kAbsent;
  HIP_TRY(hipMemcpyAsync(t.node_parent, &absent, 4, hipMemcpyHostToDevice, s));  // node 0 is the root
  hipLaunchKernelGGL(k_ploc_leaf_order, dim3(nblk(n)), dim3(256), 0, s, t, sc.subtree, job.sorted_ids, n, sc.new_pos, sc.ids2, sc.lp2);
  hipLaunchKernelGGL(k_ploc_node_ranges, dim3(nblk(ni)), dim3(256), 0, s, t, sc.subtree, ni);
  hipLaunchKernelGGL(k_ploc_renumber, dim3(nblk(ni)), dim3(256), 0, s, t, sc.new_pos, ni);
  HIP_TRY(hipMemcpyAsync(job.sorted_ids, sc.ids2, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(t.leaf_parent, sc.lp2, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipGetLastError());
  return "";
}

}  // namespace rt
