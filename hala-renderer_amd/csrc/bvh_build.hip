// bvh_build.hip — K1/K3/K4 of SURVEY.md §2.1: what the reference hands to the Vulkan driver through
// HalaAccelerationStructure::new (src/scene/loader/gpu_uploader.rs:784-811 BLAS per primitive, :937-959 TLAS),
// done here on the GPU for gfx950.  One pipeline, every arrow one host function below:
//   bvh_build : flatten+bounds -> hierarchy (sah | ploc | lbvh) -> leaf boxes -> [lbvh only: k_fit] -> collapse -> pack levels
//   bvh_refit : flatten+bounds ->                                  leaf boxes ->                                    pack levels
//   flatten     every instance (node x primitive, in the reference's instance order gpu_uploader.rs:843-875) is transformed to world
//               space once -> one triangle soup, one BVH (288 GB of HBM make the copy free and single-level traversal needs no
//               per-instance ray transform)
//   hierarchy   a binary tree over the triangles (bvh_build_impl.h: HierarchyJob): >= 4096 triangles: top-down full-sweep SAH
//               (bvh_sah.hip) | below: 60-bit Morton codes -> rocPRIM radix sort -> Karras 2012 LBVH (here) |
//               hala_rt_build_options::builder = 2: PLOC over the Morton order, the fast large-scene build (bvh_ploc.hip)
//   collapse    the cheapest 4-wide tree the hierarchy holds: a bottom-up pass prices, per binary node and per number of parent slots,
//               every cut (node visits and leaf items weighted by surface area; a leaf holds <= leaf_max triangles), then the 4-nodes
//               are filled top-down from the recorded choices, breadth-first.  The same rule for every hierarchy and for the instance
//               levels.  The 4-wide topology is what is kept; the binary tree is scratch of the build
//   pack levels one launch per level, deepest first: 64-B compressed nodes (8-bit child boxes quantised conservatively against the
//               node's own box, RENDER_SPEC §4.1b; bvh_node_pack.h).  The same pass after a build and after a refit
//   refit       (north_star; the reference only rebuilds) re-flatten + re-pack on the frozen topology
// Results are validated against the oracle through traversal results and a structural check, never topology.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include <vector>

#include "bvh_build_impl.h"

namespace rt {

namespace {

// RENDER_SPEC §3: p' = fma(m8,z, fma(m4,y, m0*x)) + m12
RT_DI f3 transform_point(const float* m, f3 p) {
  return mk3(__fmaf_rn(m[8], p.z, __fmaf_rn(m[4], p.y, m[0] * p.x)) + m[12], __fmaf_rn(m[9], p.z, __fmaf_rn(m[5], p.y, m[1] * p.x)) + m[13],
             __fmaf_rn(m[10], p.z, __fmaf_rn(m[6], p.y, m[2] * p.x)) + m[14]);
}

// one thread per global triangle id.  The three records a triangle gets (48-B Tri, 128-B ShadeTri, 24-B Box6) are staged in LDS and
// leave the block as contiguous 16-B (8-B for the boxes) stores.  Scene bounds: NO global atomics here — a device-scope atomic
// costs 11.4 ns per 128-B line however many waves issue it (scripts/microbench/atomic_rate.hip), and six of them per wave on one
// line held this kernel at 1.07 ms per million triangles; each block leaves its bounds in block_ord and k_bounds_reduce folds them.
__global__ void __launch_bounds__(256) k_flatten(const hala_gpu_mesh_data* __restrict__ prims, const uint32_t* __restrict__ first_tri,
                                                  uint32_t inst_count, uint32_t n, Tri* __restrict__ tris_by_id, ShadeTri* __restrict__ shade_tris,
                                                  Box6* __restrict__ tri_box,
                                                  uint32_t* __restrict__ block_ord /* [gridDim.x][6] min xyz, max xyz */,
                                                  const uint32_t* __restrict__ gid_first, const uint32_t* __restrict__ inst_index, int object_space) {
  __shared__ float4 stage[256 * 8];
  __shared__ uint32_t wave_ord[4][6];
  const uint32_t tid = threadIdx.x, base = blockIdx.x * 256u, g = base + tid;
  const uint32_t cnt = min(256u, n - base);
  uint32_t ord[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u};
  float4 tri[3];
  Box6 b;
  if (g < n) {
    uint32_t lo = 0, hi = inst_count;  // last instance with first_tri <= g
    while (hi - lo > 1u) {
      const uint32_t mid = (lo + hi) >> 1;
      if (first_tri[mid] <= g) lo = mid; else hi = mid;
    }
    const hala_gpu_mesh_data& md = prims[lo];
    const uint32_t lt = g - first_tri[lo];
    const uint32_t* idx = reinterpret_cast<const uint32_t*>(md.indices) + 3 * (size_t)lt;
    const hala_vertex* vb = reinterpret_cast<const hala_vertex*>(md.vertices);
    f3 v[3];
    ShadeTri st{};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const hala_vertex& vx = vb[idx[c]];
      v[c] = object_space ? ld3(vx.position) : transform_point(md.transform, ld3(vx.position));  // RENDER_SPEC 4.5: an instanced primitive keeps its local positions
      float* nc = c == 0 ? st.n0 : (c == 1 ? st.n1 : st.n2);
#pragma unroll
      for (int k = 0; k < 3; ++k) { nc[k] = vx.normal[k]; st.tg[c][k] = vx.tangent[k]; }
      st.uv[c][0] = vx.tex_coord[0]; st.uv[c][1] = vx.tex_coord[1];
    }
    const uint32_t inst = inst_index ? inst_index[lo] : lo;
    st.inst = inst; st.material = md.material_index;
    const f3 e1 = v[1] - v[0], e2 = v[2] - v[0];
    const f3 gc = cross3(e1, e2);  // RENDER_SPEC 6: the geometric normal is normalize(cross(e1, e2)) of the stored world-space edges
    st.gcross[0] = gc.x; st.gcross[1] = gc.y; st.gcross[2] = gc.z;
    tri[0] = make_float4(v[0].x, v[0].y, v[0].z, __uint_as_float(gid_first ? gid_first[lo] + lt : g));
    tri[1] = make_float4(e1.x, e1.y, e1.z, 0.0f);
    tri[2] = make_float4(e2.x, e2.y, e2.z, 0.0f);
    b.mn[0] = fminf(v[0].x, fminf(v[1].x, v[2].x)); b.mx[0] = fmaxf(v[0].x, fmaxf(v[1].x, v[2].x));
    b.mn[1] = fminf(v[0].y, fminf(v[1].y, v[2].y)); b.mx[1] = fmaxf(v[0].y, fmaxf(v[1].y, v[2].y));
    b.mn[2] = fminf(v[0].z, fminf(v[1].z, v[2].z)); b.mx[2] = fmaxf(v[0].z, fmaxf(v[1].z, v[2].z));
#pragma unroll
    for (int k = 0; k < 3; ++k) { ord[k] = f2ord(b.mn[k]); ord[3 + k] = f2ord(b.mx[k]); }
    const float4* sp = reinterpret_cast<const float4*>(&st);
#pragma unroll
    for (int k = 0; k < 8; ++k) stage[tid * 8u + k] = sp[k];
  }
  __syncthreads();
  {
    float4* out = reinterpret_cast<float4*>(shade_tris + base);
    for (uint32_t i = tid; i < cnt * 8u; i += 256u) out[i] = stage[i];
  }
  __syncthreads();
  if (g < n) { stage[tid * 3u] = tri[0]; stage[tid * 3u + 1u] = tri[1]; stage[tid * 3u + 2u] = tri[2]; }
  __syncthreads();
  {
    float4* out = reinterpret_cast<float4*>(tris_by_id + base);
    for (uint32_t i = tid; i < cnt * 3u; i += 256u) out[i] = stage[i];
  }
  __syncthreads();
  float2* stage2 = reinterpret_cast<float2*>(stage);
  if (g < n) {
    stage2[tid * 3u] = make_float2(b.mn[0], b.mn[1]); stage2[tid * 3u + 1u] = make_float2(b.mn[2], b.mx[0]);
    stage2[tid * 3u + 2u] = make_float2(b.mx[1], b.mx[2]);
  }
  __syncthreads();
  {
    float2* out = reinterpret_cast<float2*>(tri_box + base);
    for (uint32_t i = tid; i < cnt * 3u; i += 256u) out[i] = stage2[i];
  }
  block_bounds_fold(ord, wave_ord, tid, block_ord, blockIdx.x * 6u);
}
// one block: folds the per-block bounds of k_flatten into scene_ord[6]
__global__ void __launch_bounds__(256) k_bounds_reduce(const uint32_t* __restrict__ block_ord, uint32_t blocks, uint32_t* __restrict__ scene_ord) {
  __shared__ uint32_t wave_ord[4][6];
  uint32_t ord[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u};
  for (uint32_t b = threadIdx.x; b < blocks; b += 256u) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { ord[k] = min(ord[k], block_ord[b * 6u + k]); ord[3 + k] = max(ord[3 + k], block_ord[b * 6u + 3 + k]); }
  }
  block_bounds_fold(ord, wave_ord, threadIdx.x, scene_ord, 0u);
}

RT_DI unsigned long long spread21(uint32_t v) {  // 21 bits -> every third bit
  unsigned long long x = v & 0x1fffffull;
  x = (x | x << 32) & 0x1f00000000ffffull;
  x = (x | x << 16) & 0x1f0000ff0000ffull;
  x = (x | x << 8) & 0x100f00f00f00f00full;
  x = (x | x << 4) & 0x10c30c30c30c30c3ull;
  x = (x | x << 2) & 0x1249249249249249ull;
  return x;
}
__global__ void __launch_bounds__(256) k_morton(const Box6* __restrict__ tri_box, uint32_t n, const uint32_t* __restrict__ scene_ord,
                                                 unsigned long long* __restrict__ keys, uint32_t* __restrict__ ids) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const Box6 b = tri_box[g];
  uint32_t q[3];
  float scene_d2 = 0.0f, tri_d2 = 0.0f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float lo = ord2f(scene_ord[k]), hi = ord2f(scene_ord[3 + k]);
    const float c = 0.5f * (b.mn[k] + b.mx[k]);
    const float ext = hi - lo;
    float t = ext > 0.0f ? (c - lo) / ext : 0.0f;
    t = fminf(fmaxf(t, 0.0f), 1.0f);
    q[k] = min((uint32_t)(t * 1048576.0f), 1048575u);  // 20 bits per axis
    scene_d2 += ext * ext;
    tri_d2 += (b.mx[k] - b.mn[k]) * (b.mx[k] - b.mn[k]);
  }
  // Size class in the two top key bits: LBVH sorts by centroid only, so one huge triangle (a ground quad, a wall) would
  // inflate the boxes of every ancestor it shares with small neighbours.  With the class on top of the key the Karras
  // hierarchy splits by class first: big triangles form their own shallow subtrees next to the well-formed rest.
  // class 0: box diagonal > 1/8 of the scene's, 1: > 1/32, 2: > 1/128, 3: the rest.
  const float ratio2 = scene_d2 > 0.0f ? tri_d2 / scene_d2 : 0.0f;
  const uint32_t cls = ratio2 > (1.0f / 64.0f) ? 0u : (ratio2 > (1.0f / 1024.0f) ? 1u : (ratio2 > (1.0f / 16384.0f) ? 2u : 3u));
  keys[g] = ((unsigned long long)cls << 60) | (spread21(q[0]) << 2) | (spread21(q[1]) << 1) | spread21(q[2]);
  ids[g] = g;
}

// ---- Karras 2012 ------------------------------------------------------------------------------------------
RT_DI int delta(const unsigned long long* keys, int n, int i, int j) {
  if (j < 0 || j >= n) return -1;
  const unsigned long long a = keys[i], b = keys[j];
  if (a == b) return 64 + __clz((uint32_t)i ^ (uint32_t)j);
  return __clzll((long long)(a ^ b));
}
__global__ void __launch_bounds__(256) k_hierarchy(const unsigned long long* __restrict__ keys, int n, BinaryTree tree) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n - 1) return;
  const int d = (delta(keys, n, i, i + 1) - delta(keys, n, i, i - 1)) >= 0 ? 1 : -1;
  const int dmin = delta(keys, n, i, i - d);
  int lmax = 2;
  while (delta(keys, n, i, i + lmax * d) > dmin) lmax *= 2;
  int l = 0;
  for (int t = lmax / 2; t >= 1; t /= 2)
    if (delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
  const int j = i + l * d;
  const int dnode = delta(keys, n, i, j);
  int s = 0, t = l;
  do {
    t = (t + 1) >> 1;
    if (delta(keys, n, i, i + (s + t) * d) > dnode) s += t;
  } while (t > 1);
  const int gamma = i + s * d + min(d, 0);
  const int lo = min(i, j), hi = max(i, j);
  const uint32_t lc = (lo == gamma) ? (kLeafBit | (uint32_t)gamma) : (uint32_t)gamma;
  const uint32_t rc = (hi == gamma + 1) ? (kLeafBit | (uint32_t)(gamma + 1)) : (uint32_t)(gamma + 1);
  tree.left[i] = lc; tree.right[i] = rc; tree.first[i] = (uint32_t)lo; tree.last[i] = (uint32_t)hi;
  if (lc & kLeafBit) tree.leaf_parent[gamma] = (uint32_t)i; else tree.node_parent[gamma] = (uint32_t)i;
  if (rc & kLeafBit) tree.leaf_parent[gamma + 1] = (uint32_t)i; else tree.node_parent[gamma + 1] = (uint32_t)i;
  if (i == 0) tree.node_parent[0] = kAbsent;
}

__global__ void __launch_bounds__(256) k_leaf_boxes(const Box6* __restrict__ tri_box, const uint32_t* __restrict__ sorted_ids, uint32_t n,
                                                     Box6* __restrict__ leaf_box, const Tri* __restrict__ tris_by_id, Tri* __restrict__ tris, float pad,
                                                     Tri* __restrict__ tris_any, const ShadeTri* __restrict__ shade_tris,
                                                     const uint8_t* __restrict__ any_class, uint32_t material_count,
                                                     const uint8_t* __restrict__ material_kind) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const uint32_t id = sorted_ids[k];
  const uint32_t mat = shade_tris[id].material;
  // word 11: the shading kind of the triangle's material; the closest-hit traversal puts it into the hit record (hala_types.h: hit_encode)
  const float kind_word = __uint_as_float(material_kind && mat < material_count ? (uint32_t)material_kind[mat] : kShadeKindSpecial);
  leaf_box[k] = widen(tri_box[id], pad);
  const float4* src = reinterpret_cast<const float4*>(tris_by_id + id);
  float4* dst = reinterpret_cast<float4*>(tris + k);
  dst[0] = src[0]; dst[1] = src[1]; dst[2] = make_float4(src[2].x, src[2].y, src[2].z, kind_word);
  if (tris_any) {  // RENDER_SPEC 7.1d: any-hit rays do not see surfaces of opacity exactly 0 — their triangles are degenerate in this copy —
                   // and decide per (ray key, triangle) whether a translucent one blocks them: those carry a flag in word 7
    const uint32_t cls = mat < material_count ? any_class[mat] : 0u;
    const bool gone = cls == 1u;
    float4* da = reinterpret_cast<float4*>(tris_any + k);
    da[0] = src[0];
    const uint32_t flag = cls == 2u ? 1u : (cls == 3u ? 2u : (cls == 4u ? 3u : 0u));  // bit 0: translucent, bit 1: boundary of a medium (7.1g)
    da[1] = gone ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : make_float4(src[1].x, src[1].y, src[1].z, __uint_as_float(flag));
    da[2] = gone ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : make_float4(src[2].x, src[2].y, src[2].z, kind_word);
  }
}

// bottom-up fit (after k_hierarchy only: the other builders fit as they go): the second thread to arrive at a node owns it.
// Producer: stores -> __threadfence (agent release) -> atomic arrival; consumer: atomic arrival -> __threadfence (agent acquire) -> loads.
__global__ void __launch_bounds__(256) k_fit(BinaryTree tree, const Box6* __restrict__ leaf_box, uint32_t* arrivals, uint32_t n) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  uint32_t p = tree.leaf_parent[k];
  while (p != kAbsent) {
    __threadfence();
    const uint32_t old = atomicAdd(&arrivals[p], 1u);
    if (old == 0u) return;
    __threadfence();
    const uint32_t lc = tree.left[p], rc = tree.right[p];
    const volatile Box6* lb = (lc & kLeafBit) ? &leaf_box[lc & ~kLeafBit] : &tree.node_box[lc];
    const volatile Box6* rb = (rc & kLeafBit) ? &leaf_box[rc & ~kLeafBit] : &tree.node_box[rc];
    Box6 a, b;
#pragma unroll
    for (int c = 0; c < 3; ++c) { a.mn[c] = lb->mn[c]; a.mx[c] = lb->mx[c]; b.mn[c] = rb->mn[c]; b.mx[c] = rb->mx[c]; }
    const Box6 u = box_union(a, b);
    volatile Box6* o = &tree.node_box[p];
#pragma unroll
    for (int c = 0; c < 3; ++c) { o->mn[c] = u.mn[c]; o->mx[c] = u.mx[c]; }
    p = tree.node_parent[p];
  }
}

// ---- which cut of the binary tree becomes the 4-wide tree -----------------------------------------------------------------------------
// A ray that enters a 4-node pays one node visit (one lane of the node phase); a ray that enters a leaf pays one leaf item (four lanes of
// the cooperative pass, however full the leaf is).  With the chance of entering taken as the fitted box's half area, a 4-wide tree costs
//   sum over inner nodes of A * kCollapseNodeCost  +  sum over leaves of A * kCollapseLeafCost
// and the cheapest tree over a binary hierarchy is found bottom-up.  For a binary node n of c(n) triangles, C(n, j) = the cheapest way
// to stand n's subtree in at most j slots of a parent:
//   D(n, j) = min over 1 <= k < j of C(left, k) + C(right, j - k)                       j = 2, 3, 4: n is opened, its children share the slots
//   C(n, 1) = min(A(n) * kCollapseLeafCost if c(n) <= leaf_max, A(n) * kCollapseNodeCost + D(n, 4))     one slot: a leaf, or a 4-node of its own
//   C(n, j) = min(D(n, j), C(n, j - 1))                                                  j = 2, 3
// A single triangle (item) is a leaf in one slot whatever it is offered.  Ties: the leaf before the inner node, the smaller k, and D(n, j)
// before C(n, j - 1) (an opened node is one visit fewer) — the tree is a pure function of the hierarchy.  Every sum is one binary32
// addition of two costs, every product one multiplication (the build has no contraction), so tests/collapse_ref.py repeats it bit for bit.
// Only the ratio of the two constants matters.  Static counts put it between 1.2 and 2.2 (a node visit: one lane of a ~200-instruction
// phase that runs at ~52 lanes; a leaf item: four lanes of a ~75-instruction pass at ~36 lanes), but the frame time of configs[3] is flat
// from 1.2 to 20 (7.77 - 7.82 ms, profiles/collapse_cost.txt): a dearer leaf buys fewer triangle tests with more node visits at the same
// price.  8 is kept for what the tests need from the trees: from 7 up the 600 000-triangle scene of tests/test_tree_quality.py keeps
// more nodes than one pass of k_tree_cost's grid, from 10 up the Cornell box gets a sixth node and configs[1] is slower.
// (make EXTRA="-DRT_COLLAPSE_LEAF_COST=2.0f" VARIANT=_r20 builds another ratio beside the library, like every tuning build.)
#ifndef RT_COLLAPSE_LEAF_COST
#define RT_COLLAPSE_LEAF_COST 8.0f
#endif
constexpr float kCollapseNodeCost = 1.0f, kCollapseLeafCost = RT_COLLAPSE_LEAF_COST;
// choice word of a binary node: bit 0 = C(n, 1) is the inner node (keep); bits 2-3 / 4-5 = the k of C(n, 2) / C(n, 3), 0 = "as with one
// slot fewer"; bits 6-7 = the k of D(n, 4)
constexpr uint32_t kChoiceInner = 1u, kChoiceShift2 = 2u, kChoiceShift3 = 4u, kChoiceShift4 = 6u;

// cost[3 * p + j - 1] = C(p, j), choice[p], keep[p] (1 where the node, offered one slot, is an inner 4-node) of one binary node whose
// children are done
RT_DI void collapse_cost_node(const BinaryTree& tree, const Box6* __restrict__ leaf_box, uint32_t p, uint32_t leaf_max, float* cost,
                              uint32_t* __restrict__ choice, uint32_t* __restrict__ keep) {
  const uint32_t ref[2] = {tree.left[p], tree.right[p]};
  float c[2][3];
#pragma unroll
  for (int side = 0; side < 2; ++side) {
    if (ref[side] & kLeafBit) {
      c[side][0] = c[side][1] = c[side][2] = half_area(leaf_box[ref[side] & ~kLeafBit]) * kCollapseLeafCost;
    } else {
      const volatile float* src = cost + 3u * (size_t)ref[side];
      c[side][0] = src[0]; c[side][1] = src[1]; c[side][2] = src[2];
    }
  }
  const float d2 = c[0][0] + c[1][0];
  float d3 = c[0][0] + c[1][1], d4 = c[0][0] + c[1][2];
  uint32_t k3 = 1u, k4 = 1u;
  { const float v = c[0][1] + c[1][0]; if (v < d3) { d3 = v; k3 = 2u; } }
  { const float v = c[0][1] + c[1][1]; if (v < d4) { d4 = v; k4 = 2u; } }
  { const float v = c[0][2] + c[1][0]; if (v < d4) { d4 = v; k4 = 3u; } }
  const float area = half_area(tree.node_box[p]);
  const float as_leaf = area * kCollapseLeafCost, as_inner = area * kCollapseNodeCost + d4;
  const bool inner = !((tree.last[p] - tree.first[p] + 1u) <= leaf_max && as_leaf <= as_inner);
  const float c1 = inner ? as_inner : as_leaf;
  const bool open2 = d2 <= c1;
  const float c2 = open2 ? d2 : c1;
  const bool open3 = d3 <= c2;
  const float c3 = open3 ? d3 : c2;
  volatile float* dst = cost + 3u * (size_t)p;
  dst[0] = c1; dst[1] = c2; dst[2] = c3;
  choice[p] = (inner ? kChoiceInner : 0u) | ((open2 ? 1u : 0u) << kChoiceShift2) | ((open3 ? k3 : 0u) << kChoiceShift3) | (k4 << kChoiceShift4);
  keep[p] = inner ? 1u : 0u;
}

// Bottom-up over the binary tree, every node once.  With one fenced device-scope arrival per leaf and per node the pass took 5.09 ms
// for 1 M triangles, as it stands 0.85 ms (profiles/collapse_cost.txt): the bottom of the tree goes without arrivals.  A treelet = a
// node of at most kTreeletMax triangles whose parent has more; ONE thread walks it in post-order along the parent links (no stack, no
// fence: it reads what it wrote).  Above the treelets k_fit's pattern: whoever finishes a child arrives at the parent, the second to arrive owns it and goes on;
// nobody waits.  Producer: stores -> __threadfence -> atomic arrival; consumer: atomic arrival -> __threadfence -> loads.
// Threads 0 .. n - 1 stand for the leaves (a leaf arrives for itself where its parent is above the treelets), n .. 2 n - 2 for the nodes.
constexpr uint32_t kTreeletMax = 32u;
__global__ void __launch_bounds__(256) k_collapse_cost(BinaryTree tree, const Box6* __restrict__ leaf_box, uint32_t* arrivals, uint32_t n,
                                                        uint32_t leaf_max, float* cost, uint32_t* __restrict__ choice, uint32_t* __restrict__ keep) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= 2u * n - 1u) return;
  uint32_t p;
  if (g < n) {
    p = tree.leaf_parent[g];
    if (tree.last[p] - tree.first[p] + 1u <= kTreeletMax) return;  // inside a treelet
  } else {
    const uint32_t root = g - n;
    if (tree.last[root] - tree.first[root] + 1u > kTreeletMax) return;
    p = tree.node_parent[root];
    if (p != kAbsent && tree.last[p] - tree.first[p] + 1u <= kTreeletMax) return;  // inside a treelet, not its root
    uint32_t node = root;
    int from = 0;  // 0: from the parent, 1: the left child is done, 2: both are
    for (;;) {
      if (from == 0) {
        const uint32_t l = tree.left[node];
        if (!(l & kLeafBit)) { node = l; continue; }
        from = 1;
      }
      if (from == 1) {
        const uint32_t r = tree.right[node];
        if (!(r & kLeafBit)) { node = r; from = 0; continue; }
      }
      collapse_cost_node(tree, leaf_box, node, leaf_max, cost, choice, keep);
      if (node == root) break;
      const uint32_t up = tree.node_parent[node];
      from = tree.left[up] == node ? 1 : 2;
      node = up;
    }
  }
  while (p != kAbsent) {
    __threadfence();
    const uint32_t old = atomicAdd(&arrivals[p], 1u);
    if (old == 0u) return;
    __threadfence();
    collapse_cost_node(tree, leaf_box, p, leaf_max, cost, choice, keep);
    p = tree.node_parent[p];
  }
}

// ---- 4-wide nodes (RENDER_SPEC §4.1b) -----------------------------------------------------------------------------------------------
RT_DI uint32_t leaf_ref(uint32_t first, uint32_t count) { return kLeafRef | ((count - 1u) << 28) | first; }
// the one place a leaf's child reference comes from: its sorted positions, or (ITEMS: leaves of one item) the reference of the item there
template <bool ITEMS>
RT_DI uint32_t leaf_ref_of(uint32_t first, uint32_t count, const uint32_t* __restrict__ sorted_ids, const uint32_t* __restrict__ item_ref) {
  if (ITEMS) return item_ref[sorted_ids[first]];
  return leaf_ref(first, count);
}

// Top-down collapse of the binary tree into 4-wide nodes, one BFS level per launch, so that node indices come out in
// breadth-first order (the first `lds_nodes` nodes — the slice the traversal kernels stage in LDS — are the top of the
// tree, which every ray visits).  The 4-node rooted at binary node i is the cut k_collapse_cost recorded for D(i, 4): i's children
// share the four slots as its choice word says, and every child that was given more than one slot is opened, or not, as its own
// word says for that many — at most three openings, left to right.  A child left in one slot is a leaf or the root of a 4-node (keep).
// refs4[node] = the binary-tree references its slots were filled from — the frozen topology refit re-packs from.
// The level kernels take the level's first node and size from device memory (level[0], level[1]; k_level_advance closes a level):
// the host only knows an upper bound of the size — the grid — and looks at the counters every few levels.
__global__ void __launch_bounds__(256) k_collapse_level(const uint32_t* __restrict__ root_of, const uint32_t* __restrict__ level, uint32_t bound,
                                                         BinaryTree tree, const uint32_t* __restrict__ keep, const uint32_t* __restrict__ choice,
                                                         uint4* __restrict__ refs4, uint32_t* __restrict__ cnt) {
  const uint32_t* left = tree.left;
  const uint32_t* right = tree.right;
  const Box6* node_box = tree.node_box;
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= bound) return;
  const uint32_t base = level[0], size = level[1];
  if (j >= size) { cnt[j] = 0u; return; }  // the scan runs over the host's bound
  const uint32_t i = root_of[base + j];
  uint32_t c[4] = {kAbsent, kAbsent, kAbsent, kAbsent};
  int n = 0;
  uint32_t wait_ref[4], wait_slots[4];  // right siblings and the slots they were given
  int waiting = 0;
  uint32_t r = i, slots = 4u;
  bool opened = false;  // the root of the 4-node is opened whatever it says of itself
  for (;;) {
    uint32_t k = 0u;
    if (!(r & kLeafBit) && slots > 1u) {
      const uint32_t w = choice[r];
      k = (w >> (slots == 2u ? kChoiceShift2 : (slots == 3u ? kChoiceShift3 : kChoiceShift4))) & 3u;
      if (k == 0u && opened) { --slots; continue; }  // as with one slot fewer
      if (k == 0u || k >= slots) k = 1u;             // (no word the cost pass writes comes here)
    }
    if (k != 0u && waiting < 4) {
      wait_ref[waiting] = right[r]; wait_slots[waiting] = slots - k; ++waiting;
      r = left[r]; slots = k; opened = true;
      continue;
    }
    if (n < 4) c[n++] = r;
    if (waiting == 0) break;
    --waiting;
    r = wait_ref[waiting]; slots = wait_slots[waiting];
  }
  // Slot order = the order in which an any-hit ray of a large tree takes the inner children (RENDER_SPEC 4.4c): the kept inner children
  // by descending surface area, then the leaves in the order the opening left them.  configs[3]: 9.09 instead of 9.40 node visits per
  // connection ray (in-order slots), 3.40 instead of 3.45 ms per frame in the shadow passes; ascending area / triangle count / density:
  // 9.60 / 9.48 / 9.36.  Every other ray sorts the children by distance (the slot only breaks ties).
  float w[4];
  for (int k = 0; k < n; ++k) {
    const uint32_t r = c[k];
    w[k] = (r & kLeafBit) || !keep[r] ? -1.0f : half_area(node_box[r]);
  }
  for (int a = 1; a < n; ++a)  // insertion sort, descending weight, stable
    for (int b = a; b > 0 && w[b] > w[b - 1]; --b) {
      const float tw = w[b]; w[b] = w[b - 1]; w[b - 1] = tw;
      const uint32_t tc = c[b]; c[b] = c[b - 1]; c[b - 1] = tc;
    }
  refs4[base + j] = make_uint4(c[0], c[1], c[2], c[3]);
  uint32_t inner = 0;
  for (int k = 0; k < n; ++k) inner += (!(c[k] & kLeafBit) && keep[c[k]]) ? 1u : 0u;
  cnt[j] = inner;
}
__global__ void __launch_bounds__(256) k_scatter_level(uint32_t* __restrict__ root_of, const uint32_t* __restrict__ level, const uint4* __restrict__ refs4,
                                                        const uint32_t* __restrict__ keep, const uint32_t* __restrict__ off,
                                                        uint32_t* __restrict__ index4) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t base = level[0], size = level[1];
  if (j >= size) return;
  const uint4 q = refs4[base + j];
  const uint32_t c[4] = {q.x, q.y, q.z, q.w};
  uint32_t pos = base + size + off[j];
  for (int k = 0; k < 4; ++k) {
    const uint32_t r = c[k];
    if ((r & kLeafBit) || !keep[r]) continue;
    root_of[pos] = r;
    index4[r] = pos;
    ++pos;
  }
}
// closes a level: level = {base + size, inner children found, levels so far + 1}; bases[l] = first node of level l
__global__ void k_level_advance(const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ off, uint32_t* __restrict__ level,
                                uint32_t* __restrict__ bases, uint32_t max_levels) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const uint32_t base = level[0], size = level[1], l = level[2];
  if (size == 0u) return;
  if (l < max_levels) bases[l] = base;
  level[0] = base + size;
  level[1] = off[size - 1u] + cnt[size - 1u];
  level[2] = l + 1u;
}

// One BFS level of the kept 4-wide topology becomes 64-B nodes — after a build and after a refit alike.  box4 is scratch indexed by
// 4-NODE index (it lives in the binary tree's node_box, whose boxes are not needed once the tree is collapsed): a node leaves the union
// of its children there for its parent, one level up, which runs in a later launch.  The boxes are the fitted ones (min / max are exact:
// the union of a collapsed leaf's leaf boxes is the binary node's fitted box), no fences.
// ITEMS: a leaf's reference is the one its item brings (leaf_ref_of); false: the triangle trees, whose kernel the parameter leaves as it was.
template <bool ITEMS>
__global__ void __launch_bounds__(256) k_refit_level(const uint4* __restrict__ refs4, uint32_t base, uint32_t size, const uint32_t* __restrict__ first,
                                                      const uint32_t* __restrict__ last, const uint32_t* __restrict__ keep,
                                                      const uint32_t* __restrict__ index4, const Box6* __restrict__ leaf_box, Box6* box4,
                                                      BvhNode4* __restrict__ nodes, const uint32_t* __restrict__ sorted_ids,
                                                      const uint32_t* __restrict__ item_ref) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= size) return;
  const uint32_t idx = base + k;
  const uint4 q = refs4[idx];
  const uint32_t c[4] = {q.x, q.y, q.z, q.w};
  Child4 ch[4];
  int n = 0;
  for (int s = 0; s < 4; ++s) {
    const uint32_t r = c[s];
    if (r == kAbsent) continue;
    if (r & kLeafBit) { ch[n].box = leaf_box[r & ~kLeafBit]; ch[n].ref = leaf_ref_of<ITEMS>(r & ~kLeafBit, 1u, sorted_ids, item_ref); }
    else if (!keep[r]) {
      const uint32_t f = first[r], l = last[r];
      Box6 u = leaf_box[f];
      for (uint32_t t = f + 1; t <= l; ++t) u = box_union(u, leaf_box[t]);
      ch[n].box = u; ch[n].ref = leaf_ref_of<ITEMS>(f, l - f + 1u, sorted_ids, item_ref);
    } else { ch[n].box = box4[index4[r]]; ch[n].ref = index4[r]; }
    ++n;
  }
  nodes[idx] = pack_node4(ch, n);
  Box6 all = ch[0].box;
  for (int s = 1; s < n; ++s) all = box_union(all, ch[s].box);
  box4[idx] = all;
}

// scene of <= leaf_max triangles: one 4-node with a single leaf child
template <bool ITEMS>
__global__ void k_emit_single4(const Box6* __restrict__ leaf_box, uint32_t n, BvhNode4* __restrict__ nodes, const uint32_t* __restrict__ sorted_ids,
                               const uint32_t* __restrict__ item_ref) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  Child4 ch[1];
  ch[0].box = Box6{};
  if (n > 0) {
    ch[0].box = leaf_box[0];
    for (uint32_t k = 1; k < n; ++k) ch[0].box = box_union(ch[0].box, leaf_box[k]);
  }
  ch[0].ref = n > 0 ? leaf_ref_of<ITEMS>(0u, n, sorted_ids, item_ref) : kAbsent;
  nodes[0] = pack_node4(ch, 1);
}

}  // namespace

DevList BuildScratch::plan(uint32_t n, bool morton) {
  const size_t ni = n > 1 ? n - 1 : 1;
  size_t scan_bytes = 0, sort_bytes = 0;
  (void)exclusive_sum(nullptr, scan_bytes, nullptr, nullptr, ni, 0);
  DevList all = {left.of(ni), right.of(ni), node_parent.of(ni), leaf_parent.of(n), arrivals.of(ni), root_of.of(ni), cnt.of(ni), off.of(ni),
                 cost.of(3 * ni), choice.of(ni), level.of(4), bases.of(kMaxLevels), scan_tmp.of(scan_bytes)};
  if (morton) {
    (void)rocprim::radix_sort_pairs(nullptr, sort_bytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (uint32_t*)nullptr,
                                    (uint32_t*)nullptr, n, 0, 64, 0);
    for (DevBytes* d : DevList{keys_in.of(n), keys_out.of(n), ids_in.of(n), sort_tmp.of(sort_bytes)}) all.push_back(d);
  }
  return all;
}

namespace {

// RENDER_SPEC 4.1b: leaf boxes are widened by 2^-19 of the scene's largest coordinate
float box_pad(const BvhBuffers& b) {
  float amax = 0.0f;
  for (int k = 0; k < 3; ++k) amax = std::max(amax, std::max(std::fabs(b.scene_min[k]), std::fabs(b.scene_max[k])));
  return amax * 1.9073486328125e-06f;
}

std::string flatten_and_bounds(BvhBuffers& b, BvhTopology& t, hipStream_t s) {
  const uint32_t n = b.tri_count;
  if (n) {
    hipLaunchKernelGGL(k_flatten, dim3(nblk(n)), dim3(256), 0, s, b.primitives, b.inst_first_tri, b.instance_count, n, b.tris_by_id, b.shade_tris,
                       t.tri_box, t.block_ord, b.gid_first, b.inst_index, b.object_space ? 1 : 0);
    bounds_reduce(t.block_ord, nblk(n), t.scene_ord, s);
  }
  uint32_t ord[6];
  HIP_TRY(hipMemcpyAsync(ord, t.scene_ord, sizeof(ord), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int k = 0; k < 3; ++k) {
    b.scene_min[k] = n ? ord2f(ord[k]) : 0.0f;
    b.scene_max[k] = n ? ord2f(ord[3 + k]) : 0.0f;
  }
  return "";
}

void leaf_boxes(BvhBuffers& b, BvhTopology& t, hipStream_t s) {
  const uint32_t n = b.tri_count;
  if (n) hipLaunchKernelGGL(k_leaf_boxes, dim3(nblk(n)), dim3(256), 0, s, t.tri_box, t.sorted_ids, n, t.leaf_box, b.tris_by_id, b.tris, box_pad(b), b.tris_any,
                            b.shade_tris, b.material_any_class, b.material_count, b.material_kind);
}

}  // namespace

void bounds_reduce(const uint32_t* block_ord, uint32_t blocks, uint32_t* scene_ord, hipStream_t s) {
  hipLaunchKernelGGL(k_bounds_reduce, dim3(1), dim3(256), 0, s, block_ord, blocks, scene_ord);
}

// Karras' LBVH, or the Morton order PLOC starts from
std::string morton_hierarchy(const HierarchyJob& job, BuildScratch& sc, const uint32_t* scene_ord, bool ploc, hipStream_t s) {
  const uint32_t n = job.n;
  hipLaunchKernelGGL(k_morton, dim3(nblk(n)), dim3(256), 0, s, job.tri_box, n, scene_ord, sc.keys_in, sc.ids_in);
  size_t tmp_bytes = sc.sort_tmp.bytes;
  HIP_TRY(rocprim::radix_sort_pairs(sc.sort_tmp.raw, tmp_bytes, sc.keys_in.get(), sc.keys_out.get(), sc.ids_in.get(), job.sorted_ids, n, 0, 64, s));
  if (ploc) return ploc_hierarchy(job, s);
  hipLaunchKernelGGL(k_hierarchy, dim3(nblk(n - 1)), dim3(256), 0, s, sc.keys_out, (int)n, job.tree);
  return "";
}

std::string fit_hierarchy(const BinaryTree& tree, const Box6* leaf_box, uint32_t* arrivals, uint32_t n, hipStream_t s) {
  HIP_TRY(hipMemsetAsync(arrivals, 0, (size_t)(n - 1) * 4, s));
  hipLaunchKernelGGL(k_fit, dim3(nblk(n)), dim3(256), 0, s, tree, leaf_box, arrivals, n);
  return "";
}

// Chooses the 4-wide topology from the fitted binary tree (keep, refs4, index4, level_base) and with it the node count, the depth and
// the stack a ray can need: the cost pass prices every cut, the level launches walk the cheapest one down from the root.  Levels are driven like PLOC's rounds: {first node, size, level} on the device, the host looks every few
// levels; between two looks the grid covers the largest size the level can have reached (a level is at most 4 times the one above, and < n).
std::string collapse(BvhBuffers& b, BvhTopology& t, BuildScratch& sc, const BinaryTree& tree, hipStream_t s) {
  const uint32_t ni = b.tri_count - 1;
  HIP_TRY(hipMemsetAsync(sc.arrivals, 0, (size_t)ni * 4, s));
  hipLaunchKernelGGL(k_collapse_cost, dim3(nblk(2u * b.tri_count - 1u)), dim3(256), 0, s, tree, t.leaf_box, sc.arrivals, b.tri_count, t.leaf_max, sc.cost, sc.choice,
                     t.keep);
  static const uint32_t zero = 0;
  HIP_TRY(hipMemcpyAsync(sc.root_of, &zero, 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(t.index4, &zero, 4, hipMemcpyHostToDevice, s));
  const uint32_t look_every = b.opt.collapse_look_every ? b.opt.collapse_look_every : 8u;
  const uint32_t init_level[3] = {0u, 1u, 0u};
  HIP_TRY(hipMemcpyAsync(sc.level, init_level, 12, hipMemcpyHostToDevice, s));
  uint32_t now[3] = {0u, 1u, 0u};
  while (now[1] > 0u) {
    unsigned long long bound = now[1];
    for (uint32_t k = 0; k < look_every; ++k) {
      const uint32_t bd = (uint32_t)std::min<unsigned long long>(bound, ni);
      hipLaunchKernelGGL(k_collapse_level, dim3(nblk(bd)), dim3(256), 0, s, sc.root_of, sc.level, bd, tree, t.keep, sc.choice, t.refs4, sc.cnt);
      size_t tb = sc.scan_tmp.bytes;
      HIP_TRY(exclusive_sum(sc.scan_tmp.raw, tb, sc.cnt.get(), sc.off.get(), bd, s));
      hipLaunchKernelGGL(k_scatter_level, dim3(nblk(bd)), dim3(256), 0, s, sc.root_of, sc.level, t.refs4, t.keep, sc.off, t.index4);
      hipLaunchKernelGGL(k_level_advance, dim3(1), dim3(64), 0, s, sc.cnt, sc.off, sc.level, sc.bases, kMaxLevels);
      bound *= 4ull;
    }
    HIP_TRY(hipMemcpyAsync(now, sc.level, 12, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (now[2] > kMaxLevels) return "bvh_build: the tree is deeper than " + std::to_string(kMaxLevels) + " 4-wide levels";
  }
  const uint32_t node_count = now[0], levels = now[2];
  t.level_base.assign(levels, 0u);
  HIP_TRY(hipMemcpy(t.level_base.data(), sc.bases, (size_t)levels * 4, hipMemcpyDeviceToHost));
  t.level_base.push_back(node_count);
  b.node_count = node_count;
  b.max_depth = levels;
  b.stack_need = 3u * levels;  // a 4-node visit defers at most three siblings
  return "";
}

// The only writer of the 64-B nodes, after a build and after a refit: levels are contiguous in BFS order, so one launch per level from
// the deepest up derives every node from its children's boxes (leaf boxes, or the union a child node left in box4[its index]).
std::string pack_levels(BvhBuffers& b, BvhTopology& t, hipStream_t s) {
  auto* emit = t.item_ref ? k_emit_single4<true> : k_emit_single4<false>;
  auto* level = t.item_ref ? k_refit_level<true> : k_refit_level<false>;
  if (t.single_node()) hipLaunchKernelGGL(emit, dim3(1), dim3(64), 0, s, t.leaf_box, t.n, b.nodes, t.sorted_ids, t.item_ref);
  else
    for (size_t l = t.level_base.size() - 1; l-- > 0;) {
      const uint32_t base = t.level_base[l], size = t.level_base[l + 1] - base;
      hipLaunchKernelGGL(level, dim3(nblk(size)), dim3(256), 0, s, t.refs4, base, size, t.first, t.last, t.keep, t.index4, t.leaf_box, t.box4, b.nodes,
                         t.sorted_ids, t.item_ref);
    }
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipGetLastError());
  return "";
}

hipError_t exclusive_sum(void* storage, size_t& bytes, const uint32_t* in, uint32_t* out, size_t n, hipStream_t s) {
  return rocprim::exclusive_scan(storage, bytes, in, out, 0u, n, rocprim::plus<uint32_t>(), s);
}

void bvh_free_topology(void* topo) { delete static_cast<BvhTopology*>(topo); }

// the buffers of a build, the caller's tree in the place of a builder's, then collapse() as every build calls it
std::string collapse_selftest(const CollapseSelftest& job) {
  const uint32_t n = job.n, ni = n - 1;
  hipStream_t s = nullptr;
  BvhTopology t;
  t.n = n; t.leaf_max = job.leaf_max;
  BuildScratch sc;
  std::string e = alloc_all(t.plan());
  if (e.empty()) e = alloc_all(sc.plan(n, false));
  if (!e.empty()) return e;
  HIP_TRY(hipMemcpyAsync(sc.left, job.left, (size_t)ni * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(sc.right, job.right, (size_t)ni * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(sc.node_parent, job.node_parent, (size_t)ni * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(sc.leaf_parent, job.leaf_parent, (size_t)n * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(t.first, job.first, (size_t)ni * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(t.last, job.last, (size_t)ni * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(t.box4, job.node_boxes, (size_t)ni * sizeof(Box6), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(t.leaf_box, job.leaf_boxes, (size_t)n * sizeof(Box6), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemsetAsync(t.refs4, 0xff, (size_t)ni * sizeof(uint4), s));
  BvhBuffers b{};
  b.tri_count = n;
  const BinaryTree tree{sc.left, sc.right, t.first, t.last, sc.node_parent, sc.leaf_parent, t.box4};
  if (!(e = collapse(b, t, sc, tree, s)).empty()) return e;
  HIP_TRY(hipGetLastError());
  if (job.costs) HIP_TRY(hipMemcpy(job.costs, sc.cost, (size_t)ni * 12, hipMemcpyDeviceToHost));
  if (job.choices) HIP_TRY(hipMemcpy(job.choices, sc.choice, (size_t)ni * 4, hipMemcpyDeviceToHost));
  if (job.keep) HIP_TRY(hipMemcpy(job.keep, t.keep, (size_t)ni * 4, hipMemcpyDeviceToHost));
  if (job.refs4) HIP_TRY(hipMemcpy(job.refs4, t.refs4, (size_t)ni * sizeof(uint4), hipMemcpyDeviceToHost));
  if (job.node_count) *job.node_count = b.node_count;
  if (job.levels) *job.levels = b.max_depth;
  return "";
}

namespace {

// what k_flatten leaves of the scene bounds, from boxes that are already there: every block its bounds, as ordered integers
__global__ void __launch_bounds__(256) k_box_bounds(const Box6* __restrict__ tri_box, uint32_t n, uint32_t* __restrict__ block_ord) {
  __shared__ uint32_t wave_ord[4][6];
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  uint32_t ord[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u};
  if (g < n) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { ord[k] = f2ord(tri_box[g].mn[k]); ord[3 + k] = f2ord(tri_box[g].mx[k]); }
  }
  block_bounds_fold(ord, wave_ord, threadIdx.x, block_ord, blockIdx.x * 6u);
}
// k_leaf_boxes without the triangles
__global__ void __launch_bounds__(256) k_widen_boxes(const Box6* __restrict__ tri_box, const uint32_t* __restrict__ sorted_ids, uint32_t n, float pad,
                                                      Box6* __restrict__ leaf_box) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) leaf_box[k] = widen(tri_box[sorted_ids[k]], pad);
}

}  // namespace

// the buffers of a build, the caller's boxes in the place of flatten's, then the builder as bvh_build calls it; the Karras hierarchy is
// fitted as there, so that node_box means the same for every builder
std::string hierarchy_selftest(const HierarchySelftest& job) {
  const uint32_t n = job.n, ni = n - 1;
  hipStream_t s = nullptr;
  const bool sah = job.builder == 1u, ploc = job.builder == 2u;
  BvhTopology t;
  t.n = n; t.leaf_max = 1;
  BuildScratch sc;
  std::string e = alloc_all(t.plan());
  if (e.empty()) e = alloc_all(sc.plan(n, !sah));
  if (!e.empty()) return e;
  HIP_TRY(hipMemcpyAsync(t.tri_box, job.boxes, (size_t)n * sizeof(Box6), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_box_bounds, dim3(nblk(n)), dim3(256), 0, s, t.tri_box, n, t.block_ord);
  bounds_reduce(t.block_ord, nblk(n), t.scene_ord, s);
  const BinaryTree tree{sc.left, sc.right, t.first, t.last, sc.node_parent, sc.leaf_parent, t.box4};
  BuildOptions opt;
  opt.builder = job.builder; opt.ploc_tail = job.ploc_tail; opt.ploc_look_every = job.ploc_look_every;
  const HierarchyJob hj{n, job.pad, opt, t.tri_box, t.sorted_ids, tree};
  if (!(e = sah ? sah_hierarchy(hj, s) : morton_hierarchy(hj, sc, t.scene_ord, ploc, s)).empty()) return e;
  if (!sah && !ploc) {
    hipLaunchKernelGGL(k_widen_boxes, dim3(nblk(n)), dim3(256), 0, s, t.tri_box, t.sorted_ids, n, job.pad, t.leaf_box);
    if (!(e = fit_hierarchy(tree, t.leaf_box, sc.arrivals, n, s)).empty()) return e;
  }
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(job.sorted_ids, t.sorted_ids, (size_t)n * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(job.left, sc.left, (size_t)ni * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(job.right, sc.right, (size_t)ni * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(job.first, t.first, (size_t)ni * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(job.last, t.last, (size_t)ni * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(job.node_parent, sc.node_parent, (size_t)ni * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(job.leaf_parent, sc.leaf_parent, (size_t)n * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(job.node_boxes, t.box4, (size_t)ni * sizeof(Box6), hipMemcpyDeviceToHost));
  return "";
}

std::string bvh_build(BvhBuffers& b, uint32_t leaf_max, hipStream_t s) {
  const uint32_t n = b.tri_count;
  if (b.topology) { bvh_free_topology(b.topology); b.topology = nullptr; }
  BvhTopology* tp = new BvhTopology();
  b.topology = tp;
  BvhTopology& t = *tp;
  t.n = n; t.leaf_max = leaf_max;
  // hierarchy over the triangles: full-sweep SAH rounds for scenes large enough to repay them (1 M triangles: 34 ms of build instead
  // of PLOC's 11 ms for 10-15 % fewer node visits per closest-hit ray, profiles/r02_experiments.txt), Karras' LBVH over the Morton
  // order otherwise; PLOC (nearest-neighbour clustering along the Morton order) stays selectable as the fast large-scene build
  const bool sah = n >= 2 && (b.opt.builder ? b.opt.builder == 1u : n >= 4096u);
  const bool ploc = n >= 2 && !sah && b.opt.builder == 2u;
  // one allocation for everything the topology keeps and one for the build's temporaries (sort keys, the binary tree, the builder's
  // rounds), each as large as the buffers it will hold, instead of ~60 hipMalloc / hipFree pairs
  const DevList kept = t.plan();
  std::string e = t.arena.open(arena_bytes(kept));
  if (e.empty()) e = alloc_all(kept);
  t.arena.close();
  if (!e.empty()) return e;
  Arena scratch;  // declared before the temporaries below: released after them
  BuildScratch sc;
  const DevList temporaries = sc.plan(n, n >= 2 && !sah);
  if (!(e = scratch.open(arena_bytes(temporaries) + (sah ? sah_scratch_bytes(n) : 0) + (ploc ? ploc_scratch_bytes(n) : 0))).empty()) return e;
  if (!(e = alloc_all(temporaries)).empty()) return e;
  if (leaf_max > 8u || n >= (1u << 28)) return "bvh_build: the 4-wide node format holds leaves of <= 8 triangles and < 2^28 triangles";
  if (!(e = flatten_and_bounds(b, t, s)).empty()) return e;
  const BinaryTree tree{sc.left, sc.right, t.first, t.last, sc.node_parent, sc.leaf_parent, t.box4};
  if (n >= 2) {
    const HierarchyJob job{n, box_pad(b), b.opt, t.tri_box, t.sorted_ids, tree};
    if (!(e = sah ? sah_hierarchy(job, s) : morton_hierarchy(job, sc, t.scene_ord, ploc, s)).empty()) return e;
  } else if (n == 1) {
    static const uint32_t zero = 0;
    HIP_TRY(hipMemcpyAsync(t.sorted_ids, &zero, 4, hipMemcpyHostToDevice, s));
  }
  leaf_boxes(b, t, s);
  if (t.single_node()) {  // one 4-node with a single leaf child
    b.node_count = 1;
    b.max_depth = 1;
    b.stack_need = 1;
  } else {
    if (!sah && !ploc) {  // the Karras hierarchy has no boxes yet
      if (!(e = fit_hierarchy(tree, t.leaf_box, sc.arrivals, n, s)).empty()) return e;
    }
    if (!(e = collapse(b, t, sc, tree, s)).empty()) return e;
  }
  return pack_levels(b, t, s);
}

__global__ void __launch_bounds__(256) k_relocate(BvhNode4* __restrict__ nodes, uint32_t count, uint32_t node_offset, uint32_t tri_offset) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count * 4u) return;
  uint32_t& ref = nodes[i >> 2].ref[i & 3u];
  if (ref == kAbsent) return;
  ref += (ref & kLeafRef) ? tri_offset : node_offset;  // a leaf's first triangle sits in the low 28 bits: the sum stays below 2^28 (checked by the caller)
}
std::string bvh_relocate(BvhBuffers& b, uint32_t node_offset, uint32_t tri_offset, hipStream_t s) {
  if (node_offset == 0u && tri_offset == 0u) return "";
  if ((unsigned long long)tri_offset + b.tri_count >= (1ull << 28)) return "bvh_relocate: the scene holds 2^28 triangles or more";
  hipLaunchKernelGGL(k_relocate, dim3(nblk(b.node_count * 4u)), dim3(256), 0, s, b.nodes, b.node_count, node_offset, tri_offset);
  HIP_TRY(hipGetLastError());
  return "";
}

// node_count / max_depth / stack_need stand as the build left them: the topology is frozen
std::string bvh_refit(BvhBuffers& b, hipStream_t s) {
  if (!b.topology) return "bvh_refit: no BVH has been built";
  BvhTopology& t = *static_cast<BvhTopology*>(b.topology);
  if (t.n != b.tri_count) return "bvh_refit: triangle count changed, rebuild required";
  std::string e = flatten_and_bounds(b, t, s);
  if (!e.empty()) return e;
  leaf_boxes(b, t, s);
  return pack_levels(b, t, s);
}

}  // namespace rt
