// bvh_instances.hip — the instance levels of a two-level tree (RENDER_SPEC 4.5) built on the GPU: hala_rt_build_options::instance_levels = 1,
// the device counterpart of bvh_tlas.cpp.  One item per instanced instance, plus one for the world-space tree over the flattened
// instances; every build, at commit and at every refit and shutter step, is
//   items      k_instance_items: world -> object of every instanced instance (the InstRef the traversal reads), its world box, its child
//              reference; the scene bounds of 4.5 folded per block, then by one block (bounds_reduce) — no float atomics
//   hierarchy  a binary tree over the item boxes through HierarchyJob (bvh_build_impl.h), the boxes in the place of the triangle boxes with
//              pad = 0: they are padded already.  The builder is hala_rt_build_options::builder as for triangles (automatic: LBVH below
//              4096 items, full-sweep SAH from there)
//   collapse, pack levels   bvh_build.hip's, leaf_max = 1; a leaf's reference is the item's (BvhTopology::item_ref)
// Everything a build carves comes out of one arena that the renderer keeps between builds (InstanceLevelsJob::arena), so a refit
// allocates nothing.  The arithmetic of the items is the host path's (rt_trees.hip: world_to_object, build_instance_levels), operation
// for operation: the InstRef records and the scene bounds are the same bits whichever path built them; the tree above them is not.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bvh_build_impl.h"

namespace rt {

namespace {

// the tables of one build, in the order they are carved
struct ItemTables {
  Dev<uint32_t> item_ref;  // [n] the child reference a node slot gets for the item
  DevList plan(uint32_t n) { return {item_ref.of(n)}; }
};

// std::min(a, b) / std::max(a, b) of the host path, select for select (they differ from fminf / fmaxf in which zero they keep)
RT_DI float std_min(float a, float b) { return b < a ? b : a; }
RT_DI float std_max(float a, float b) { return a < b ? b : a; }

// One thread per item.  Item 0 is the world tree's when `world_item` is set; item j > that is the instanced instance items[j].inst,
// whose InstRef is number j - world_item.
__global__ void __launch_bounds__(256) k_instance_items(const InstItem* __restrict__ items, uint32_t n, uint32_t world_item,
                                                         const InstTree* __restrict__ trees, const hala_gpu_mesh_data* __restrict__ instances,
                                                         const uint32_t* __restrict__ inst_first_tri, InstRef* __restrict__ inst_refs,
                                                         Box6* __restrict__ item_box, uint32_t* __restrict__ item_ref,
                                                         uint32_t* __restrict__ block_ord /* [gridDim.x][6] */) {
  __shared__ uint32_t wave_ord[4][6];
  const uint32_t tid = threadIdx.x, j = blockIdx.x * 256u + tid;
  uint32_t ord[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u};
  if (j < n) {
    const InstItem it = items[j];
    const InstTree tr = trees[it.tree];
    Box6 box;
    float wmn[3], wmx[3];
    if (it.inst == kAbsent) {  // the world tree: its root as an ordinary inner child, no transform; its exact bounds count for the scene's
      float amax = 0.0f;
#pragma unroll
      for (int k = 0; k < 3; ++k) { wmn[k] = tr.mn[k]; wmx[k] = tr.mx[k]; amax = std_max(amax, std_max(fabsf(tr.mn[k]), fabsf(tr.mx[k]))); }
      const float pad = amax * 1.9073486328125e-06f * 2.0f;
#pragma unroll
      for (int k = 0; k < 3; ++k) { box.mn[k] = wmn[k] - pad; box.mx[k] = wmx[k] + pad; }
      item_ref[j] = tr.node_off;
    } else {
      const float* m = instances[it.inst].transform;
      // world -> object: rows of the inverse of the upper 3x3 (cross products of its columns over the determinant) and the translation
      const f3 c0 = mk3(m[0], m[1], m[2]), c1 = mk3(m[4], m[5], m[6]), c2 = mk3(m[8], m[9], m[10]);
      const f3 k0 = cross3(c1, c2), k1 = cross3(c2, c0), k2 = cross3(c0, c1);
      const float inv = 1.0f / dot3(c0, k0);  // IEEE division, correctly rounded under the library's flags, like the host's
      InstRef ref;
      ref.r0[0] = k0.x * inv; ref.r0[1] = k0.y * inv; ref.r0[2] = k0.z * inv;
      ref.r1[0] = k1.x * inv; ref.r1[1] = k1.y * inv; ref.r1[2] = k1.z * inv;
      ref.r2[0] = k2.x * inv; ref.r2[1] = k2.y * inv; ref.r2[2] = k2.z * inv;
      ref.tr[0] = m[12]; ref.tr[1] = m[13]; ref.tr[2] = m[14];
      ref.root = tr.node_off; ref.gid_base = inst_first_tri[it.inst]; ref.shade_base = tr.tri_off; ref.inst = it.inst;
      {  // one 64-B record, four 16-B stores
        const float4* src = reinterpret_cast<const float4*>(&ref);
        float4* dst = reinterpret_cast<float4*>(inst_refs + (j - world_item));
#pragma unroll
        for (int k = 0; k < 4; ++k) dst[k] = src[k];
      }
      // world box: the eight corners of the primitive's exact object-space bounds, moved to world space (RENDER_SPEC 3)
#pragma unroll
      for (int k = 0; k < 3; ++k) { wmn[k] = INFINITY; wmx[k] = -INFINITY; }
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const float p[3] = {(c & 1) ? tr.mx[0] : tr.mn[0], (c & 2) ? tr.mx[1] : tr.mn[1], (c & 4) ? tr.mx[2] : tr.mn[2]};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float q = __fmaf_rn(m[8 + k], p[2], __fmaf_rn(m[4 + k], p[1], m[k] * p[0])) + m[12 + k];
          wmn[k] = std_min(wmn[k], q); wmx[k] = std_max(wmx[k], q);
        }
      }
      // padded like every box (4.1b), twice: for the rounding of the move to world space and for the object-space pad of the leaves below
      float amax = 0.0f;
#pragma unroll
      for (int k = 0; k < 3; ++k) amax = std_max(amax, std_max(fabsf(wmn[k]), fabsf(wmx[k])));
      const float ext = std_max(std_max(wmx[0] - wmn[0], wmx[1] - wmn[1]), wmx[2] - wmn[2]);
      const float pad = (amax + ext) * 1.9073486328125e-06f * 2.0f;
#pragma unroll
      for (int k = 0; k < 3; ++k) { box.mn[k] = wmn[k] - pad; box.mx[k] = wmx[k] + pad; }
      item_ref[j] = kInstLeafTag | (j - world_item);
    }
    item_box[j] = box;
#pragma unroll
    for (int k = 0; k < 3; ++k) { ord[k] = f2ord(wmn[k]); ord[3 + k] = f2ord(wmx[k]); }
  }
  block_bounds_fold(ord, wave_ord, tid, block_ord, blockIdx.x * 6u);
}

// the boxes in sorted order: what the level pack reads (the item boxes are padded already, nothing is widened)
__global__ void __launch_bounds__(256) k_item_leaf_boxes(const Box6* __restrict__ item_box, const uint32_t* __restrict__ sorted_ids, uint32_t n,
                                                          Box6* __restrict__ leaf_box) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) leaf_box[k] = item_box[sorted_ids[k]];
}

struct Builder { bool sah, ploc; };
Builder builder_for(uint32_t n, const BuildOptions& opt) {  // bvh_build's rule, items in the place of triangles
  Builder b;
  b.sah = n >= 2 && (opt.builder ? opt.builder == 1u : n >= 4096u);
  b.ploc = n >= 2 && !b.sah && opt.builder == 2u;
  return b;
}

}  // namespace

size_t instance_levels_arena_bytes(uint32_t n, const BuildOptions& opt) {
  const Builder how = builder_for(n, opt);
  BvhTopology t;
  t.n = n; t.leaf_max = 1;
  BuildScratch sc;
  ItemTables it;
  return arena_bytes(t.plan()) + arena_bytes(sc.plan(n, n >= 2 && !how.sah)) + arena_bytes(it.plan(n)) + (how.sah ? sah_scratch_bytes(n) : 0) +
         (how.ploc ? ploc_scratch_bytes(n) : 0);
}

std::string instance_levels_build(InstanceLevelsJob& job, hipStream_t s) {
  const uint32_t n = job.n;
  if (n == 0) return "instance levels: no items";
  if (n - job.world_item >= 0x0ffffff0u) return "Too many instances.";
  const Builder how = builder_for(n, job.opt);
  Arena arena;  // declared before what is carved from it: released after
  arena.adopt(job.arena, job.arena_bytes);
  BvhTopology t;
  t.n = n; t.leaf_max = 1;
  BuildScratch sc;
  ItemTables it;
  std::string e = alloc_all(t.plan());
  if (e.empty()) e = alloc_all(sc.plan(n, n >= 2 && !how.sah));
  if (e.empty()) e = alloc_all(it.plan(n));
  if (!e.empty()) return e;
  t.item_ref = it.item_ref;
  hipLaunchKernelGGL(k_instance_items, dim3(nblk(n)), dim3(256), 0, s, job.items, n, job.world_item, job.trees, job.instances, job.inst_first_tri,
                     job.inst_refs, t.tri_box, it.item_ref, t.block_ord);
  bounds_reduce(t.block_ord, nblk(n), t.scene_ord, s);
  // the six floats come back with the first look the host takes anyway (a builder's, the collapse's, or the level pack's at the end)
  uint32_t ord[6];
  HIP_TRY(hipMemcpyAsync(ord, t.scene_ord, sizeof(ord), hipMemcpyDeviceToHost, s));
  BvhBuffers b{};
  b.tri_count = n; b.opt = job.opt; b.nodes = job.nodes;
  const BinaryTree tree{sc.left, sc.right, t.first, t.last, sc.node_parent, sc.leaf_parent, t.box4};
  if (n >= 2) {
    const HierarchyJob hj{n, 0.0f, job.opt, t.tri_box, t.sorted_ids, tree};
    if (!(e = how.sah ? sah_hierarchy(hj, s) : morton_hierarchy(hj, sc, t.scene_ord, how.ploc, s)).empty()) return e;
  } else {
    static const uint32_t zero = 0;
    HIP_TRY(hipMemcpyAsync(t.sorted_ids, &zero, 4, hipMemcpyHostToDevice, s));
  }
  hipLaunchKernelGGL(k_item_leaf_boxes, dim3(nblk(n)), dim3(256), 0, s, t.tri_box, t.sorted_ids, n, t.leaf_box);
  if (t.single_node()) {
    b.node_count = 1; b.max_depth = 1;
  } else {
    if (!how.sah && !how.ploc && !(e = fit_hierarchy(tree, t.leaf_box, sc.arrivals, n, s)).empty()) return e;  // the Karras hierarchy has no boxes yet
    if (!(e = collapse(b, t, sc, tree, s)).empty()) return e;
  }
  if (b.node_count > job.node_capacity) return "internal: instance levels larger than reserved";
  if (!(e = pack_levels(b, t, s)).empty()) return e;  // synchronises: `ord` has arrived
  job.node_count = b.node_count;
  job.levels = b.max_depth;
  for (int k = 0; k < 3; ++k) { job.scene_min[k] = ord2f(ord[k]); job.scene_max[k] = ord2f(ord[3 + k]); }
  return "";
}

}  // namespace rt
