// rt_trees.hip — the trees of the committed scene (hala_rt_renderer::trees) and what stands in front of them: building and refitting a
// tree (tree_publish, tree_fit), the instance levels of a two-level scene (RENDER_SPEC 4.5), the traversal configuration, tree quality
// and the refit policy (RENDER_SPEC 4.6), the one refit sequence (refit_trees), the build options and the introspection of the trees.
#include "renderer_state.h"

namespace rt {

using Tree = hala_rt_renderer::Tree;

static int fetch_instance_refs(hala_rt_renderer* r);
static int configure_traversal(hala_rt_renderer* r) {
  const size_t nb = (size_t)r->bvh.node_count * 64, tb = (size_t)r->bvh.tri_count * 48;
  // Whole BVH in LDS when it fits the budget (the STAGED kernel variants read it with ds_read only); otherwise nothing
  // is staged: a top-of-tree slice measured no gain (profiles/r01_h_experiments.txt), the caches already hold it.
  r->staged = !r->two_level && nb + tb <= kLdsStageBudget;  // (the LDS-staged kernel variants know no instances)
  r->lds_nodes = r->staged ? r->bvh.node_count : 0u;
  r->lds_tris = r->staged ? r->bvh.tri_count : 0u;
  const TreeForm tree = tree_form(r->view());
  if (r->leaf_max_built > traverse_max_leaf(tree)) RT_FAIL("The BVH was built with larger leaves than the traversal variant for its size accepts.");
  const size_t smem = (size_t)r->lds_nodes * 64 + (size_t)r->lds_tris * 48 + traverse_fixed_lds_bytes(tree);
  const uint32_t per_cu = traverse_blocks_per_cu(smem, tree);
  if (per_cu == 0) RT_FAIL("The traversal kernel does not fit on a compute unit with the requested LDS staging.");
  r->lcfg.persistent_blocks = r->cu_count * std::min(per_cu, 8u);
  r->lcfg.smem = smem;
  r->lcfg.spill = nullptr;
  // measured (profiles/r01_c_refill_sweep.txt): whole-wave refills are best when the BVH lives in LDS (uniform, cheap rays);
  // refilling once half the wave is idle is best when node fetches go to L2 / Infinity Cache
  r->lcfg.refill = r->staged ? 64u : kRefillThreshold;
  if (r->two_level || r->bvh.stack_need > traverse_stack_lds_levels(tree)) {
    // (instance levels built on the GPU bring a conservative need and keep their InstRef table on the device: the exact sweep, a download
    // of all nodes, only runs for them when that need would refuse the tree)
    const bool over = r->bvh.stack_need > traverse_stack_lds_levels(tree) + traverse_stack_spill_levels();
    if (over && r->two_level && fetch_instance_refs(r) != HALA_OK) return HALA_ERR;
    if ((r->two_level && r->levels.mode == 0u) || over) {
      // 3 x levels is a loose bound (every node on the path deferring three siblings).  Before refusing the tree, take the exact
      // one: need(node) = (inner children - 1) + max need(inner child) — the worst order visits the child with the deepest
      // need first while all its siblings wait.  Nodes are in breadth-first order (children behind their parent): one reverse sweep.
      std::vector<BvhNode4> nodes(r->bvh.node_count);
      RT_HIP(hipMemcpy(nodes.data(), r->d_nodes.ptr, nodes.size() * sizeof(BvhNode4), hipMemcpyDeviceToHost));
      std::vector<uint32_t> need(nodes.size(), 0u);
      for (size_t i = nodes.size(); i-- > 0;) {
        uint32_t inner = 0, deepest = 0;
        for (uint32_t ref : nodes[i].ref) {
          if (ref == kAbsent) continue;
          if (is_inst_leaf(ref)) {  // RENDER_SPEC 4.5: the world-space ray (3 entries) and the exit mark wait below the instance's own entries
            const uint32_t k = ref & 0x0fffffffu;
            ++inner;
            if (k < r->inst_refs.size() && r->inst_refs[k].root < need.size()) deepest = std::max(deepest, 4u + need[r->inst_refs[k].root]);
            continue;
          }
          if (ref & kLeafRef) continue;
          ++inner;
          if (ref < need.size()) deepest = std::max(deepest, need[ref]);
        }
        need[i] = inner ? inner - 1u + deepest : 0u;
      }
      r->bvh.stack_need = need.empty() ? 1u : std::max(1u, need[0]);
    }
    if (r->bvh.stack_need > traverse_stack_lds_levels(tree) + traverse_stack_spill_levels())
      RT_FAIL("The BVH is deeper than the traversal stack supports (" + std::to_string(r->bvh.max_depth) + " levels, " + std::to_string(r->bvh.stack_need) + " stack entries).");
    for (FrameSlot& s : r->slots.slot)  // one area per frame slot: the slots' launches run beside each other
      RT_HIP(s.spill.resize((size_t)r->lcfg.persistent_blocks * 256 * traverse_stack_spill_levels()));
    r->lcfg.spill = r->slots.slot[0].spill.ptr;
  }
  const float ex = r->bvh.scene_max[0] - r->bvh.scene_min[0], ey = r->bvh.scene_max[1] - r->bvh.scene_min[1], ez = r->bvh.scene_max[2] - r->bvh.scene_min[2];
  r->ray_eps = std::sqrt(std::fmaf(ez, ez, std::fmaf(ey, ey, ex * ex))) * 1e-5f;  // RENDER_SPEC §3
  return HALA_OK;
}

// RENDER_SPEC 7.1d: scenes with opacity-0 materials get a second copy of the BVH-order triangles for the any-hit launches (the trees
// learn of it, and of the material tables, when they are next published: tree_publish)
int attach_any_triangles(hala_rt_renderer* r) {
  const HostScene& hs = r->hs;
  std::vector<uint8_t> cls(hs.gpu_materials.size());
  r->any_invisible = false; r->any_translucent = false;
  for (size_t i = 0; i < cls.size(); ++i) {
    const hala_gpu_material& m = hs.gpu_materials[i];
    const bool cutout = m.base_color_map_index < hs.texture_image.size() && hs.images[hs.texture_image[m.base_color_map_index]].has_alpha;
    cls[i] = any_class_of(m, cutout);
    r->any_invisible = r->any_invisible || cls[i] != 0;
    r->any_translucent = r->any_translucent || cls[i] >= 2;
  }
  r->material_any_class = cls;
  RT_HIP(r->d_material_any_class.upload(cls.data(), cls.size(), r->stream));
  if (r->any_invisible) RT_HIP(r->d_tris_any.resize(r->stored_tris));
  return HALA_OK;
}

// ---- two-level trees (RENDER_SPEC 4.5) ---------------------------------------------------------------------------------------------
// instance levels built on the GPU write the InstRef table on the device: the host copy follows when somebody asks for it
static int fetch_instance_refs(hala_rt_renderer* r) {
  if (r->levels.refs_on_host) return HALA_OK;
  RT_HIP(hipStreamSynchronize(r->stream));
  if (!r->inst_refs.empty()) RT_HIP(hipMemcpy(r->inst_refs.data(), r->d_inst_refs.ptr, r->inst_refs.size() * sizeof(InstRef), hipMemcpyDeviceToHost));
  r->levels.refs_on_host = true;
  return HALA_OK;
}
// world -> object of one instance: rows of the inverse of the upper 3x3 (cross products of its columns over the determinant) and the
// translation; false: not invertible in float (the instance is flattened to world space like a primitive that is referenced once)
static float h_dot3(const float* a, const float* b) { return std::fmaf(a[2], b[2], std::fmaf(a[1], b[1], a[0] * b[0])); }
static void h_cross3(const float* a, const float* b, float* o) {
  o[0] = std::fmaf(a[1], b[2], -(a[2] * b[1])); o[1] = std::fmaf(a[2], b[0], -(a[0] * b[2])); o[2] = std::fmaf(a[0], b[1], -(a[1] * b[0]));
}
static bool world_to_object(const float* m, InstRef* o) {
  const float c0[3] = {m[0], m[1], m[2]}, c1[3] = {m[4], m[5], m[6]}, c2[3] = {m[8], m[9], m[10]};
  float k0[3], k1[3], k2[3];
  h_cross3(c1, c2, k0); h_cross3(c2, c0, k1); h_cross3(c0, c1, k2);
  const float det = h_dot3(c0, k0);
  if (!(det != 0.0f) || !std::isfinite(det)) return false;
  const float inv = 1.0f / det;
  for (int k = 0; k < 3; ++k) { o->r0[k] = k0[k] * inv; o->r1[k] = k1[k] * inv; o->r2[k] = k2[k] * inv; o->tr[k] = m[12 + k]; }
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(o->r0[k]) || !std::isfinite(o->r1[k]) || !std::isfinite(o->r2[k]) || !std::isfinite(o->tr[k])) return false;
  return true;
}
static void h_transform_point(const float* m, const float* p, float* o) {  // RENDER_SPEC 3
  for (int k = 0; k < 3; ++k) o[k] = std::fmaf(m[8 + k], p[2], std::fmaf(m[4 + k], p[1], m[k] * p[0])) + m[12 + k];
}
// which instances are intersected in object space: those of a primitive that several instances reference, if their transform can be inverted
// (the first half of it: which instances the rule considers at all; hala_rt_refit_nodes runs the second half on the device)
void instancing_candidates(const hala_rt_renderer* r, std::vector<uint8_t>* considered) {
  const HostScene& hs = r->hs;
  considered->assign(hs.instances.size(), 0);
  // automatic: the flattened tree is the faster one (no moves into object space, no instance levels to walk) while it fits comfortably
  constexpr uint32_t kFlattenLimit = 1u << 26;  // triangles: ~15 GB of nodes, triangles and shading records
  if (r->instancing_mode == 1u || (r->instancing_mode == 0u && hs.triangle_count <= kFlattenLimit)) return;
  std::vector<uint32_t> refs(hs.prims.size(), 0u);
  for (uint32_t p : hs.instance_prim) refs[p]++;
  for (size_t i = 0; i < hs.instances.size(); ++i)
    (*considered)[i] = refs[hs.instance_prim[i]] >= 2u && hs.prims[hs.instance_prim[i]].indices.size() >= 3 ? 1 : 0;
}
void classify_instances(hala_rt_renderer* r, std::vector<uint8_t>* flags) {
  const HostScene& hs = r->hs;
  instancing_candidates(r, flags);
  for (size_t i = 0; i < hs.instances.size(); ++i) {
    InstRef tmp;
    (*flags)[i] = (*flags)[i] && world_to_object(hs.instances[i].transform, &tmp) ? 1 : 0;
  }
}

// The instance levels on the GPU (hala_rt_build_options::instance_levels = 1; bvh_instances.hip).  fresh: a commit — the tables a pose does
// not change (InstInfo, the items' instance and tree) are made and uploaded and the arena is sized; a refit reuses them and allocates
// nothing.  Per build the host writes the small table of the trees, and only if a tree below was built or refitted since, then launches.
// (No test for a transform that stopped being invertible here: classify_instances has just made it, on the same transforms, for every
// instance this build treats as instanced.)
static int build_instance_levels_gpu(hala_rt_renderer* r, bool fresh) {
  const HostScene& hs = r->hs;
  InstanceLevels& lv = r->levels;
  const Tree* w = r->world_tree();
  const bool world = w && w->b.tri_count;
  std::vector<InstTree> trees(r->trees.size());
  uint32_t deepest = 0, largest_need = 0;
  for (size_t t = 0; t < r->trees.size(); ++t) {
    const Tree& bl = *r->trees[t];
    InstTree& tr = trees[t];
    tr.node_off = bl.node_off; tr.tri_off = bl.tri_off; tr.need = bl.b.stack_need; tr.depth = bl.b.max_depth;
    memcpy(tr.mn, bl.b.scene_min, 12); memcpy(tr.mx, bl.b.scene_max, 12);
    if (!bl.object_space && !world) continue;  // a world tree without triangles has no item
    deepest = std::max(deepest, bl.b.max_depth);
    // an instance: the world-space ray (3 entries) and the exit mark wait below its own entries
    largest_need = std::max(largest_need, bl.object_space ? 4u + bl.b.stack_need : bl.b.stack_need);
  }
  if (fresh) {
    std::vector<InstItem> items;
    std::vector<InstInfo> info(hs.instances.size());
    std::vector<uint32_t> flat_base(hs.instances.size(), 0u);
    if (w) {
      uint32_t at = w->tri_off;
      for (uint32_t i : w->insts) { flat_base[i] = at; at += hs.inst_first_tri[i + 1] - hs.inst_first_tri[i]; }
    }
    if (world) items.push_back(InstItem{kAbsent, 0u});
    for (size_t i = 0; i < hs.instances.size(); ++i) {
      info[i].first_tri = hs.inst_first_tri[i];
      info[i].instanced = r->inst_instanced[i];
      info[i].pad = 0;
      if (!r->inst_instanced[i]) { info[i].shade_base = flat_base[i]; continue; }
      const uint32_t t = (uint32_t)r->prim_tree[hs.instance_prim[i]];
      info[i].shade_base = r->trees[t]->tri_off;
      items.push_back(InstItem{(uint32_t)i, t});
    }
    if (items.empty() || items.size() > r->tlas_capacity) RT_FAIL("internal: instance levels larger than reserved");
    lv.items = (uint32_t)items.size(); lv.world_item = world ? 1u : 0u;
    if (lv.items - lv.world_item >= 0x0ffffff0u) RT_FAIL("Too many instances.");
    lv.opt = r->bvh.opt;
    r->inst_refs.assign(lv.items - lv.world_item, InstRef{});
    RT_HIP(r->d_inst_refs.resize(r->inst_refs.size()));
    RT_HIP(lv.arena.resize(instance_levels_arena_bytes(lv.items, lv.opt)));
    RT_HIP(lv.d_items.upload(items.data(), items.size(), r->stream));
    RT_HIP(r->d_inst_info.upload(info.data(), info.size(), r->stream));
    RT_HIP(hipStreamSynchronize(r->stream));  // `items`, `info` go out of scope
  }
  if (fresh || trees.size() != lv.trees.size() || memcmp(trees.data(), lv.trees.data(), trees.size() * sizeof(InstTree)) != 0) {
    lv.trees = trees;  // (the copy the upload reads outlives it)
    RT_HIP(lv.d_trees.upload(lv.trees.data(), lv.trees.size(), r->stream));
  }
  InstanceLevelsJob job{};
  job.n = lv.items; job.world_item = lv.world_item;
  job.items = lv.d_items.ptr; job.trees = lv.d_trees.ptr; job.instances = r->d_instances.ptr; job.inst_first_tri = r->d_inst_first_tri.ptr;
  job.inst_refs = r->d_inst_refs.ptr; job.nodes = r->d_nodes.ptr; job.node_capacity = r->tlas_capacity;
  job.arena = lv.arena.ptr; job.arena_bytes = lv.arena.bytes(); job.opt = lv.opt;
  const std::string e = instance_levels_build(job, r->stream);
  if (!e.empty()) RT_FAIL(e);
  lv.refs_on_host = false;
  r->tlas_nodes = job.node_count;
  r->bvh.max_depth = job.levels + deepest;
  r->bvh.stack_need = 3u * job.levels + largest_need;  // a 4-node visit defers at most three siblings; an item brings its own need
  memcpy(r->bvh.scene_min, job.scene_min, 12); memcpy(r->bvh.scene_max, job.scene_max, 12);
  return HALA_OK;
}

// the instance levels: InstRef per instanced instance, one item per instanced instance + one for the world tree, the host build, the upload;
// also the scene bounds (RENDER_SPEC 4.5: world tree's exact bounds + the boxes of the transformed corners of the instanced primitives' bounds)
static int build_instance_levels(hala_rt_renderer* r, bool fresh) {
  if (r->levels.mode == 1u) return build_instance_levels_gpu(r, fresh);
  const HostScene& hs = r->hs;
  std::vector<TlasItem> items;
  r->inst_refs.clear();
  std::vector<InstInfo> info(hs.instances.size());
  float smin[3] = {INFINITY, INFINITY, INFINITY}, smax[3] = {-INFINITY, -INFINITY, -INFINITY};
  uint32_t deepest = 0;
  // shading records: the world tree's triangles in its own order (instance order), then every instanced primitive's
  std::vector<uint32_t> flat_base(hs.instances.size(), 0u);
  if (const Tree* wt = r->world_tree()) {
    const Tree& w = *wt;
    uint32_t at = w.tri_off;
    for (uint32_t i : w.insts) { flat_base[i] = at; at += hs.inst_first_tri[i + 1] - hs.inst_first_tri[i]; }
    if (w.b.tri_count) {
      TlasItem it{};
      const float pad = std::max({std::fabs(w.b.scene_min[0]), std::fabs(w.b.scene_min[1]), std::fabs(w.b.scene_min[2]), std::fabs(w.b.scene_max[0]),
                                  std::fabs(w.b.scene_max[1]), std::fabs(w.b.scene_max[2])}) * 1.9073486328125e-06f * 2.0f;
      for (int k = 0; k < 3; ++k) { it.mn[k] = w.b.scene_min[k] - pad; it.mx[k] = w.b.scene_max[k] + pad; smin[k] = std::min(smin[k], w.b.scene_min[k]); smax[k] = std::max(smax[k], w.b.scene_max[k]); }
      it.ref = w.node_off;  // its root: an inner child, no transform
      it.need = w.b.stack_need;
      deepest = std::max(deepest, w.b.max_depth);
      items.push_back(it);
    }
  }
  for (size_t i = 0; i < hs.instances.size(); ++i) {
    info[i].first_tri = hs.inst_first_tri[i];
    info[i].instanced = r->inst_instanced[i];
    info[i].pad = 0;
    if (!r->inst_instanced[i]) { info[i].shade_base = flat_base[i]; continue; }
    const Tree& bl = *r->trees[(size_t)r->prim_tree[hs.instance_prim[i]]];
    info[i].shade_base = bl.tri_off;
    InstRef ref{};
    if (!world_to_object(hs.instances[i].transform, &ref)) RT_FAIL("An instanced node's transform stopped being invertible: commit() again.");
    ref.root = bl.node_off; ref.gid_base = hs.inst_first_tri[i]; ref.shade_base = bl.tri_off; ref.inst = (uint32_t)i;
    // world box of the instance: the eight corners of its primitive's exact object-space bounds, moved to world space
    TlasItem it{};
    float wmn[3] = {INFINITY, INFINITY, INFINITY}, wmx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int c = 0; c < 8; ++c) {
      const float p[3] = {(c & 1) ? bl.b.scene_max[0] : bl.b.scene_min[0], (c & 2) ? bl.b.scene_max[1] : bl.b.scene_min[1], (c & 4) ? bl.b.scene_max[2] : bl.b.scene_min[2]};
      float q[3];
      h_transform_point(hs.instances[i].transform, p, q);
      for (int k = 0; k < 3; ++k) { wmn[k] = std::min(wmn[k], q[k]); wmx[k] = std::max(wmx[k], q[k]); }
    }
    // padded like every box (RENDER_SPEC 4.1b), twice: once for the rounding of the move to world space, once for the object-space pad of the leaves below
    const float amax = std::max({std::fabs(wmn[0]), std::fabs(wmn[1]), std::fabs(wmn[2]), std::fabs(wmx[0]), std::fabs(wmx[1]), std::fabs(wmx[2])});
    const float ext = std::max({wmx[0] - wmn[0], wmx[1] - wmn[1], wmx[2] - wmn[2]});
    const float pad = (amax + ext) * 1.9073486328125e-06f * 2.0f;
    for (int k = 0; k < 3; ++k) { it.mn[k] = wmn[k] - pad; it.mx[k] = wmx[k] + pad; smin[k] = std::min(smin[k], wmn[k]); smax[k] = std::max(smax[k], wmx[k]); }
    it.ref = kInstLeafTag | (uint32_t)r->inst_refs.size();
    it.need = 4u + bl.b.stack_need;  // the world-space ray (3 entries) and the exit mark wait below the instance's own entries
    deepest = std::max(deepest, bl.b.max_depth);
    if (r->inst_refs.size() >= 0x0ffffff0u) RT_FAIL("Too many instances.");
    r->inst_refs.push_back(ref);
    items.push_back(it);
  }
  if (items.size() > r->tlas_capacity) RT_FAIL("internal: instance levels larger than reserved");
  std::vector<BvhNode4> nodes;
  uint32_t levels = 0, need = 0;
  r->tlas_nodes = tlas_build(items, nodes, &levels, &need);
  RT_HIP(hipMemcpyAsync(r->d_nodes.ptr, nodes.data(), nodes.size() * sizeof(BvhNode4), hipMemcpyHostToDevice, r->stream));
  RT_HIP(r->d_inst_refs.upload(r->inst_refs.data(), r->inst_refs.size(), r->stream));
  RT_HIP(r->d_inst_info.upload(info.data(), info.size(), r->stream));
  RT_HIP(hipStreamSynchronize(r->stream));  // `nodes`, `info` go out of scope
  r->levels.refs_on_host = true;
  r->bvh.max_depth = levels + deepest;
  r->bvh.stack_need = need;
  for (int k = 0; k < 3; ++k) { r->bvh.scene_min[k] = items.empty() ? 0.0f : smin[k]; r->bvh.scene_max[k] = items.empty() ? 0.0f : smax[k]; }
  return HALA_OK;
}

// ---- one tree -------------------------------------------------------------------------------------------------------------------------
// Everything a tree reads that the host decides: its own instance tables, uploaded, and every field of Tree::b but the results — the
// tables' addresses, the tree's sub-ranges of the scene's arrays, the any-hit copy, the material tables, the build options.  The one
// tree of a one-level scene reads the scene's instance tables as they are and uploads nothing.
static int tree_publish(hala_rt_renderer* r, Tree& t) {
  const HostScene& hs = r->hs;
  BvhBuffers& b = t.b;
  if (!r->two_level) {  // the whole scene, flattened: triangle k of the tree has global id k
    b.primitives = r->d_instances.ptr; b.inst_first_tri = r->d_inst_first_tri.ptr;
    b.instance_count = (uint32_t)hs.instances.size(); b.tri_count = hs.triangle_count;
    b.gid_first = nullptr; b.inst_index = nullptr;
  } else {
    std::vector<hala_gpu_mesh_data> md;
    std::vector<uint32_t> first{0u}, gid, inst;
    if (t.object_space) {
      hala_gpu_mesh_data m{};
      uint32_t any = 0;
      while (hs.instance_prim[any] != t.prim) ++any;  // any instance of the primitive: material and buffer addresses are the primitive's
      m = hs.instances[any];
      const Mat4 id = Mat4::identity();
      memcpy(m.transform, id.m, 64);
      md.push_back(m); gid.push_back(0u); inst.push_back(kAbsent);
      first.push_back((uint32_t)(hs.prims[t.prim].indices.size() / 3));
    } else {
      for (uint32_t i : t.insts) {
        md.push_back(hs.instances[i]); gid.push_back(hs.inst_first_tri[i]); inst.push_back(i);
        first.push_back(first.back() + (hs.inst_first_tri[i + 1] - hs.inst_first_tri[i]));
      }
    }
    RT_HIP(t.d_md.upload(md.data(), md.size(), r->stream));
    RT_HIP(t.d_first.upload(first.data(), first.size(), r->stream));
    RT_HIP(t.d_gid.upload(gid.data(), gid.size(), r->stream));
    RT_HIP(t.d_inst.upload(inst.data(), inst.size(), r->stream));
    RT_HIP(hipStreamSynchronize(r->stream));
    b.primitives = t.d_md.ptr; b.inst_first_tri = t.d_first.ptr; b.instance_count = (uint32_t)md.size(); b.tri_count = first.back();
    b.gid_first = t.d_gid.ptr; b.inst_index = t.d_inst.ptr;
  }
  b.object_space = t.object_space;
  b.tris_by_id = r->d_tris_by_id.ptr + t.tri_off; b.tris = r->d_tris.ptr + t.tri_off; b.shade_tris = r->d_shade_tris.ptr + t.tri_off;
  b.tris_any = r->any_invisible ? r->d_tris_any.ptr + t.tri_off : nullptr;
  b.material_any_class = r->d_material_any_class.ptr; b.material_kind = r->d_material_kind.ptr; b.material_count = (uint32_t)hs.gpu_materials.size();
  b.nodes = r->d_nodes.ptr + t.node_off;
  b.opt = r->bvh.opt;
  return HALA_OK;
}

// builds / refits a published tree into its sub-ranges and makes its references absolute (nothing to do at offsets 0, 0: a one-level tree)
static int tree_fit(hala_rt_renderer* r, Tree& t, bool refit) {
  const std::string e = refit ? bvh_refit(t.b, r->stream) : bvh_build(t.b, r->leaf_max_built, r->stream);
  if (!e.empty()) RT_FAIL(e);
  const std::string e2 = bvh_relocate(t.b, t.node_off, t.tri_off, r->stream);
  if (!e2.empty()) RT_FAIL(e2);
  return HALA_OK;
}

// ---- tree quality (RENDER_SPEC §4.6) ------------------------------------------------------------------------------------------------
// the cost of the trees `which` (indices into QualityState::trees) as the node array stands -> their `now` fields.  Waits for the stream.
static int quality_measure(hala_rt_renderer* r, const std::vector<uint32_t>& which) {
  QualityState& q = r->quality;
  if (which.empty()) return HALA_OK;
  const size_t words = q.trees.size() * 3u;
  RT_HIP(q.d_out.grow(words));
  RT_HIP(q.d_partials.grow(kTreeCostPartialWords));
  if (q.h_words < words) {
    if (q.h_out) (void)hipHostFree(q.h_out);
    q.h_out = nullptr; q.h_words = 0;
    RT_HIP(hipHostMalloc(reinterpret_cast<void**>(&q.h_out), words * sizeof(unsigned long long), hipHostMallocDefault));
    q.h_words = words;
  }
  RT_HIP(hipMemsetAsync(q.d_out.ptr, 0, words * sizeof(unsigned long long), r->stream));
  for (uint32_t k : which) {
    const hala_tree_quality& t = q.trees[k];
    if ((size_t)t.first_node + t.node_count > r->d_nodes.count) RT_FAIL("internal: a measured tree lies outside the node array");
    launch_tree_cost(r->d_nodes.ptr + t.first_node, t.node_count, q.d_partials.ptr, q.d_out.ptr + 3u * (size_t)k, r->stream);
  }
  RT_HIP(hipGetLastError());
  RT_HIP(hipMemcpyAsync(q.h_out, q.d_out.ptr, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, r->stream));
  RT_HIP(hipStreamSynchronize(r->stream));
  for (uint32_t k : which) {
    hala_tree_quality& t = q.trees[k];
    t.node_q_now = q.h_out[3u * (size_t)k]; t.tri_q_now = q.h_out[3u * (size_t)k + 1u]; t.valid = q.h_out[3u * (size_t)k + 2u] ? 1u : 0u;
  }
  return HALA_OK;
}

// behind a build: the trees as they were just built become the baseline (built = now).  Policy off: nothing is kept, nothing runs
static int quality_built(hala_rt_renderer* r) {
  QualityState& q = r->quality;
  q.trees.clear();
  if (q.mode == HALA_REFIT_POLICY_OFF) return HALA_OK;
  std::vector<uint32_t> all;
  for (const auto& tr : r->trees) {
    hala_tree_quality t{};
    t.first_node = tr->node_off; t.node_count = tr->b.node_count;
    all.push_back((uint32_t)q.trees.size());
    q.trees.push_back(t);
  }
  if (quality_measure(r, all) != HALA_OK) { q.trees.clear(); return HALA_ERR; }
  for (hala_tree_quality& t : q.trees) { t.node_q_built = t.node_q_now; t.tri_q_built = t.tri_q_now; }
  return HALA_OK;
}

// behind the refits of a refit: `refitted` (indices as in hala_rt_renderer::trees) are measured and the policy is applied.  *rebuilt:
// build_bvh ran (all trees anew, traversal configured); the caller has nothing left to do for the trees
static int quality_after_refit(hala_rt_renderer* r, const std::vector<uint32_t>& refitted, bool* rebuilt) {
  QualityState& q = r->quality;
  if (q.mode == HALA_REFIT_POLICY_OFF) return HALA_OK;
  if (q.trees.size() != r->trees.size()) RT_FAIL("internal: the measured trees are not the scene's");
  for (hala_tree_quality& t : q.trees) t.rebuilt_last_refit = 0u;
  if (refitted.empty()) return HALA_OK;  // cameras, lights, nodes of instanced primitives: no tree moved
  if (quality_measure(r, refitted) != HALA_OK) return HALA_ERR;
  ++q.refits_measured;
  bool due = q.mode == HALA_REFIT_POLICY_ALWAYS;
  if (q.mode == HALA_REFIT_POLICY_THRESHOLD)
    for (uint32_t k : refitted) {
      const hala_tree_quality& t = q.trees[k];
      const double built = (double)(t.node_q_built + t.tri_q_built), now = (double)(t.node_q_now + t.tri_q_now);
      due = due || (t.valid && built > 0.0 && now / built > (double)q.max_inflation);
    }
  if (!due) return HALA_OK;
  if (build_bvh(r) != HALA_OK) return HALA_ERR;  // (measures what it built: built = now)
  for (hala_tree_quality& t : q.trees) t.rebuilt_last_refit = 1u;
  q.trees_rebuilt += q.trees.size();
  *rebuilt = true;
  return HALA_OK;
}

// ---- all trees ------------------------------------------------------------------------------------------------------------------------
// The trees: [0] the world tree over the instances that stay flattened (if any; in a one-level scene all of them, and the tree exists
// even when empty), then one per instanced primitive in order of first use — sub-ranges of the scene's arrays behind the nodes reserved
// for the instance levels (none in a one-level scene: its tree sits at node 0, triangle 0)
static int build_trees(hala_rt_renderer* r) {
  const HostScene& hs = r->hs;
  r->sync_host_mirror();
  r->nodes.analysed = false;  // RENDER_SPEC §20: the bind-time tables name the trees and the flags of the build before this one
  r->build_options_dirty = false;  // (they take effect here)
  classify_instances(r, &r->inst_instanced);
  r->two_level = false;
  for (uint8_t f : r->inst_instanced) r->two_level = r->two_level || f != 0;
  r->trees.clear();
  r->levels.release();
  r->levels.mode = r->levels.requested;  // the build option takes effect here: at a commit, or when a refit has to build again
  r->prim_tree.assign(hs.prims.size(), -1);
  std::unique_ptr<Tree> world(new Tree());
  uint32_t n_items = 0;
  for (size_t i = 0; i < hs.instances.size(); ++i) {
    if (!r->inst_instanced[i]) { world->insts.push_back((uint32_t)i); continue; }
    ++n_items;
    const uint32_t p = hs.instance_prim[i];
    if (r->prim_tree[p] < 0) r->prim_tree[p] = -2;  // marked; numbered below
  }
  uint32_t tri_at = 0;
  if (!r->two_level || !world->insts.empty()) {
    for (uint32_t i : world->insts) tri_at += hs.inst_first_tri[i + 1] - hs.inst_first_tri[i];
    world->b.tri_count = tri_at;
    ++n_items;
    r->trees.push_back(std::move(world));
  }
  for (size_t i = 0; i < hs.instances.size(); ++i) {
    const uint32_t p = hs.instance_prim[i];
    if (!r->inst_instanced[i] || r->prim_tree[p] != -2) continue;
    std::unique_ptr<Tree> t(new Tree());
    t->object_space = true; t->prim = p; t->tri_off = tri_at;
    t->b.tri_count = (uint32_t)(hs.prims[p].indices.size() / 3);
    tri_at += t->b.tri_count;
    r->prim_tree[p] = (int32_t)r->trees.size();
    r->trees.push_back(std::move(t));
  }
  if (r->two_level && tri_at >= (1u << 28)) RT_FAIL("The scene stores 2^28 triangles or more.");
  r->stored_tris = tri_at;
  r->tlas_nodes = 0;
  r->tlas_capacity = r->two_level ? std::max(1u, n_items) : 0u;
  uint32_t node_at = r->tlas_capacity;
  for (auto& t : r->trees) {
    t->node_off = node_at;
    t->node_cap = std::max<uint32_t>(t->b.tri_count, 2) - 1;
    node_at += t->node_cap;
  }
  RT_HIP(r->d_tris_by_id.resize(tri_at)); RT_HIP(r->d_tris.resize(tri_at)); RT_HIP(r->d_shade_tris.resize(tri_at));
  RT_HIP(r->d_nodes.resize(node_at));
  if (r->two_level) RT_HIP(hipMemsetAsync(r->d_nodes.ptr, 0xff, (size_t)node_at * sizeof(BvhNode4), r->stream));  // unused slots of the reserved ranges: absent children
  if (attach_any_triangles(r) != HALA_OK) return HALA_ERR;
  r->leaf_max_built = kLeafMax;
  if (!r->two_level) {
    // a scene this small will be staged in LDS (configure_traversal: 48 B per triangle + at most ~32 B of nodes per triangle); a larger
    // one-level tree: one consumer lane per triangle of a leaf item
    r->leaf_max_built = (size_t)tri_at * 80 <= kLdsStageBudget ? kLeafMaxStaged : std::min(kLeafMax, traverse_max_leaf(TreeForm::Large));
  }
  for (auto& t : r->trees)
    if (tree_publish(r, *t) != HALA_OK || tree_fit(r, *t, false) != HALA_OK) return HALA_ERR;
  r->bvh.tri_count = tri_at;
  if (r->two_level) {
    r->bvh.node_count = node_at;  // the node array as a whole (reserved ranges included: hala_rt_download_bvh)
    if (build_instance_levels(r, true) != HALA_OK) return HALA_ERR;
  } else {  // no levels in front: the totals are the tree's
    const BvhBuffers& b = r->trees[0]->b;
    r->bvh.node_count = b.node_count; r->bvh.max_depth = b.max_depth; r->bvh.stack_need = b.stack_need;
    memcpy(r->bvh.scene_min, b.scene_min, 12); memcpy(r->bvh.scene_max, b.scene_max, 12);
  }
  return configure_traversal(r);
}

int build_bvh(hala_rt_renderer* r) {
  if (build_trees(r) != HALA_OK) return HALA_ERR;
  return quality_built(r);  // RENDER_SPEC §4.6 (nothing with the policy off)
}

int refit_trees(hala_rt_renderer* r, const std::vector<uint32_t>& moved, bool published, bool policy, bool* rebuilt) {
  *rebuilt = false;
  if (published && r->two_level && r->levels.mode != 1u) RT_FAIL("internal: the instance levels are built on the host");
  for (uint32_t k : moved) {
    Tree& t = *r->trees[k];
    if (!published && tree_publish(r, t) != HALA_OK) return HALA_ERR;
    if (tree_fit(r, t, true) != HALA_OK) return HALA_ERR;
  }
  if (policy && quality_after_refit(r, moved, rebuilt) != HALA_OK) return HALA_ERR;  // RENDER_SPEC §4.6
  if (*rebuilt) return HALA_OK;
  if (r->two_level) {
    // RENDER_SPEC 4.5: a node that moves an instanced primitive only touches the instance levels, rebuilt at every refit
    if (build_instance_levels(r, false) != HALA_OK) return HALA_ERR;
  } else {
    if (moved.empty()) return HALA_OK;  // only cameras / lights moved (the interactive case: a camera node): the tree stands as it is
    const BvhBuffers& b = r->trees[0]->b;  // (a refit moves the bounds alone: the topology is frozen)
    memcpy(r->bvh.scene_min, b.scene_min, 12); memcpy(r->bvh.scene_max, b.scene_max, 12);
  }
  return configure_traversal(r);
}

}  // namespace rt

extern "C" {

int hala_rt_set_build_options(hala_rt_renderer* r, const hala_rt_build_options* o) {
  if (!r) RT_FAIL("The renderer handle is null!");
  if (!o) RT_FAIL("The build options are null!");
  if (o->builder > 3u || o->ploc_tail > 2u || o->instancing > 2u || o->texture_bundles > 1u || o->instance_levels > 1u) RT_FAIL("Invalid build options.");
  for (uint32_t v : o->reserved) if (v != 0u) RT_FAIL("Invalid build options (reserved fields must be 0).");
  r->instancing_mode = o->instancing;
  r->levels.requested = o->instance_levels;
  r->bundles.mode = o->texture_bundles;
  r->bvh.opt.builder = o->builder; r->bvh.opt.ploc_tail = o->ploc_tail;
  r->bvh.opt.ploc_look_every = o->ploc_look_every; r->bvh.opt.collapse_look_every = o->collapse_look_every;
  // RENDER_SPEC §20: the next hala_rt_refit classifies by the new rule and may build anew by these options; hala_rt_refit_nodes leaves
  // that to it (the host path), and the bind-time tables, which hold the old rule's candidates, are made again
  r->build_options_dirty = true;
  r->nodes.analysed = false;
  return HALA_OK;
}

int hala_rt_set_refit_policy(hala_rt_renderer* r, const hala_refit_policy* p) {
  if (!r) RT_FAIL("The renderer handle is null!");
  if (!p) RT_FAIL("The refit policy is null!");
  if (p->mode > HALA_REFIT_POLICY_MEASURE) RT_FAIL("Invalid refit policy (mode).");
  if (p->mode == HALA_REFIT_POLICY_THRESHOLD ? !(std::isfinite(p->max_inflation) && p->max_inflation >= 1.0f) : !(p->max_inflation == 0.0f))
    RT_FAIL("Invalid refit policy (max_inflation: finite and >= 1 with mode 1, 0 otherwise).");
  for (uint32_t v : p->reserved) if (v != 0u) RT_FAIL("Invalid refit policy (reserved fields must be 0).");
  QualityState& q = r->quality;
  q.mode = p->mode; q.max_inflation = p->max_inflation;
  if (q.mode == HALA_REFIT_POLICY_OFF) { q.trees.clear(); return HALA_OK; }
  if (!r->committed || !q.trees.empty()) return HALA_OK;
  // the trees as they stand become the baseline
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  RT_HIP(hipStreamSynchronize(r->stream));
  return quality_built(r);
}

int hala_rt_get_tree_quality(hala_rt_renderer* r, hala_tree_quality* dst, uint32_t capacity, uint32_t* tree_count,
                             unsigned long long* refits_measured, unsigned long long* trees_rebuilt_by_policy) {
  if (!r) RT_FAIL("The renderer handle is null!");
  const QualityState& q = r->quality;
  const size_t n = r->committed ? q.trees.size() : 0u;
  if (dst) memcpy(dst, q.trees.data(), std::min<size_t>(capacity, n) * sizeof(hala_tree_quality));
  if (tree_count) *tree_count = (uint32_t)n;
  if (refits_measured) *refits_measured = q.refits_measured;
  if (trees_rebuilt_by_policy) *trees_rebuilt_by_policy = q.trees_rebuilt;
  return HALA_OK;
}

int hala_rt_get_bvh_info(hala_rt_renderer* r, hala_bvh_info* out) {
  if (!r || !out) RT_FAIL("The renderer handle is null!");
  if (!r->committed) RT_FAIL("The top level acceleration structure is none!");
  out->node_count = r->bvh.node_count; out->triangle_count = r->hs.triangle_count; out->max_depth = r->bvh.max_depth; out->lds_node_count = r->lds_nodes;
  out->node_width = 4u;
  out->stored_triangle_count = r->stored_tris; out->instance_node_count = r->two_level ? r->tlas_nodes : 0u;
  out->instance_ref_count = r->two_level ? (uint32_t)r->inst_refs.size() : 0u;
  out->tree_bytes = (uint64_t)r->d_nodes.bytes() + r->d_tris.bytes() + r->d_tris_any.bytes() + r->d_shade_tris.bytes() + r->d_inst_refs.bytes() + r->d_inst_info.bytes();
  memcpy(out->scene_min, r->bvh.scene_min, 12); memcpy(out->scene_max, r->bvh.scene_max, 12);
  return HALA_OK;
}
int hala_rt_download_bvh(hala_rt_renderer* r, void* nodes_64B, void* triangles_48B) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!r->committed) RT_FAIL("The top level acceleration structure is none!");
  RT_HIP(hipStreamSynchronize(r->stream));
  if (nodes_64B) RT_HIP(hipMemcpy(nodes_64B, r->d_nodes.ptr, (size_t)r->bvh.node_count * 64, hipMemcpyDeviceToHost));
  if (triangles_48B && r->bvh.tri_count) {
    RT_HIP(hipMemcpy(triangles_48B, r->d_tris.ptr, (size_t)r->bvh.tri_count * 48, hipMemcpyDeviceToHost));
    Tri* t = static_cast<Tri*>(triangles_48B);
    for (uint32_t i = 0; i < r->bvh.tri_count; ++i) t[i].pad2 = 0u;  // word 11 is the library's own (shading kind for the hit queue): not part of the 48-B format
  }
  return HALA_OK;
}

int hala_rt_download_instance_refs(hala_rt_renderer* r, void* refs_64B, uint32_t capacity, uint32_t* count) {
  if (!r || !count) RT_FAIL("Invalid argument.");
  if (!r->committed) RT_FAIL("The top level acceleration structure is none!");
  *count = r->two_level ? (uint32_t)r->inst_refs.size() : 0u;
  if (refs_64B && r->two_level && fetch_instance_refs(r) != HALA_OK) return HALA_ERR;
  if (refs_64B && r->two_level) memcpy(refs_64B, r->inst_refs.data(), std::min<size_t>(capacity, r->inst_refs.size()) * sizeof(InstRef));
  return HALA_OK;
}

}  // extern "C"
