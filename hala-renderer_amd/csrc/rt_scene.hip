// rt_scene.hip — the scene on the device: the packed records, the textures and their bundles (BundleState), the trees (one level
// or two) and the traversal configuration, the edit and refit API, and the introspection of trees and textures.
#include "renderer_state.h"

namespace rt {

// geometry = false re-publishes only the small records (cameras, lights, materials, instances): what a refit needs, since
// node transforms move instances, cameras and lights but leave the vertex / index arenas untouched.
int upload_packed(hala_rt_renderer* r, bool geometry) {
  HostScene& hs = r->hs;
  if (geometry) {
  // one arena each for all vertex / index buffers (the reference creates one buffer pair per primitive,
  // gpu_uploader.rs:421-456; device addresses per primitive are what matters to the shaders, :869-870)
  size_t nv = 0, ni = 0;
  r->prim_vertex_offset.clear(); r->prim_index_offset.clear();
  for (const auto& p : hs.prims) {
    r->prim_vertex_offset.push_back(nv); r->prim_index_offset.push_back(ni);
    nv += p.vertices.size();
    ni += (p.indices.size() + 3) & ~size_t(3);  // keep every index buffer 16-B aligned
  }
  RT_HIP(r->d_vertices.resize(nv)); RT_HIP(r->d_indices.resize(ni));
  for (size_t k = 0; k < hs.prims.size(); ++k) {
    const auto& p = hs.prims[k];
    if (!p.vertices.empty()) RT_HIP(hipMemcpyAsync(r->arena(k), p.vertices.data(), p.vertices.size() * sizeof(hala_vertex), hipMemcpyHostToDevice, r->stream));
    if (!p.indices.empty()) RT_HIP(hipMemcpyAsync(r->d_indices.ptr + r->prim_index_offset[k], p.indices.data(), p.indices.size() * 4, hipMemcpyHostToDevice, r->stream));
  }
  }
  for (size_t i = 0; i < hs.instances.size(); ++i) {
    const uint32_t p = hs.instance_prim[i];
    hs.instances[i].vertices = reinterpret_cast<uint64_t>(r->arena(p));  // get_device_address (:869)
    hs.instances[i].indices = reinterpret_cast<uint64_t>(r->d_indices.ptr + r->prim_index_offset[p]);     // (:870)
  }
  RT_HIP(r->d_cameras.upload(hs.cameras.data(), hs.cameras.size(), r->stream));
  RT_HIP(r->d_lights.upload(hs.lights.data(), hs.lights.size(), r->stream));
  RT_HIP(r->d_materials.upload(hs.gpu_materials.data(), hs.gpu_materials.size(), r->stream));
  {
    std::vector<uint8_t> kind(hs.gpu_materials.size());
    for (size_t i = 0; i < kind.size(); ++i) kind[i] = shade_kind_of(hs.gpu_materials[i], (uint32_t)hs.texture_image.size());
    RT_HIP(r->d_material_kind.upload(kind.data(), kind.size(), r->stream));
    r->material_kind = kind;
    uint32_t seen = 0;
    for (uint8_t k : kind) seen |= 1u << k;
    r->shade_sort = (seen & (seen - 1u)) != 0u;  // two kinds or more (a one-kind scene like the Cornell box only pays for the sort)
    r->scatter_media = false;
    for (const auto& m : hs.gpu_materials) r->scatter_media = r->scatter_media || m.medium_type == 2u;
    r->simple_materials = seen == (1u << kShadeKindFirst);  // nothing but untextured opaque DIFFUSE: the SIMPLE shade kernels (configs[1])
  }
  RT_HIP(r->d_instances.upload(hs.instances.data(), hs.instances.size(), r->stream));
  RT_HIP(r->d_inst_first_tri.upload(hs.inst_first_tri.data(), hs.inst_first_tri.size(), r->stream));
  // RENDER_SPEC §13: the node each instance and each light came from (the ids AOV)
  RT_HIP(r->d_inst_node.upload(hs.instance_node.data(), hs.instance_node.size(), r->stream));
  RT_HIP(r->d_light_node.upload(hs.light_node.data(), hs.light_node.size(), r->stream));
  RT_HIP(hipStreamSynchronize(r->stream));
  return HALA_OK;
}

// textures: upload level 0 of every image, build the mip chains on the GPU (gen_mipmaps, gpu_uploader.rs:400), publish
// one TexDesc per texture.  mip count = ceil(log2(max(w,h))) + 1 (gpu_uploader.rs:366), capped at kMaxMips.
int upload_textures(hala_rt_renderer* r) {
  const HostScene& hs = r->hs;
  std::vector<TexDesc> img_desc(hs.images.size());
  size_t total_f = 0, total_8 = 0, largest_8 = 0;  // float4 texels / tiled 4-B texels / largest level 0 among the 8-bit images
  for (size_t k = 0; k < hs.images.size(); ++k) {
    TexDesc& td = img_desc[k];
    memset(&td, 0, sizeof(td));
    td.width = hs.images[k].width; td.height = hs.images[k].height; td.format = hs.images[k].format;
    uint32_t m = std::max(td.width, td.height), p2 = 1, lg = 0;
    while (p2 < m) { p2 <<= 1; ++lg; }
    td.mips = std::min<uint32_t>(lg + 1, kMaxMips);
    size_t& total = td.format == kTexFloat ? total_f : total_8;
    for (uint32_t l = 0; l < td.mips; ++l) {
      if (total > 0xffffffffull) RT_FAIL("The texture arena exceeds 2^32 texels.");
      td.mip_offset[l] = (uint32_t)total;
      const uint32_t lw = std::max(1u, td.width >> l), lh = std::max(1u, td.height >> l);
      total += td.format == kTexFloat ? (size_t)lw * lh : (size_t)tex_tiled_size(lw, lh);
    }
    if (td.format != kTexFloat) largest_8 = std::max(largest_8, (size_t)td.width * td.height);
  }
  RT_HIP(r->d_tex_arena.resize(total_f));
  RT_HIP(r->d_tex_arena8.resize(total_8));
  if (total_8) RT_HIP(hipMemsetAsync(r->d_tex_arena8.ptr, 0, total_8 * 4, r->stream));  // the padding texels of partial tiles
  // the sRGB decode table and the midpoints between its entries (the encoder of the 8-bit mip chain bisects them)
  const float* lut = srgb_decode_lut();
  float thr[256];
  for (int k = 0; k < 255; ++k) thr[k] = (lut[k] + lut[k + 1]) * 0.5f;
  thr[255] = 3.402823466e+38f;
  float lut512[512];  // shading.h::tex8_fetch: the sRGB EOTF, then b / 255
  for (int k = 0; k < 256; ++k) { lut512[k] = lut[k]; lut512[256 + k] = (float)k / 255.0f; }
  RT_HIP(r->d_srgb_lut.upload(lut512, 512, r->stream));
  RT_HIP(r->d_srgb_thr.upload(thr, 256, r->stream));
  DeviceArray<uint32_t> staging;  // row-major level 0 of one 8-bit image at a time
  RT_HIP(staging.resize(largest_8));
  for (size_t k = 0; k < hs.images.size(); ++k) {
    const TexDesc& td = img_desc[k];
    if (td.format == kTexFloat) {
      RT_HIP(hipMemcpyAsync(r->d_tex_arena.ptr + td.mip_offset[0], hs.images[k].rgba.data(), (size_t)td.width * td.height * 16, hipMemcpyHostToDevice, r->stream));
      for (uint32_t l = 1; l < td.mips; ++l)
        launch_mip_downsample(r->d_tex_arena.ptr + td.mip_offset[l - 1], std::max(1u, td.width >> (l - 1)), std::max(1u, td.height >> (l - 1)),
                              r->d_tex_arena.ptr + td.mip_offset[l], std::max(1u, td.width >> l), std::max(1u, td.height >> l), r->stream);
    } else {
      RT_HIP(hipMemcpyAsync(staging.ptr, hs.images[k].rgba8.data(), (size_t)td.width * td.height * 4, hipMemcpyHostToDevice, r->stream));
      launch_tile8(staging.ptr, td.width, td.height, r->d_tex_arena8.ptr + td.mip_offset[0], r->stream);
      for (uint32_t l = 1; l < td.mips; ++l)
        launch_mip_downsample8(r->d_tex_arena8.ptr + td.mip_offset[l - 1], std::max(1u, td.width >> (l - 1)), std::max(1u, td.height >> (l - 1)),
                               r->d_tex_arena8.ptr + td.mip_offset[l], std::max(1u, td.width >> l), std::max(1u, td.height >> l), td.format,
                               r->d_srgb_lut.ptr, r->d_srgb_thr.ptr, r->stream);
    }
  }
  std::vector<TexDesc> tex(hs.texture_image.size());
  for (size_t i = 0; i < tex.size(); ++i) tex[i] = img_desc[hs.texture_image[i]];
  RT_HIP(r->d_textures.upload(tex.data(), tex.size(), r->stream));
  RT_HIP(hipStreamSynchronize(r->stream));  // (also: `staging` and the host images may go)
  RT_HIP(hipGetLastError());
  r->host_textures = tex;
  return HALA_OK;
}

// Texel bundles: one per distinct tuple of images that a material's maps show, for the materials that reference at least two maps, all
// 8-bit and of equal width and height; every other material keeps fetching from the per-texture arenas (kAbsent in the table).
// fresh: a commit — everything is decided and built again.  Otherwise a refit: hala_rt_update_material may have changed map indices; the
// table follows, and the arena is rebuilt when a tuple appears that has no bundle yet (bundles no longer referenced stay until then).
// The levels are interleaved on the device from the levels upload_textures built: the texel words are the same by construction.
int update_texture_bundles(hala_rt_renderer* r, bool fresh) {
  const HostScene& hs = r->hs;
  const uint32_t nt = (uint32_t)r->host_textures.size();
  if (fresh) {
    r->bundles.on = r->bundles.mode == 0u;
    r->bundles.sources.clear(); r->bundles.host.clear();
  }
  std::vector<BundleState::Source> sources = r->bundles.sources;
  std::vector<uint32_t> table(hs.gpu_materials.size(), kAbsent);
  uint32_t bundled = 0, textured = 0;
  for (size_t m = 0; m < hs.gpu_materials.size(); ++m) {
    const hala_gpu_material& gm = hs.gpu_materials[m];
    const uint32_t idx[kBundleLanes] = {gm.base_color_map_index, gm.normal_map_index, gm.metallic_roughness_map_index, gm.emission_map_index};
    BundleState::Source src;
    uint32_t maps = 0, w = 0, h = 0;
    bool same = true;
    for (uint32_t k = 0; k < kBundleLanes; ++k) {
      src.image[k] = src.texture[k] = kAbsent;
      if (idx[k] >= nt) continue;
      const TexDesc& td = r->host_textures[idx[k]];
      if (maps == 0) { w = td.width; h = td.height; }
      same = same && td.format != kTexFloat && td.width == w && td.height == h;
      src.image[k] = hs.texture_image[idx[k]]; src.texture[k] = idx[k];
      ++maps;
    }
    if (maps == 0) continue;
    ++textured;
    if (!r->bundles.on || maps < kBundleMinMaps || !same) continue;
    size_t b = 0;
    while (b < sources.size() && memcmp(sources[b].image, src.image, sizeof(src.image)) != 0) ++b;
    if (b == sources.size()) sources.push_back(src);
    table[m] = (uint32_t)b;
    ++bundled;
  }
  if (sources.size() != r->bundles.host.size()) {  // new tuples: lay the arena out again and fill it
    std::vector<BundleDesc> descs(sources.size());
    size_t lines = 0;
    for (size_t b = 0; b < sources.size(); ++b) {
      BundleDesc& bd = descs[b];
      memset(&bd, 0, sizeof(bd));
      for (uint32_t k = 0; k < kBundleLanes; ++k) {
        if (sources[b].texture[k] == kAbsent) continue;
        const TexDesc& td = r->host_textures[sources[b].texture[k]];
        bd.width = td.width; bd.height = td.height; bd.mips = td.mips;
        bd.formats |= td.format << (8u * k);
      }
      for (uint32_t l = 0; l < bd.mips; ++l) {
        if (lines > 0xffffffffull) break;
        bd.mip_offset[l] = (uint32_t)lines;
        lines += bundle_level_lines(std::max(1u, bd.width >> l), std::max(1u, bd.height >> l));
      }
    }
    // automatic mode: an arena that cannot be addressed or cannot be had leaves every material on the per-texture path
    bool ok = lines <= 0xffffffffull;
    if (ok && r->bundles.d_arena.resize(lines * 4) != hipSuccess) { (void)hipGetLastError(); ok = false; }
    if (!ok) {
      r->bundles.off();
      std::fill(table.begin(), table.end(), kAbsent);
      bundled = 0;
    } else {
      RT_HIP(hipMemsetAsync(r->bundles.d_arena.ptr, 0, lines * 64, r->stream));  // absent lanes, the padding texels of odd sizes
      for (size_t b = 0; b < sources.size(); ++b)
        for (uint32_t k = 0; k < kBundleLanes; ++k) {
          if (sources[b].texture[k] == kAbsent) continue;
          const TexDesc& td = r->host_textures[sources[b].texture[k]];
          for (uint32_t l = 0; l < td.mips; ++l)
            launch_bundle_interleave(r->d_tex_arena8.ptr + td.mip_offset[l], std::max(1u, td.width >> l), std::max(1u, td.height >> l),
                                     r->bundles.d_arena.ptr + ((size_t)descs[b].mip_offset[l] << 2), k, r->stream);
        }
      RT_HIP(r->bundles.d_descs.upload(descs.data(), descs.size(), r->stream));
      r->bundles.sources = sources; r->bundles.host = descs;
    }
  }
  if (r->bundles.host.empty()) r->bundles.d_arena.release();
  RT_HIP(r->bundles.d_material.upload(table.data(), table.size(), r->stream));
  RT_HIP(hipStreamSynchronize(r->stream));  // (`table` and `descs` may go)
  RT_HIP(hipGetLastError());
  r->bundles.bundled_materials = bundled; r->bundles.unbundled_textured_materials = textured - bundled;
  return HALA_OK;
}

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

// RENDER_SPEC 7.1d: scenes with opacity-0 materials get a second copy of the BVH-order triangles for the any-hit launches
static int attach_any_triangles(hala_rt_renderer* r) {
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
  if (r->any_invisible) RT_HIP(r->d_tris_any.resize(r->two_level ? r->stored_tris : r->hs.triangle_count));
  r->bvh.tris_any = r->any_invisible ? r->d_tris_any.ptr : nullptr;
  r->bvh.material_any_class = r->d_material_any_class.ptr;
  r->bvh.material_kind = r->d_material_kind.ptr;
  r->bvh.material_count = (uint32_t)r->hs.gpu_materials.size();
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
static void classify_instances(hala_rt_renderer* r, std::vector<uint8_t>* flags) {
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
  const bool world = !r->blas.empty() && !r->blas[0]->object_space && r->blas[0]->b.tri_count;
  std::vector<InstTree> trees(r->blas.size());
  uint32_t deepest = 0, largest_need = 0;
  for (size_t t = 0; t < r->blas.size(); ++t) {
    const hala_rt_renderer::Blas& bl = *r->blas[t];
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
    if (!r->blas.empty() && !r->blas[0]->object_space) {
      uint32_t at = r->blas[0]->tri_off;
      for (uint32_t i : r->blas[0]->insts) { flat_base[i] = at; at += hs.inst_first_tri[i + 1] - hs.inst_first_tri[i]; }
    }
    if (world) items.push_back(InstItem{kAbsent, 0u});
    for (size_t i = 0; i < hs.instances.size(); ++i) {
      info[i].first_tri = hs.inst_first_tri[i];
      info[i].instanced = r->inst_instanced[i];
      info[i].pad = 0;
      if (!r->inst_instanced[i]) { info[i].shade_base = flat_base[i]; continue; }
      const uint32_t t = (uint32_t)r->prim_blas[hs.instance_prim[i]];
      info[i].shade_base = r->blas[t]->tri_off;
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
  if (!r->blas.empty() && !r->blas[0]->object_space) {
    const hala_rt_renderer::Blas& w = *r->blas[0];
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
    const hala_rt_renderer::Blas& bl = *r->blas[(size_t)r->prim_blas[hs.instance_prim[i]]];
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

// builds / refits one tree of a two-level scene into its sub-ranges and makes its references absolute
static int blas_build_or_refit(hala_rt_renderer* r, hala_rt_renderer::Blas& bl, bool refit) {
  const HostScene& hs = r->hs;
  std::vector<hala_gpu_mesh_data> md;
  std::vector<uint32_t> first{0u}, gid, inst;
  if (bl.object_space) {
    hala_gpu_mesh_data m{};
    uint32_t any = 0;
    while (hs.instance_prim[any] != bl.prim) ++any;  // any instance of the primitive: material and buffer addresses are the primitive's
    m = hs.instances[any];
    const Mat4 id = Mat4::identity();
    memcpy(m.transform, id.m, 64);
    md.push_back(m); gid.push_back(0u); inst.push_back(kAbsent);
    first.push_back((uint32_t)(hs.prims[bl.prim].indices.size() / 3));
  } else {
    for (uint32_t i : bl.insts) {
      md.push_back(hs.instances[i]); gid.push_back(hs.inst_first_tri[i]); inst.push_back(i);
      first.push_back(first.back() + (hs.inst_first_tri[i + 1] - hs.inst_first_tri[i]));
    }
  }
  RT_HIP(bl.d_md.upload(md.data(), md.size(), r->stream));
  RT_HIP(bl.d_first.upload(first.data(), first.size(), r->stream));
  RT_HIP(bl.d_gid.upload(gid.data(), gid.size(), r->stream));
  RT_HIP(bl.d_inst.upload(inst.data(), inst.size(), r->stream));
  RT_HIP(hipStreamSynchronize(r->stream));
  BvhBuffers& b = bl.b;
  b.primitives = bl.d_md.ptr; b.inst_first_tri = bl.d_first.ptr; b.instance_count = (uint32_t)md.size(); b.tri_count = first.back();
  b.gid_first = bl.d_gid.ptr; b.inst_index = bl.d_inst.ptr; b.object_space = bl.object_space;
  b.tris_by_id = r->d_tris_by_id.ptr + bl.tri_off; b.tris = r->d_tris.ptr + bl.tri_off; b.shade_tris = r->d_shade_tris.ptr + bl.tri_off;
  b.tris_any = r->any_invisible ? r->d_tris_any.ptr + bl.tri_off : nullptr;
  b.material_any_class = r->d_material_any_class.ptr; b.material_kind = r->d_material_kind.ptr; b.material_count = (uint32_t)hs.gpu_materials.size();
  b.nodes = r->d_nodes.ptr + bl.node_off;
  b.opt = r->bvh.opt;
  const std::string e = refit ? bvh_refit(b, r->stream) : bvh_build(b, kLeafMax, r->stream);
  if (!e.empty()) RT_FAIL(e);
  const std::string e2 = bvh_relocate(b, bl.node_off, bl.tri_off, r->stream);
  if (!e2.empty()) RT_FAIL(e2);
  return HALA_OK;
}

static int build_two_level(hala_rt_renderer* r) {
  const HostScene& hs = r->hs;
  r->blas.clear();
  r->prim_blas.assign(hs.prims.size(), -1);
  // the trees: [0] the world tree over the instances that stay flattened (if any), then one per instanced primitive in order of first use
  std::unique_ptr<hala_rt_renderer::Blas> world(new hala_rt_renderer::Blas());
  uint32_t n_items = 0;
  for (size_t i = 0; i < hs.instances.size(); ++i) {
    if (!r->inst_instanced[i]) { world->insts.push_back((uint32_t)i); continue; }
    ++n_items;
    const uint32_t p = hs.instance_prim[i];
    if (r->prim_blas[p] < 0) r->prim_blas[p] = -2;  // marked; numbered below
  }
  uint32_t tri_at = 0;
  if (!world->insts.empty()) {
    for (uint32_t i : world->insts) tri_at += hs.inst_first_tri[i + 1] - hs.inst_first_tri[i];
    world->tri_off = 0; world->b.tri_count = tri_at;
    ++n_items;
    r->blas.push_back(std::move(world));
  }
  for (size_t i = 0; i < hs.instances.size(); ++i) {
    const uint32_t p = hs.instance_prim[i];
    if (!r->inst_instanced[i] || r->prim_blas[p] != -2) continue;
    std::unique_ptr<hala_rt_renderer::Blas> bl(new hala_rt_renderer::Blas());
    bl->object_space = true; bl->prim = p; bl->tri_off = tri_at;
    bl->b.tri_count = (uint32_t)(hs.prims[p].indices.size() / 3);
    tri_at += bl->b.tri_count;
    r->prim_blas[p] = (int32_t)r->blas.size();
    r->blas.push_back(std::move(bl));
  }
  if (tri_at >= (1u << 28)) RT_FAIL("The scene stores 2^28 triangles or more.");
  r->stored_tris = tri_at;
  r->tlas_capacity = std::max(1u, n_items);
  uint32_t node_at = r->tlas_capacity;
  for (auto& bl : r->blas) {
    bl->node_off = node_at;
    bl->node_cap = std::max<uint32_t>(bl->b.tri_count, 2) - 1;
    node_at += bl->node_cap;
  }
  RT_HIP(r->d_tris_by_id.resize(tri_at)); RT_HIP(r->d_tris.resize(tri_at)); RT_HIP(r->d_shade_tris.resize(tri_at));
  RT_HIP(r->d_nodes.resize(node_at));
  RT_HIP(hipMemsetAsync(r->d_nodes.ptr, 0xff, (size_t)node_at * sizeof(BvhNode4), r->stream));  // unused slots of the reserved ranges: absent children
  if (attach_any_triangles(r) != HALA_OK) return HALA_ERR;
  uint32_t nodes_used = r->tlas_capacity;
  for (auto& bl : r->blas) {
    if (blas_build_or_refit(r, *bl, false) != HALA_OK) return HALA_ERR;
    nodes_used = std::max(nodes_used, bl->node_off + bl->b.node_count);
  }
  r->bvh.tri_count = tri_at;
  r->bvh.node_count = node_at;  // the node array as a whole (reserved ranges included: hala_rt_download_bvh)
  r->bvh.tris_any = r->any_invisible ? r->d_tris_any.ptr : nullptr;
  r->leaf_max_built = kLeafMax;
  if (build_instance_levels(r, true) != HALA_OK) return HALA_ERR;
  return configure_traversal(r);
}

// ---- tree quality (RENDER_SPEC §4.6) ------------------------------------------------------------------------------------------------
// the cost of the trees `which` (indices into QualityState::trees) as the node array stands -> their `now` fields.  Waits for the stream.
static int quality_measure(hala_rt_renderer* r, const std::vector<uint32_t>& which) {
  QualityState& q = r->quality;
  if (which.empty()) return HALA_OK;
  const size_t words = q.trees.size() * 3u;
  if (q.d_out.count < words) RT_HIP(q.d_out.resize(words));
  if (q.d_partials.count < kTreeCostPartialWords) RT_HIP(q.d_partials.resize(kTreeCostPartialWords));
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
  if (r->two_level) {
    for (const auto& bl : r->blas) {
      hala_tree_quality t{};
      t.first_node = bl->node_off; t.node_count = bl->b.node_count;
      all.push_back((uint32_t)q.trees.size());
      q.trees.push_back(t);
    }
  } else {
    hala_tree_quality t{};
    t.first_node = 0u; t.node_count = r->bvh.node_count;
    all.push_back(0u);
    q.trees.push_back(t);
  }
  if (quality_measure(r, all) != HALA_OK) { q.trees.clear(); return HALA_ERR; }
  for (hala_tree_quality& t : q.trees) { t.node_q_built = t.node_q_now; t.tri_q_built = t.tri_q_now; }
  return HALA_OK;
}

// behind the refits of a refit: `refitted` (indices as in hala_rt_renderer::blas; {0} for a one-level tree) are measured and the policy
// is applied.  *rebuilt: build_bvh ran (all trees anew, traversal configured); the caller has nothing left to do for the trees
static int quality_after_refit(hala_rt_renderer* r, const std::vector<uint32_t>& refitted, bool* rebuilt) {
  QualityState& q = r->quality;
  *rebuilt = false;
  if (q.mode == HALA_REFIT_POLICY_OFF) return HALA_OK;
  if (q.trees.size() != (r->two_level ? r->blas.size() : (size_t)1)) RT_FAIL("internal: the measured trees are not the scene's");
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

static int build_trees(hala_rt_renderer* r) {
  r->sync_host_mirror();
  r->nodes.analysed = false;  // RENDER_SPEC §20: the bind-time tables name the trees and the flags of the build before this one
  r->build_options_dirty = false;  // (they take effect here)
  classify_instances(r, &r->inst_instanced);
  r->two_level = false;
  for (uint8_t f : r->inst_instanced) r->two_level = r->two_level || f != 0;
  if (r->bvh.topology) { bvh_free_topology(r->bvh.topology); r->bvh.topology = nullptr; }
  r->blas.clear();
  r->levels.release();
  r->levels.mode = r->levels.requested;  // the build option takes effect here: at a commit, or when a refit has to build again
  r->bvh.gid_first = nullptr; r->bvh.inst_index = nullptr; r->bvh.object_space = false;
  if (r->two_level) return build_two_level(r);
  const uint32_t n = r->hs.triangle_count;
  r->stored_tris = n; r->tlas_nodes = 0; r->tlas_capacity = 0;
  RT_HIP(r->d_tris_by_id.resize(n)); RT_HIP(r->d_tris.resize(n)); RT_HIP(r->d_shade_tris.resize(n));
  RT_HIP(r->d_nodes.resize(std::max<uint32_t>(n, 2) - 1));
  r->bvh.primitives = r->d_instances.ptr; r->bvh.inst_first_tri = r->d_inst_first_tri.ptr;
  r->bvh.instance_count = (uint32_t)r->hs.instances.size(); r->bvh.tri_count = n;
  r->bvh.tris_by_id = r->d_tris_by_id.ptr; r->bvh.shade_tris = r->d_shade_tris.ptr; r->bvh.tris = r->d_tris.ptr; r->bvh.nodes = r->d_nodes.ptr;
  if (attach_any_triangles(r) != HALA_OK) return HALA_ERR;
  // a scene this small will be staged in LDS (configure_traversal: 48 B per triangle + at most ~32 B of nodes per triangle)
  uint32_t leaf_max = (size_t)n * 80 <= kLdsStageBudget ? kLeafMaxStaged : kLeafMax;
  if ((size_t)n * 80 > kLdsStageBudget) leaf_max = std::min(leaf_max, traverse_max_leaf(TreeForm::Large));  // one consumer lane per triangle of a leaf item
  const std::string e = bvh_build(r->bvh, leaf_max, r->stream);
  if (!e.empty()) RT_FAIL(e);
  r->leaf_max_built = leaf_max;
  return configure_traversal(r);
}

int build_bvh(hala_rt_renderer* r) {
  if (build_trees(r) != HALA_OK) return HALA_ERR;
  return quality_built(r);  // RENDER_SPEC §4.6 (nothing with the policy off)
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

// ---- textures (set 2 binding 0) ---------------------------------------------------------------------------------------
int hala_rt_get_texture_info(hala_rt_renderer* r, uint32_t texture, uint32_t* width, uint32_t* height, uint32_t* mips) {
  if (!r) RT_FAIL("The renderer handle is null!");
  if (!r->has_scene || texture >= r->host_textures.size()) RT_FAIL("The texture does not exist.");
  const TexDesc& td = r->host_textures[texture];
  if (width) *width = td.width;
  if (height) *height = td.height;
  if (mips) *mips = td.mips;
  return HALA_OK;
}
int hala_rt_texture_bundle_info(hala_rt_renderer* r, hala_texture_bundle_info* info) {
  if (!r) RT_FAIL("The renderer handle is null!");
  if (!info) RT_FAIL("Invalid argument.");
  if (!r->committed) RT_FAIL("The top level acceleration structure is none!");
  info->bundle_count = (uint32_t)r->bundles.host.size();
  info->bundled_materials = r->bundles.bundled_materials;
  info->unbundled_textured_materials = r->bundles.unbundled_textured_materials;
  info->reserved = 0;
  info->bundle_bytes = r->bundles.host.empty() ? 0ull : (unsigned long long)r->bundles.d_arena.count * 16ull;
  return HALA_OK;
}
int hala_rt_read_texture_level(hala_rt_renderer* r, uint32_t texture, uint32_t level, float* dst_rgba32f) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!r->has_scene || texture >= r->host_textures.size() || !dst_rgba32f) RT_FAIL("The texture does not exist.");
  const TexDesc& td = r->host_textures[texture];
  if (level >= td.mips) RT_FAIL("The mip level does not exist.");
  const uint32_t lw = std::max(1u, td.width >> level), lh = std::max(1u, td.height >> level);
  const size_t n = (size_t)lw * lh;
  if (td.format == kTexFloat) {
    RT_HIP(hipMemcpy(dst_rgba32f, r->d_tex_arena.ptr + td.mip_offset[level], n * 16, hipMemcpyDeviceToHost));
    return HALA_OK;
  }
  // 8-bit texels: de-tile and decode on the host exactly like the sampler does on the device
  std::vector<uint32_t> tiled(tex_tiled_size(lw, lh));
  RT_HIP(hipMemcpy(tiled.data(), r->d_tex_arena8.ptr + td.mip_offset[level], tiled.size() * 4, hipMemcpyDeviceToHost));
  const float* lut = srgb_decode_lut();
  for (uint32_t y = 0; y < lh; ++y)
    for (uint32_t x = 0; x < lw; ++x) {
      const uint32_t t = tiled[tex_tiled_index(x, y, lw)];
      float* o = dst_rgba32f + ((size_t)y * lw + x) * 4;
      for (int c = 0; c < 3; ++c) { const uint32_t b = (t >> (8 * c)) & 0xffu; o[c] = td.format == kTexSrgb8 ? lut[b] : (float)b / 255.0f; }
      o[3] = (float)(t >> 24) / 255.0f;
    }
  return HALA_OK;
}
int hala_rt_sample_texture_host(hala_rt_renderer* r, uint32_t texture, const float* uv_lod, uint32_t count, float* dst_rgba32f) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!r->has_scene || texture >= r->host_textures.size()) RT_FAIL("The texture does not exist.");
  if (!count) return HALA_OK;
  if (!uv_lod || !dst_rgba32f) RT_FAIL("Invalid argument.");
  DeviceArray<float> d_in;
  DeviceArray<float4> d_out;
  RT_HIP(d_in.upload(uv_lod, (size_t)count * 3, r->stream));
  RT_HIP(d_out.resize(count));
  launch_sample_texture(r->view(), texture, d_in.ptr, count, d_out.ptr, r->stream);
  RT_HIP(hipMemcpyAsync(dst_rgba32f, d_out.ptr, (size_t)count * 16, hipMemcpyDeviceToHost, r->stream));
  RT_HIP(hipStreamSynchronize(r->stream));
  RT_HIP(hipGetLastError());
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
int hala_rt_update_node_transform(hala_rt_renderer* r, uint32_t node_index, const float local_transform[16]) {
  if (!r || !local_transform) RT_FAIL("Invalid argument.");
  if (!r->committed) RT_FAIL("The top level acceleration structure is none!");  // commit builds from what set_scene packed: an edit before it would not reach it
  if (node_index >= r->hs.nodes.size()) RT_FAIL("The node does not exist.");
  if (r->shutter.rec.nodes.count(node_index)) RT_FAIL("The node has shutter keys: clear them first (hala_rt_set_node_keys with both keys NULL).");
  r->sync_host_mirror();  // RENDER_SPEC §20: from the locals the trees stand at, before one of them changes
  memcpy(r->hs.nodes[node_index].local.m, local_transform, 64);
  r->nodes_dirty = true;
  return HALA_OK;
}
int hala_rt_update_vertices(hala_rt_renderer* r, uint32_t mesh_index, uint32_t primitive_index, const hala_vertex* vertices, uint32_t vertex_count) {
  if (!r || !vertices) RT_FAIL("Invalid argument.");
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!r->committed) RT_FAIL("The top level acceleration structure is none!");
  uint32_t prim = 0;
  if (find_primitive(r, mesh_index, primitive_index, &prim) != HALA_OK) return HALA_ERR;
  HostPrimitive& p = r->hs.prims[prim];
  if (deform_registered(r, prim)) RT_FAIL("The primitive has a deformer: clear it first (hala_rt_clear_deformer).");
  if (r->shutter.rec.vertices.count(prim)) RT_FAIL("The primitive has shutter keys: clear them first (hala_rt_set_vertex_keys with both keys NULL).");
  if (vertex_count != p.vertices.size()) RT_FAIL("The vertex count differs from the primitive's (" + std::to_string(p.vertices.size()) + "): refit keeps the topology, use set_scene + commit.");
  for (uint32_t k = 0; k < vertex_count; ++k)
    if (!all_finite(vertices[k].position, 3)) RT_FAIL("Vertex position is not finite.");
  memcpy(p.vertices.data(), vertices, (size_t)vertex_count * sizeof(hala_vertex));
  r->vertices_dirty = true;
  if (r->shutter.act.active()) {  // RENDER_SPEC §18: the steps until the refit read the arena; the refit uploads the host copy
    r->shutter.stale.push_back(prim);
    return HALA_OK;
  }
  // the copy below reads the renderer's own host copy, which outlives it; earlier frames still read the arena: wait for them
  RT_HIP(hipStreamSynchronize(r->stream));
  mark_no_history(r, prim);
  if (vertex_count) RT_HIP(hipMemcpyAsync(r->arena(prim), p.vertices.data(), (size_t)vertex_count * sizeof(hala_vertex), hipMemcpyHostToDevice, r->stream));
  return HALA_OK;
}
int hala_rt_update_material(hala_rt_renderer* r, uint32_t material_index, const hala_material_desc* material) {
  if (!r || !material) RT_FAIL("Invalid argument.");
  if (!r->committed) RT_FAIL("The top level acceleration structure is none!");
  if (material_index >= r->hs.materials.size()) RT_FAIL("The material does not exist.");
  if (material->type > 1u) RT_FAIL("Invalid material type.");  // cpu/material.rs:14
  if (r->hs.materials[material_index].opacity == 0.0f || material->opacity == 0.0f) r->materials_dirty_any = true;
  r->hs.materials[material_index] = *material;
  r->materials_dirty = true;
  if (r->temporal.enabled && material_index < r->temporal.mat_marked.size()) { r->temporal.mat_marked[material_index] = 1; r->temporal.table_dirty = true; }  // RENDER_SPEC §16
  return HALA_OK;
}
}  // extern "C"

namespace rt {

// The geometry part of hala_rt_refit: everything but the restart of the accumulation, fitted to `in` (renderer_state.h).  The caller has
// joined both frame slots, waited, and posed what is posed on the device (deform_pose, k_shutter_lerp).  A step of the shutter
// (RENDER_SPEC §18) is this alone.  What the caller recorded — HostNode::local, HostScene::materials, the dirty flags — is neither read
// nor written here.
int refit_geometry(hala_rt_renderer* r, const RefitInputs& in) {
  // RENDER_SPEC §20: `before` must describe the state the trees are fitted to, also after hala_rt_refit_nodes posed it on the device; and
  // what follows moves the world transforms on the host, so the device tables of the node batch lag from here on
  r->sync_host_mirror();
  r->nodes.tables_current = false;
  const std::vector<hala_gpu_mesh_data> before = r->hs.instances;  // object -> world of every instance as the tree was fitted to it
  const std::vector<uint8_t> kinds_before = r->material_kind;
  r->hs.update_node_hierarchies(in.locals);
  const std::string e = r->hs.pack(in.materials);
  if (!e.empty()) RT_FAIL(e);
  if (upload_packed(r, false) != HALA_OK) return HALA_ERR;
  if (update_texture_bundles(r, false) != HALA_OK) return HALA_ERR;  // a material edit may have changed which maps a material references
  r->bvh.primitives = r->d_instances.ptr; r->bvh.inst_first_tri = r->d_inst_first_tri.ptr;
  // only cameras / lights moved (the interactive case: a camera node): the geometry and its tree stand as they are
  const bool had_invisible = r->any_invisible;
  const std::vector<uint8_t> classes_before = r->material_any_class;
  if (attach_any_triangles(r) != HALA_OK) return HALA_ERR;
  // (a material edit can change which triangles the shadow rays see: their copy is rewritten by the refit pass)
  // (the BVH-order triangles carry their material's shading kind: rewritten by the refit pass as well)
  // what the trees hold changed: vertices or materials (the any-hit copy of the triangles must be rewritten when a class changed)
  const bool content = in.arena_changed || in.opacity0_edit || classes_before != r->material_any_class || had_invisible != r->any_invisible ||
                       kinds_before != r->material_kind;
  bool geometry_moved = content || before.size() != r->hs.instances.size();
  for (size_t i = 0; i < before.size() && !geometry_moved; ++i) geometry_moved = memcmp(before[i].transform, r->hs.instances[i].transform, 64) != 0;
  // which instances are intersected in object space may have changed (a transform that is no longer invertible, or is again): rebuild
  std::vector<uint8_t> flags;
  classify_instances(r, &flags);
  if (flags != r->inst_instanced) return build_bvh(r);
  std::vector<uint32_t> refitted;  // RENDER_SPEC §4.6: what the policy measures
  bool rebuilt = false;
  if (r->two_level) {
    // RENDER_SPEC 4.5: a node that moves an instanced primitive only touches the instance levels (rebuilt below, on the host or on the GPU).  The trees
    // underneath are refitted when what THEY hold changed: `content` (any tree), the transform of a flattened instance (the world tree)
    r->bvh.tris_any = r->any_invisible ? r->d_tris_any.ptr : nullptr;
    for (size_t k = 0; k < r->blas.size(); ++k) {
      hala_rt_renderer::Blas& bl = *r->blas[k];
      bool moved = content;
      if (!bl.object_space)
        for (uint32_t i : bl.insts) moved = moved || memcmp(before[i].transform, r->hs.instances[i].transform, 64) != 0;
      if (!moved) continue;
      if (blas_build_or_refit(r, bl, true) != HALA_OK) return HALA_ERR;
      refitted.push_back((uint32_t)k);
    }
    if (in.policy && quality_after_refit(r, refitted, &rebuilt) != HALA_OK) return HALA_ERR;
    if (rebuilt) return HALA_OK;
    if (build_instance_levels(r, false) != HALA_OK) return HALA_ERR;
    return configure_traversal(r);
  }
  if (geometry_moved) {
    const std::string e2 = bvh_refit(r->bvh, r->stream);
    if (!e2.empty()) RT_FAIL(e2);
    refitted.push_back(0u);
  }
  if (in.policy && quality_after_refit(r, refitted, &rebuilt) != HALA_OK) return HALA_ERR;
  return geometry_moved && !rebuilt ? configure_traversal(r) : HALA_OK;
}

// RENDER_SPEC §20, the device path of hala_rt_refit_nodes: refit_geometry's tree part when nothing but transforms changed and the kernels
// of node_batch.hip have written them — into d_instances, and into the world tree's own instance table (Blas::d_md) for the flattened
// instances of a two-level tree, so that no table is uploaded.  The refits are the ones refit_geometry runs; a refit of unmoved content
// reproduces its bytes, so running one where refit_geometry would have found nothing moved changes nothing.
// The world tree is refitted without blas_build_or_refit's uploads: everything else that function sets — the rest of Blas::d_md (material,
// addresses), d_first / d_gid / d_inst, and every field of Blas::b (tris_any, the material tables, the sub-ranges, opt) — must still be
// what its last run left.  That holds because hala_rt_refit_nodes takes the host path for every edit that changes one of them (a
// material, vertices, a deformer, build options) and a reclassification rebuilds.  A change to blas_build_or_refit has to be mirrored here.
int refit_posed_on_device(hala_rt_renderer* r, bool moved, bool world_tree_moved, bool* rebuilt) {
  *rebuilt = false;
  if (r->two_level) {
    if (r->levels.mode != 1u) RT_FAIL("internal: the instance levels are built on the host");
    std::vector<uint32_t> refitted;
    if (world_tree_moved && !r->blas.empty() && !r->blas[0]->object_space) {
      hala_rt_renderer::Blas& bl = *r->blas[0];
      const std::string e = bvh_refit(bl.b, r->stream);
      if (!e.empty()) RT_FAIL(e);
      const std::string e2 = bvh_relocate(bl.b, bl.node_off, bl.tri_off, r->stream);
      if (!e2.empty()) RT_FAIL(e2);
      refitted.push_back(0u);
    }
    if (quality_after_refit(r, refitted, rebuilt) != HALA_OK) return HALA_ERR;
    if (*rebuilt) return HALA_OK;
    if (build_instance_levels_gpu(r, false) != HALA_OK) return HALA_ERR;
    return configure_traversal(r);
  }
  const std::string e = bvh_refit(r->bvh, r->stream);
  if (!e.empty()) RT_FAIL(e);
  // (with the policy on `moved` is what refit_geometry's comparison would have found: an unmoved tree is not measured)
  if (quality_after_refit(r, moved ? std::vector<uint32_t>{0u} : std::vector<uint32_t>{}, rebuilt) != HALA_OK) return HALA_ERR;
  return *rebuilt ? HALA_OK : configure_traversal(r);
}

}  // namespace rt

extern "C" {

int hala_rt_refit(hala_rt_renderer* r) {
  RtRange range("halart::refit");
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!r->committed) RT_FAIL("The top level acceleration structure is none!");
  RT_HIP(hipStreamSynchronize(r->stream));
  // RENDER_SPEC §17 and §18: the posed vertices (and the keyed state at step 0), just ahead of the refit that reads them; then the geometry part
  if (shutter_refit(r) != HALA_OK) return HALA_ERR;
  r->invalidate(Changed::Refit);
  r->reset_accumulation();  // like the device-lost path: accumulation restarts (src/rt_renderer.rs:557)
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

}  // extern "C"
