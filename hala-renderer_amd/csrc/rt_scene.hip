// rt_scene.hip — the scene on the device: the packed records, the textures and their bundles (BundleState), the edit and refit API up
// to the list of trees a refit moved (rt_trees.hip takes it from there), and the introspection of the textures.
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

}  // namespace rt

extern "C" {

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
  const bool had_invisible = r->any_invisible;
  const std::vector<uint8_t> classes_before = r->material_any_class;
  if (attach_any_triangles(r) != HALA_OK) return HALA_ERR;
  // (a material edit can change which triangles the shadow rays see: their copy is rewritten by the refit pass)
  // (the BVH-order triangles carry their material's shading kind: rewritten by the refit pass as well)
  // what the trees hold changed: vertices or materials (the any-hit copy of the triangles must be rewritten when a class changed)
  const bool content = in.arena_changed || in.opacity0_edit || classes_before != r->material_any_class || had_invisible != r->any_invisible ||
                       kinds_before != r->material_kind || before.size() != r->hs.instances.size();
  // which instances are intersected in object space may have changed (a transform that is no longer invertible, or is again): rebuild
  std::vector<uint8_t> flags;
  classify_instances(r, &flags);
  if (flags != r->inst_instanced) return build_bvh(r);
  // The trees that moved: those whose content changed (any tree) or that hold an instance whose transform did (a world tree; the tree of
  // a one-level scene holds every instance).  A node that moves an instanced primitive, a camera or a light moves no tree
  std::vector<uint32_t> moved;
  for (size_t k = 0; k < r->trees.size(); ++k) {
    bool m = content;
    if (!r->trees[k]->object_space)
      for (uint32_t i : r->trees[k]->insts) m = m || memcmp(before[i].transform, r->hs.instances[i].transform, 64) != 0;
    if (m) moved.push_back((uint32_t)k);
  }
  bool rebuilt = false;
  return refit_trees(r, moved, false, in.policy, &rebuilt);
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

}  // extern "C"
