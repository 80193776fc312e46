// rt_deform.hip — deformers (docs/RENDER_SPEC.md 17; include/halart.h "Deformers"): the registry of one deformer per primitive, the
// host-side checks of tables and parameters, the launch of k_deform (deform.hip) that hala_rt_refit makes ahead of refitting the
// tree, and the read-back of a primitive's vertices.  Invariants: the primitive's range of the vertex arena holds the rest pose while
// Deformer::posed is false, and k_deform(rest, tables, Deformer::applied) otherwise; HostPrimitive::vertices stays the rest pose;
// Deformer::pending and dirty hold what the caller recorded, and posing (deform_pose) takes its parameters as arguments.
// Recomputed normals (Deformer::normals_mode 1; deform_normals.hip) are part of posing: launch_poses queues the two passes behind the
// pose launch, so the arena of a posed deformer with Deformer::normals_applied holds them too.
#include "deform_adjacency.h"
#include "renderer_state.h"

namespace rt {

// the arena's range of the primitive <- the rest pose (stream-ordered); the tree follows at the next refit
static int restore_rest(hala_rt_renderer* r, Deformer& d) {
  if (d.vertex_count)
    RT_HIP(hipMemcpyAsync(r->arena(d.prim), d.d_rest.ptr, (size_t)d.vertex_count * sizeof(hala_vertex), hipMemcpyDeviceToDevice, r->stream));
  d.posed = false; d.normals_applied = false;
  return HALA_OK;
}

static DeformTables tables_of(hala_rt_renderer* r, Deformer& d, const float* palette, uint32_t* flag) {
  DeformTables t{};
  t.rest = d.d_rest.ptr; t.out = r->arena(d.prim);
  t.dp = d.target_count ? d.d_dp.ptr : nullptr;
  t.dn = d.has_dn ? d.d_dn.ptr : nullptr;
  t.dt = d.has_dt ? d.d_dt.ptr : nullptr;
  t.joints = d.joint_count ? d.d_joints.ptr : nullptr;
  t.weights = d.d_weights.ptr; t.palette = palette;
  t.vertex_count = d.vertex_count; t.joint_count = d.joint_count;
  t.flag = flag;
  return t;
}

static NormalsTables normals_tables_of(hala_rt_renderer* r, Deformer& d) {
  NormalsTables t{};
  t.indices = r->d_indices.ptr + r->prim_index_offset[d.prim]; t.vertices = r->arena(d.prim); t.faces = d.d_faces.ptr;
  t.class_of = d.d_class_of.ptr; t.offsets = d.d_class_offsets.ptr; t.entries = d.d_class_entries.ptr;
  t.triangle_count = d.triangle_count; t.vertex_count = d.vertex_count;
  return t;
}

static size_t blocks_of(uint32_t count) { return (count + kDeformThreads - 1) / kDeformThreads; }
// the block map of one segment: (segment, first item) per 256 items of `count`, appended at blocks[*n]
static void append_blocks(DeformBlock* blocks, uint32_t* n, uint32_t segment, uint32_t count) {
  for (uint32_t first = 0; first < count; first += kDeformThreads) blocks[(*n)++] = DeformBlock{segment, first};
}

// Poses `items`, one or many, with one launch of k_deform, item k raising flags[k]; behind it the face pass and the vertex pass
// (deform_normals.hip) of the items that want them, one launch each: those in mode 1, or, where the call puts an applied pose back
// (`applied`), those whose applied pose had them.  The others are no segment of the two passes.  What the launches read — the pose
// segments, the normals segments, the block maps of the three launches, the active targets and the palettes, each section 16-B aligned —
// is laid out in DeformState::h_stage and copied to the device in one piece.  (The staged bytes stay as they are until the caller
// has synchronised: deform_pose does, inside launch_flagged before it stages the put-back and again behind the put-back.)
static int launch_poses(hala_rt_renderer* r, const std::vector<DeformPose>& items, uint32_t* flags, bool count, bool applied) {
  if (items.empty()) return HALA_OK;
  DeformState& ds = r->deform;
  auto wants_normals = [applied](const Deformer& d) {  // (no triangle: every list is empty, nothing would be written)
    return (applied ? d.normals_applied : d.normals_mode == HALA_DEFORM_NORMALS_RECOMPUTED) && d.triangle_count && d.vertex_count;
  };
  size_t normals = 0, pose_blocks = 0, face_blocks = 0, vertex_blocks = 0, actives = 0, palette_floats = 0;
  uint32_t max_joints = 0;
  for (const DeformPose& it : items) {
    pose_blocks += blocks_of(it.d->vertex_count);
    if (wants_normals(*it.d)) { ++normals; face_blocks += blocks_of(it.d->triangle_count); vertex_blocks += blocks_of(it.d->vertex_count); }
    for (float w : it.p->weights) actives += w != 0.0f;
    palette_floats += (size_t)it.d->joint_count * 12u;
    max_joints = std::max(max_joints, it.d->joint_count);
  }
  if (pose_blocks) {
    size_t total = 0;
    auto section = [&total](size_t bytes) { const size_t at = total; total = (total + bytes + 15u) & ~(size_t)15u; return at; };
    const size_t off_seg = section(items.size() * sizeof(DeformSegment)), off_nseg = section(normals * sizeof(NormalsTables)),
                 off_pose = section(pose_blocks * sizeof(DeformBlock)), off_face = section(face_blocks * sizeof(DeformBlock)),
                 off_vertex = section(vertex_blocks * sizeof(DeformBlock)), off_active = section(actives * sizeof(DeformActiveEntry)),
                 off_palette = section(palette_floats * 4u);
    ds.h_stage.assign(total, 0);
    if (total > ds.d_stage.count) RT_HIP(ds.d_stage.resize(total));
    unsigned char *h = ds.h_stage.data(), *d = ds.d_stage.ptr;
    DeformSegment* seg = reinterpret_cast<DeformSegment*>(h + off_seg);
    NormalsTables* nseg = reinterpret_cast<NormalsTables*>(h + off_nseg);
    DeformBlock *pb = reinterpret_cast<DeformBlock*>(h + off_pose), *fb = reinterpret_cast<DeformBlock*>(h + off_face), *vb = reinterpret_cast<DeformBlock*>(h + off_vertex);
    DeformActiveEntry* act = reinterpret_cast<DeformActiveEntry*>(h + off_active);
    float* pal = reinterpret_cast<float*>(h + off_palette);
    uint32_t npb = 0, nfb = 0, nvb = 0, na = 0, nn = 0;
    size_t np = 0;
    for (size_t k = 0; k < items.size(); ++k) {
      Deformer& df = *items[k].d;
      const Deformer::Params& p = *items[k].p;
      seg[k].t = tables_of(r, df, reinterpret_cast<const float*>(d + off_palette) + np, flags + k);
      seg[k].active_first = na;
      for (uint32_t t = 0; t < df.target_count; ++t)
        if (p.weights[t] != 0.0f) act[na++] = DeformActiveEntry{t, p.weights[t]};
      seg[k].active_count = na - seg[k].active_first;
      std::copy(p.palette.begin(), p.palette.begin() + (size_t)df.joint_count * 12u, pal + np);
      np += (size_t)df.joint_count * 12u;
      append_blocks(pb, &npb, (uint32_t)k, df.vertex_count);
      if (!wants_normals(df)) continue;
      nseg[nn] = normals_tables_of(r, df);
      append_blocks(fb, &nfb, nn, df.triangle_count);
      append_blocks(vb, &nvb, nn, df.vertex_count);
      ++nn;
    }
    RT_HIP(hipMemcpyAsync(d, h, total, hipMemcpyHostToDevice, r->stream));
    launch_deform(reinterpret_cast<const DeformSegment*>(d + off_seg), reinterpret_cast<const DeformBlock*>(d + off_pose),
                  reinterpret_cast<const DeformActiveEntry*>(d + off_active), npb, max_joints, r->stream);
    launch_deform_normals(reinterpret_cast<const NormalsTables*>(d + off_nseg), reinterpret_cast<const DeformBlock*>(d + off_face), nfb,
                          reinterpret_cast<const DeformBlock*>(d + off_vertex), nvb, r->stream);
    RT_HIP(hipGetLastError());
  }
  if (count) {
    ds.launches += 1; ds.batch_launches += items.size() >= 2; ds.segments += items.size();
    if (normals) ds.normals_launches += 2;
  }
  return HALA_OK;
}

// Overflow to a non-finite position: the arena is put back by running the kernel again with the last applied parameters — it is
// deterministic, and the common case pays for no spare buffer and no copy.  A HIP error between the first launch and the bookkeeping
// leaves some deformers posed on the device and none recorded as such (such errors are sticky: the device is gone).  The invariant above
// no longer holds, so every later call is refused until hala_rt_set_scene uploads the arena again: `lost` stands unless the call
// returns with the arena posed or put back.
int deform_pose(hala_rt_renderer* r, const std::vector<DeformPose>& items, std::vector<size_t>* overflowed) {
  DeformState& ds = r->deform;
  if (ds.lost) RT_FAIL("A device error interrupted an earlier deformation and the vertices on the device are undefined: set the scene again.");
  if (items.empty()) return HALA_OK;
  ds.lost = true;
  std::vector<uint32_t> flags;
  bool overflow = false;
  if (launch_flagged(ds.d_flags, items.size(), r->stream, [&](uint32_t* words) { return launch_poses(r, items, words, true, false); }, &flags, &overflow) != HALA_OK)
    return HALA_ERR;
  if (overflow) {
    std::vector<DeformPose> back;
    for (const DeformPose& it : items) {
      if (!it.d->posed) { if (restore_rest(r, *it.d) != HALA_OK) return HALA_ERR; }
      else back.push_back(DeformPose{it.d, &it.d->applied});
    }
    if (launch_poses(r, back, ds.d_flags.ptr, false, true) != HALA_OK) return HALA_ERR;
    RT_HIP(hipStreamSynchronize(r->stream));
    for (size_t k = 0; k < items.size() && overflowed; ++k)
      if (flags[k]) overflowed->push_back(k);
    ds.lost = false;
    set_last_error("Vertex position is not finite.");
    return kDeformOverflow;
  }
  for (const DeformPose& it : items) {
    it.d->applied = *it.p; it.d->posed = true;
    it.d->normals_applied = it.d->normals_mode == HALA_DEFORM_NORMALS_RECOMPUTED;
    if (!it.d->normals_applied && it.d->has_normals_tables()) it.d->release_normals_tables();  // (hipFree waits for the device)
    mark_no_history(r, it.d->prim);
  }
  ds.lost = false;
  return HALA_OK;
}

// On success nothing of the list is dirty any more; an unkeyed deformer whose pending parameters overflowed drops them, and the refit fails.
int deform_refit(hala_rt_renderer* r, const std::map<uint32_t, Deformer::Params>& keyed, const std::vector<uint32_t>& again, bool* moved) {
  std::vector<DeformPose> items;
  for (auto& kv : r->deform.by_prim) {
    auto key = keyed.find(kv.first);
    if (key != keyed.end()) items.push_back(DeformPose{kv.second.get(), &key->second});
    else if (kv.second->dirty || std::count(again.begin(), again.end(), kv.first)) items.push_back(DeformPose{kv.second.get(), &kv.second->pending});
  }
  std::vector<size_t> overflowed;
  const int e = deform_pose(r, items, &overflowed);
  for (size_t k : overflowed)
    if (!keyed.count(items[k].d->prim)) { items[k].d->pending = items[k].d->applied; items[k].d->dirty = false; }
  if (e != HALA_OK) return HALA_ERR;
  for (const DeformPose& it : items) it.d->dirty = false;
  if (!items.empty()) *moved = true;
  return HALA_OK;
}

bool deform_registered(const hala_rt_renderer* r, uint32_t prim) { return r->deform.by_prim.count(prim) != 0; }

}  // namespace rt

extern "C" {

int hala_rt_set_deformer(hala_rt_renderer* r, const hala_deformer_desc* desc) {
  if (!r || !desc) RT_FAIL("Invalid argument.");
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!r->committed) RT_FAIL("The top level acceleration structure is none!");
  uint32_t prim = 0;
  if (find_primitive(r, desc->mesh_index, desc->primitive_index, &prim) != HALA_OK) return HALA_ERR;
  if (r->shutter.rec.vertices.count(prim) || r->shutter.act.vertices.count(prim)) RT_FAIL("The primitive has shutter vertex keys: clear them and refit first (hala_rt_set_vertex_keys).");
  if (r->shutter.rec.deformers.count(prim) || r->shutter.act.deformers.count(prim)) RT_FAIL("The primitive's deformer has shutter keys: clear them and refit first (hala_rt_set_deformer_keys).");
  if (desc->target_count > kMaxMorphTargets) RT_FAIL("The deformer has more than " + std::to_string(kMaxMorphTargets) + " morph targets.");
  if (desc->joint_count > kMaxJoints) RT_FAIL("The deformer has more than " + std::to_string(kMaxJoints) + " joints.");
  if (desc->target_count == 0u && desc->joint_count == 0u) RT_FAIL("The deformer has neither morph targets nor a skin.");
  if (desc->target_count && !desc->target_position_deltas) RT_FAIL("The deformer's morph targets have no position deltas.");
  if (desc->joint_count && (!desc->joints || !desc->weights)) RT_FAIL("The deformer's skin has no joints or no weights.");
  const HostPrimitive& p = r->hs.prims[prim];
  const size_t nv = p.vertices.size(), nd = (size_t)desc->target_count * nv * 3u;
  const bool has_dn = desc->target_count && desc->target_normal_deltas, has_dt = desc->target_count && desc->target_tangent_deltas;
  if (!all_finite(desc->target_position_deltas, nd) || (has_dn && !all_finite(desc->target_normal_deltas, nd)) ||
      (has_dt && !all_finite(desc->target_tangent_deltas, nd)))
    RT_FAIL("A morph target delta is not finite.");
  if (desc->joint_count) {
    for (size_t k = 0; k < nv * 4u; ++k)
      if (desc->joints[k] >= desc->joint_count) RT_FAIL("A joint index is not below the joint count (" + std::to_string(desc->joint_count) + ").");
    if (!all_finite(desc->weights, nv * 4u)) RT_FAIL("A skin weight is not finite.");
  }
  std::unique_ptr<Deformer> d(new Deformer());
  d->id = ++r->deform.next_id;
  d->prim = prim; d->vertex_count = (uint32_t)nv; d->target_count = desc->target_count; d->joint_count = desc->joint_count;
  d->has_dn = has_dn; d->has_dt = has_dt;
  RT_HIP(d->d_rest.upload(p.vertices.data(), nv, r->stream));  // (the host copy is the rest pose: nothing but the upload reads it after commit)
  if (desc->target_count) RT_HIP(d->d_dp.upload(desc->target_position_deltas, nd, r->stream));
  if (has_dn) RT_HIP(d->d_dn.upload(desc->target_normal_deltas, nd, r->stream));
  if (has_dt) RT_HIP(d->d_dt.upload(desc->target_tangent_deltas, nd, r->stream));
  if (desc->joint_count) {
    RT_HIP(d->d_joints.upload(reinterpret_cast<const uint2*>(desc->joints), nv, r->stream));
    RT_HIP(d->d_weights.upload(reinterpret_cast<const float4*>(desc->weights), nv, r->stream));
  }
  d->applied.weights.assign(desc->target_count, 0.0f);
  d->applied.palette.assign((size_t)desc->joint_count * 12u, 0.0f);
  for (uint32_t j = 0; j < desc->joint_count; ++j) d->applied.palette[j * 12u] = d->applied.palette[j * 12u + 5u] = d->applied.palette[j * 12u + 10u] = 1.0f;
  d->pending = d->applied;
  auto old = r->deform.by_prim.find(prim);
  if (old != r->deform.by_prim.end() && old->second->posed) {  // the arena holds the old deformer's pose: back to the rest pose
    if (restore_rest(r, *d) != HALA_OK) return HALA_ERR;
    r->vertices_dirty = true;
    mark_no_history(r, prim);
  }
  RT_HIP(hipStreamSynchronize(r->stream));  // the caller's tables may go
  r->deform.by_prim[prim] = std::move(d);
  return HALA_OK;
}

int hala_rt_update_deformer(hala_rt_renderer* r, uint32_t mesh_index, uint32_t primitive_index, const float* morph_weights, uint32_t weight_count,
                            const float* joint_matrices_3x4, uint32_t joint_count) {
  if (!r) RT_FAIL("The renderer handle is null!");
  if (!r->committed) RT_FAIL("The top level acceleration structure is none!");
  uint32_t prim = 0;
  if (find_primitive(r, mesh_index, primitive_index, &prim) != HALA_OK) return HALA_ERR;
  auto it = r->deform.by_prim.find(prim);
  if (it == r->deform.by_prim.end()) RT_FAIL("The primitive has no deformer.");
  Deformer& d = *it->second;
  if (r->shutter.rec.deformers.count(prim)) RT_FAIL("The deformer has shutter keys: clear them first (hala_rt_set_deformer_keys with all keys NULL).");
  if (morph_weights && weight_count != d.target_count)
    RT_FAIL("The weight count differs from the deformer's target count (" + std::to_string(d.target_count) + ").");
  if (joint_matrices_3x4 && joint_count != d.joint_count)
    RT_FAIL("The joint count differs from the deformer's joint count (" + std::to_string(d.joint_count) + ").");
  if (morph_weights && !all_finite(morph_weights, weight_count)) RT_FAIL("A morph weight is not finite.");
  if (joint_matrices_3x4 && !all_finite(joint_matrices_3x4, (size_t)joint_count * 12u)) RT_FAIL("A joint matrix is not finite.");
  if (morph_weights) d.pending.weights.assign(morph_weights, morph_weights + weight_count);
  if (joint_matrices_3x4) d.pending.palette.assign(joint_matrices_3x4, joint_matrices_3x4 + (size_t)joint_count * 12u);
  d.dirty = d.dirty || morph_weights || joint_matrices_3x4;
  return HALA_OK;
}

int hala_rt_clear_deformer(hala_rt_renderer* r, uint32_t mesh_index, uint32_t primitive_index) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!r->committed) RT_FAIL("The top level acceleration structure is none!");
  uint32_t prim = 0;
  if (find_primitive(r, mesh_index, primitive_index, &prim) != HALA_OK) return HALA_ERR;
  auto it = r->deform.by_prim.find(prim);
  if (it == r->deform.by_prim.end()) RT_FAIL("The primitive has no deformer.");
  if (r->shutter.rec.deformers.count(prim) || r->shutter.act.deformers.count(prim)) RT_FAIL("The deformer has shutter keys: clear them and refit first (hala_rt_set_deformer_keys).");
  if (it->second->posed) {
    if (restore_rest(r, *it->second) != HALA_OK) return HALA_ERR;
    RT_HIP(hipStreamSynchronize(r->stream));  // the copy reads the tables freed below
    r->vertices_dirty = true;
    mark_no_history(r, prim);
  }
  r->deform.by_prim.erase(it);
  return HALA_OK;
}

int hala_rt_set_deformer_normals(hala_rt_renderer* r, uint32_t mesh_index, uint32_t primitive_index, uint32_t mode) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!r->committed) RT_FAIL("The top level acceleration structure is none!");
  uint32_t prim = 0;
  if (find_primitive(r, mesh_index, primitive_index, &prim) != HALA_OK) return HALA_ERR;
  auto it = r->deform.by_prim.find(prim);
  if (it == r->deform.by_prim.end()) RT_FAIL("The primitive has no deformer.");
  if (mode > HALA_DEFORM_NORMALS_RECOMPUTED) RT_FAIL("The normals mode is neither HALA_DEFORM_NORMALS_AS_POSED nor HALA_DEFORM_NORMALS_RECOMPUTED.");
  if (r->shutter.rec.deformers.count(prim) || r->shutter.act.deformers.count(prim)) RT_FAIL("The deformer has shutter keys: clear them and refit first (hala_rt_set_deformer_keys).");
  if (r->deform.lost) RT_FAIL("A device error interrupted an earlier deformation and the vertices on the device are undefined: set the scene again.");
  Deformer& d = *it->second;
  if (mode == d.normals_mode) return HALA_OK;
  if (mode == HALA_DEFORM_NORMALS_RECOMPUTED && !d.has_normals_tables()) {
    const HostPrimitive& p = r->hs.prims[prim];  // (HostPrimitive::vertices is the rest pose the deformer took)
    DeformAdjacency adj;
    if (!build_deform_adjacency(p.vertices.data(), sizeof(hala_vertex), p.vertices.size(), p.indices.data(), p.indices.size(), &adj))
      RT_FAIL("A vertex index of the primitive is not below its vertex count.");
    const size_t triangles = p.indices.size() / 3u;
    hipError_t e = d.d_class_of.upload(adj.class_of.data(), adj.class_of.size(), r->stream);
    if (e == hipSuccess) e = d.d_class_offsets.upload(adj.offsets.data(), adj.offsets.size(), r->stream);
    if (e == hipSuccess) e = d.d_class_entries.upload(adj.entries.data(), adj.entries.size(), r->stream);
    if (e == hipSuccess) e = d.d_faces.resize(triangles);
    if (e == hipSuccess) e = hipStreamSynchronize(r->stream);  // the tables above go with this scope
    if (e != hipSuccess) {
      d.release_normals_tables();
      RT_FAIL(std::string("hala_rt_set_deformer_normals: ") + hipGetErrorString(e));
    }
    d.triangle_count = (uint32_t)triangles; d.class_count = adj.class_count();
  }
  if (mode == HALA_DEFORM_NORMALS_AS_POSED && !d.normals_applied) d.release_normals_tables();  // nothing on the device was made with them
  d.normals_mode = mode;
  d.dirty = true;
  return HALA_OK;
}

int hala_rt_get_deformer_normals(hala_rt_renderer* r, uint32_t mesh_index, uint32_t primitive_index, hala_deformer_normals_info* out) {
  if (!r || !out) RT_FAIL("Invalid argument.");
  if (!r->committed) RT_FAIL("The top level acceleration structure is none!");
  uint32_t prim = 0;
  if (find_primitive(r, mesh_index, primitive_index, &prim) != HALA_OK) return HALA_ERR;
  auto it = r->deform.by_prim.find(prim);
  if (it == r->deform.by_prim.end()) RT_FAIL("The primitive has no deformer.");
  const Deformer& d = *it->second;
  const bool on = d.normals_mode == HALA_DEFORM_NORMALS_RECOMPUTED;
  out->mode = d.normals_mode; out->class_count = on ? d.class_count : 0u; out->entry_count = on ? d.triangle_count * 3u : 0u; out->reserved = 0u;
  out->launches = r->deform.normals_launches;
  return HALA_OK;
}

int hala_rt_read_vertices(hala_rt_renderer* r, uint32_t mesh_index, uint32_t primitive_index, hala_vertex* dst, uint32_t capacity, uint32_t* count) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!count) RT_FAIL("Invalid argument.");
  if (!r->committed) RT_FAIL("The top level acceleration structure is none!");
  uint32_t prim = 0;
  if (find_primitive(r, mesh_index, primitive_index, &prim) != HALA_OK) return HALA_ERR;
  const size_t nv = r->hs.prims[prim].vertices.size();
  *count = (uint32_t)nv;
  const size_t n = std::min<size_t>(capacity, nv);
  if (dst && n) {
    RT_HIP(hipMemcpyAsync(dst, r->arena(prim), n * sizeof(hala_vertex), hipMemcpyDeviceToHost, r->stream));
    RT_HIP(hipStreamSynchronize(r->stream));
  }
  return HALA_OK;
}

}  // extern "C"
