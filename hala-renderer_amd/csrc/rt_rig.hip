// rt_rig.hip — rigs and clips (docs/RENDER_SPEC.md 19; include/halart.h "Rigs and clips"): a hala_rig_desc registered on the committed
// scene as one deformer per binding, and the poses of its clips handed to the entry points the host would call itself —
// hala_rt_update_node_transform / hala_rt_update_deformer (hala_rt_pose_rig), hala_rt_set_node_keys / hala_rt_set_deformer_keys
// (hala_rt_key_rig).  Nothing here touches the device: the evaluation is rig.cpp's, the posing rt_deform.hip's.
#include "renderer_state.h"

namespace rt {

static std::string binding_name(const hala_rig_binding& b) { return "mesh " + std::to_string(b.mesh_index) + " primitive " + std::to_string(b.primitive_index); }

// the deformer on binding b's primitive is the one hala_rt_set_rig registered (the host may have cleared or replaced it since)
static bool own_deformer(const hala_rt_renderer* r, size_t b) {
  auto it = r->deform.by_prim.find(r->rig.prims[b]);
  return it != r->deform.by_prim.end() && it->second->id == r->rig.deformer_ids[b];
}

// Every check a pose or a pair of keys has to pass before anything is recorded, so that a refused call changes nothing.  It covers
// each refusal of the four entry points the pose goes through: the node exists and the values are finite (rig_sample), the deformer is
// the rig's own (hence its counts fit), and no holder has keys that a plain edit would run into (`keys`: hala_rt_key_rig replaces
// keys, so those do not refuse it).
static int pose_acceptable(hala_rt_renderer* r, const RigPose& pose, bool keys) {
  const RigState& rg = r->rig;
  for (uint32_t n = 0; n < pose.touched.size(); ++n) {
    if (!pose.touched[n] && !rg.posed_nodes[n]) continue;
    if (n >= r->hs.nodes.size()) RT_FAIL("The node does not exist.");
    if (!keys && r->shutter.rec.nodes.count(n)) RT_FAIL("The node has shutter keys: clear them first (hala_rt_set_node_keys with both keys NULL).");
  }
  for (size_t b = 0; b < rg.prims.size(); ++b) {
    if (!own_deformer(r, b)) RT_FAIL("The primitive no longer has the deformer the rig registered (" + binding_name(rg.copy.bindings[b]) + ").");
    if (!keys && r->shutter.rec.deformers.count(rg.prims[b])) RT_FAIL("The deformer has shutter keys: clear them first (hala_rt_set_deformer_keys with all keys NULL).");
  }
  return HALA_OK;
}

// A pose is the whole rig's: a node that an earlier pose or pair of keys of this rig wrote and that this one does not touch goes back
// to the file's local transform (which is what `pose.locals` holds for it).
static int restore_untouched(hala_rt_renderer* r, const RigPose& pose) {
  RigState& rg = r->rig;
  for (uint32_t n = 0; n < pose.touched.size(); ++n)
    if (rg.posed_nodes[n] && !pose.touched[n] && !r->shutter.rec.nodes.count(n)) {
      if (hala_rt_update_node_transform(r, n, &pose.locals[(size_t)n * 16u]) != HALA_OK) return HALA_ERR;
      rg.posed_nodes[n] = 0;
    }
  return HALA_OK;
}

static int clear_rig_keys(hala_rt_renderer* r) {
  RigState& rg = r->rig;
  for (uint32_t n : rg.keyed_nodes)
    if (n < r->hs.nodes.size() && hala_rt_set_node_keys(r, n, nullptr, nullptr) != HALA_OK) return HALA_ERR;
  rg.keyed_nodes.clear();
  if (rg.keyed_deformers)
    for (size_t b = 0; b < rg.prims.size(); ++b) {
      const hala_rig_binding& bd = rg.copy.bindings[b];
      if (own_deformer(r, b) && hala_rt_set_deformer_keys(r, bd.mesh_index, bd.primitive_index, nullptr, nullptr, 0, nullptr, nullptr, 0) != HALA_OK)
        return HALA_ERR;
    }
  rg.keyed_deformers = false;
  return HALA_OK;
}

}  // namespace rt

extern "C" {

int hala_rt_set_rig(hala_rt_renderer* r, const hala_rig_desc* rig) {
  if (!r) RT_FAIL("The renderer handle is null!");
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!r->committed) RT_FAIL("The top level acceleration structure is none!");
  RigState& rg = r->rig;
  if (!rig) {
    if (!rg.set) return HALA_OK;
    for (size_t b = 0; b < rg.prims.size(); ++b)  // (what hala_rt_clear_deformer would refuse, found before anything changes)
      if (own_deformer(r, b) && (r->shutter.rec.deformers.count(rg.prims[b]) || r->shutter.act.deformers.count(rg.prims[b])))
        RT_FAIL("A deformer of the rig has shutter keys: clear them and refit first (hala_rt_key_rig with HALA_INVALID_INDEX).");
    if (clear_rig_keys(r) != HALA_OK) return HALA_ERR;
    r->sync_host_mirror();  // RENDER_SPEC §20: before a local changes
    r->nodes_dirty = true;
    for (uint32_t n = 0; n < rg.posed_nodes.size(); ++n)  // the nodes the rig's poses moved: back to the file's transforms
      if (rg.posed_nodes[n] && n < r->hs.nodes.size() && !r->shutter.rec.nodes.count(n)) memcpy(r->hs.nodes[n].local.m, rg.copy.nodes[n].local_transform, 64);
    for (size_t b = 0; b < rg.prims.size(); ++b)  // the deformers the rig registered; one the host put there since is the host's
      if (own_deformer(r, b) && hala_rt_clear_deformer(r, rg.copy.bindings[b].mesh_index, rg.copy.bindings[b].primitive_index) != HALA_OK) return HALA_ERR;
    rg.off();
    return HALA_OK;
  }
  if (rg.set) RT_FAIL("A rig is set: clear it first (hala_rt_set_rig with NULL).");
  const std::string bad = rig_validate(rig);
  if (!bad.empty()) RT_FAIL(bad);
  if (rig->node_count != r->hs.nodes.size()) RT_FAIL("The rig has " + std::to_string(rig->node_count) + " nodes and the committed scene " + std::to_string(r->hs.nodes.size()) + ".");
  for (uint32_t n = 0; n < rig->node_count; ++n)
    if (rig->nodes[n].parent != r->hs.nodes[n].parent) RT_FAIL("Node " + std::to_string(n) + " of the rig has another parent than the committed scene's.");
  std::vector<uint32_t> prims;
  for (uint32_t k = 0; k < rig->binding_count; ++k) {
    const hala_rig_binding& b = rig->bindings[k];
    const std::string name = binding_name(b);
    uint32_t prim = 0;
    if (find_primitive(r, b.mesh_index, b.primitive_index, &prim) != HALA_OK) RT_FAIL(std::string(get_last_error()) + " (" + name + ")");
    uint32_t instances = 0;
    for (const HostNode& n : r->hs.nodes) instances += n.mesh_index == b.mesh_index ? 1u : 0u;
    if (instances != 1u || b.node_count != 1u)
      RT_FAIL("Mesh " + std::to_string(b.mesh_index) + " is instantiated by " + std::to_string(std::max(instances, b.node_count)) + " nodes: a rig poses a primitive once, not per instance (" + name + ").");
    if (r->hs.nodes[b.node].mesh_index != b.mesh_index) RT_FAIL("Node " + std::to_string(b.node) + " does not instantiate the mesh of the binding (" + name + ").");
    if (b.vertex_count != r->hs.prims[prim].vertices.size()) RT_FAIL("The vertex count differs from the primitive's (" + name + ").");
    const uint32_t joints = b.skin == HALA_INVALID_INDEX ? 0u : rig->skins[b.skin].joint_count;
    if (joints > kMaxJoints) RT_FAIL("The skin of " + name + " has more than " + std::to_string(kMaxJoints) + " joints.");
    if (b.target_count > kMaxMorphTargets) RT_FAIL(name + " has more than " + std::to_string(kMaxMorphTargets) + " morph targets.");
    if (!joints && !b.target_count) RT_FAIL(name + " has neither morph targets nor a skin.");
    if ((joints && (!b.joints || !b.weights)) || (b.target_count && !b.target_position_deltas)) RT_FAIL("A table of " + name + " is NULL.");
    if (deform_registered(r, prim)) RT_FAIL("The primitive already has a deformer (" + name + ").");
    if (r->shutter.rec.vertices.count(prim) || r->shutter.act.vertices.count(prim)) RT_FAIL("The primitive has shutter vertex keys (" + name + ").");
    for (uint32_t p : prims) if (p == prim) RT_FAIL("Two bindings name " + name + ".");
    prims.push_back(prim);
  }
  for (uint32_t k = 0; k < rig->binding_count; ++k) {
    const hala_rig_binding& b = rig->bindings[k];
    hala_deformer_desc d{};
    d.mesh_index = b.mesh_index; d.primitive_index = b.primitive_index;
    d.target_count = b.target_count;
    d.target_position_deltas = b.target_position_deltas; d.target_normal_deltas = b.target_normal_deltas; d.target_tangent_deltas = b.target_tangent_deltas;
    d.joint_count = b.skin == HALA_INVALID_INDEX ? 0u : rig->skins[b.skin].joint_count;
    d.joints = b.joints; d.weights = b.weights;
    if (hala_rt_set_deformer(r, &d) != HALA_OK) {  // (a table entry that is not finite, a joint index too high): take back what was registered
      const std::string msg = std::string(get_last_error()) + " (" + binding_name(b) + ")";
      for (uint32_t u = 0; u < k; ++u) (void)hala_rt_clear_deformer(r, rig->bindings[u].mesh_index, rig->bindings[u].primitive_index);
      RT_FAIL(msg);
    }
  }
  rg.copy.assign(*rig);
  rg.prims = prims;
  rg.deformer_ids.clear();
  for (uint32_t prim : prims) rg.deformer_ids.push_back(r->deform.by_prim[prim]->id);
  rg.posed_nodes.assign(rig->node_count, 0);
  rg.set = true;
  return HALA_OK;
}

int hala_rt_pose_rig(hala_rt_renderer* r, uint32_t clip, float time) {
  if (!r) RT_FAIL("The renderer handle is null!");
  if (!r->committed) RT_FAIL("The top level acceleration structure is none!");
  RigState& rg = r->rig;
  if (!rg.set) RT_FAIL("No rig is set (hala_rt_set_rig).");
  RigPose pose;
  const std::string e = rig_sample(&rg.copy.desc, clip, time, &pose, /*validated*/ true);
  if (!e.empty()) RT_FAIL(e);
  if (pose_acceptable(r, pose, false) != HALA_OK) return HALA_ERR;
  if (restore_untouched(r, pose) != HALA_OK) return HALA_ERR;
  for (uint32_t n = 0; n < pose.touched.size(); ++n) {
    if (!pose.touched[n]) continue;
    if (hala_rt_update_node_transform(r, n, &pose.locals[(size_t)n * 16u]) != HALA_OK) return HALA_ERR;
    rg.posed_nodes[n] = 1;
  }
  for (size_t b = 0; b < rg.prims.size(); ++b) {
    const hala_rig_binding& bd = rg.copy.bindings[b];
    const uint32_t joints = bd.skin == HALA_INVALID_INDEX ? 0u : rg.copy.skins[bd.skin].joint_count;
    if (hala_rt_update_deformer(r, bd.mesh_index, bd.primitive_index, bd.target_count ? &pose.weights[bd.weight_first] : nullptr, bd.target_count,
                                joints ? &pose.palettes[bd.palette_first] : nullptr, joints) != HALA_OK)
      return HALA_ERR;
  }
  rg.pose[0] = std::move(pose);
  rg.poses = 1;
  return HALA_OK;
}

int hala_rt_key_rig(hala_rt_renderer* r, uint32_t clip, float t_open, float t_close) {
  if (!r) RT_FAIL("The renderer handle is null!");
  if (!r->committed) RT_FAIL("The top level acceleration structure is none!");
  RigState& rg = r->rig;
  if (!rg.set) RT_FAIL("No rig is set (hala_rt_set_rig).");
  if (clip == HALA_INVALID_INDEX) return clear_rig_keys(r);
  RigPose open, close;
  std::string e = rig_sample(&rg.copy.desc, clip, t_open, &open, /*validated*/ true);
  if (e.empty()) e = rig_sample(&rg.copy.desc, clip, t_close, &close, /*validated*/ true);
  if (!e.empty()) RT_FAIL(e);
  if (pose_acceptable(r, open, true) != HALA_OK) return HALA_ERR;
  if (clear_rig_keys(r) != HALA_OK) return HALA_ERR;  // the keys of an earlier call
  if (restore_untouched(r, open) != HALA_OK) return HALA_ERR;
  for (uint32_t n = 0; n < open.touched.size(); ++n) {
    if (!open.touched[n]) continue;
    if (hala_rt_set_node_keys(r, n, &open.locals[(size_t)n * 16u], &close.locals[(size_t)n * 16u]) != HALA_OK) return HALA_ERR;
    rg.keyed_nodes.push_back(n);
    rg.posed_nodes[n] = 1;
  }
  for (size_t b = 0; b < rg.prims.size(); ++b) {
    const hala_rig_binding& bd = rg.copy.bindings[b];
    const uint32_t joints = bd.skin == HALA_INVALID_INDEX ? 0u : rg.copy.skins[bd.skin].joint_count;
    rg.keyed_deformers = true;
    if (hala_rt_set_deformer_keys(r, bd.mesh_index, bd.primitive_index, bd.target_count ? &open.weights[bd.weight_first] : nullptr,
                                  bd.target_count ? &close.weights[bd.weight_first] : nullptr, bd.target_count, joints ? &open.palettes[bd.palette_first] : nullptr,
                                  joints ? &close.palettes[bd.palette_first] : nullptr, joints) != HALA_OK)
      return HALA_ERR;
  }
  rg.pose[0] = std::move(open); rg.pose[1] = std::move(close);
  rg.poses = 2;
  return HALA_OK;
}

int hala_rt_get_rig_pose(hala_rt_renderer* r, uint32_t key, uint32_t* clip, float* time, float* locals, float* weights, float* palettes) {
  if (!r) RT_FAIL("The renderer handle is null!");
  const RigState& rg = r->rig;
  if (!rg.set) RT_FAIL("No rig is set (hala_rt_set_rig).");
  if (key >= rg.poses) RT_FAIL(rg.poses ? "The last call recorded no second pose (hala_rt_key_rig records two)." : "No pose has been recorded (hala_rt_pose_rig, hala_rt_key_rig).");
  const RigPose& p = rg.pose[key];
  if (clip) *clip = p.clip;
  if (time) *time = p.time;
  if (locals && !p.locals.empty()) memcpy(locals, p.locals.data(), p.locals.size() * 4u);
  if (weights && !p.weights.empty()) memcpy(weights, p.weights.data(), p.weights.size() * 4u);
  if (palettes && !p.palettes.empty()) memcpy(palettes, p.palettes.data(), p.palettes.size() * 4u);
  return HALA_OK;
}

int hala_rt_get_rig_status(hala_rt_renderer* r, hala_rig_status* out) {
  if (!r || !out) RT_FAIL("Invalid argument.");
  memset(out, 0, sizeof(*out));
  out->bindings = r->rig.set ? (uint32_t)r->rig.prims.size() : 0u;
  out->deformers = (uint32_t)r->deform.by_prim.size();
  out->pose_launches = r->deform.launches;
  out->batch_launches = r->deform.batch_launches;
  out->segments_posed = r->deform.segments;
  return HALA_OK;
}

}  // extern "C"
