// rt_shutter.hip — shutter motion blur (docs/RENDER_SPEC.md 18; include/halart.h "Shutter"): the keys the setters record, the refit
// that applies them and leaves the scene at step 0, and the step that moves the scene to another instant of the shutter interval
// between two frames of one accumulation.  Node and deformer keys are interpolated here, on the host; vertex keys by k_shutter_lerp
// (shutter.hip).  Invariant: HostNode::local, HostScene::materials, Deformer::pending and HostPrimitive::vertices always hold what the
// caller recorded (for a keyed holder: its open key).  A refit or a step computes the state at its time beside them and hands it to
// refit_geometry (RefitInputs) and deform_pose as arguments; nothing here writes them.  ShutterState::act is what the device stands at,
// together with ShutterState::step / time.
#include "renderer_state.h"

namespace rt {

static int upload_host_copy(hala_rt_renderer* r, uint32_t prim) {
  const HostPrimitive& p = r->hs.prims[prim];
  if (!p.vertices.empty())
    RT_HIP(hipMemcpyAsync(r->arena(prim), p.vertices.data(), p.vertices.size() * sizeof(hala_vertex), hipMemcpyHostToDevice, r->stream));
  return HALA_OK;
}

// the vertex keys of `k` at `tau` into the arena (in a step: only the ones that move; *moved: some were); overflow, where asked for: some
// interpolated position is not finite (one read-back and one wait).  Only the refit asks: `b - a` does not depend on tau and the state
// lies between the keys, so keys that overflow do so at step 0 already, and a step queues its launches without waiting for them
static int lerp_vertices(hala_rt_renderer* r, const ShutterKeys& k, float tau, bool step, bool* moved, bool* overflow) {
  if (k.vertices.empty()) return HALA_OK;
  std::vector<uint32_t> flags;
  return launch_flagged(r->shutter.d_flags, k.vertices.size(), r->stream, [&](uint32_t* flag) {
    for (const auto& kv : k.vertices) {
      const ShutterVertexKeys& vk = *kv.second;
      ShutterLerp t{};
      t.flag = flag++;
      if (step && !vk.moving) continue;  // the arena holds it since the refit
      t.open = reinterpret_cast<const float*>(vk.d_open.ptr); t.close = reinterpret_cast<const float*>(vk.d_close.ptr);
      t.out = reinterpret_cast<float*>(r->arena(kv.first));
      t.words = (size_t)vk.vertex_count * (sizeof(hala_vertex) / 4);
      t.tau = tau;
      launch_shutter_lerp(t, r->stream);
      *moved = true;
    }
    RT_HIP(hipGetLastError());
    return HALA_OK;
  }, overflow ? &flags : nullptr, overflow);
}

// the arena ranges that `k` wrote, back to what they held: `prev` at `prev_tau` (the kernel again: it is deterministic, as in
// rt_deform.hip), or the host copy where `prev` has no keys for the primitive
static int restore_vertices(hala_rt_renderer* r, const ShutterKeys& k, const ShutterKeys& prev, float prev_tau) {
  ShutterKeys again;
  for (const auto& kv : k.vertices) {
    auto it = prev.vertices.find(kv.first);
    if (it != prev.vertices.end()) again.vertices[kv.first] = it->second;
    else if (upload_host_copy(r, kv.first) != HALA_OK) return HALA_ERR;
  }
  bool moved = false;
  if (lerp_vertices(r, again, prev_tau, false, &moved, nullptr) != HALA_OK) return HALA_ERR;
  RT_HIP(hipStreamSynchronize(r->stream));
  return HALA_OK;
}

static Deformer::Params mix_params(const ShutterDeformKeys& k, float tau) {
  Deformer::Params out;
  out.weights.resize(k.open.weights.size()); out.palette.resize(k.open.palette.size());
  for (size_t i = 0; i < out.weights.size(); ++i) out.weights[i] = shutter_mix(k.open.weights[i], k.close.weights[i], tau);
  for (size_t i = 0; i < out.palette.size(); ++i) out.palette[i] = shutter_mix(k.open.palette[i], k.close.palette[i], tau);
  return out;
}

// What lives on the device, at `tau`: the vertex keys, then the keyed deformers at their mix (deform_pose: k_deform as it is).  A refit
// poses every keyed deformer and what the caller recorded for the others; a step the moving keyed ones only: the deformers without keys
// wait for the refit.  *moved: the arena changed.  A position that is not finite: the arena is put back to `prev` at `prev_tau` and the
// call fails.
static int pose_device(hala_rt_renderer* r, const ShutterKeys& k, float tau, bool step, const ShutterKeys& prev, float prev_tau, bool* moved) {
  bool overflow = false;
  if (lerp_vertices(r, k, tau, step, moved, step ? nullptr : &overflow) != HALA_OK) return HALA_ERR;
  if (overflow) {
    if (restore_vertices(r, k, prev, prev_tau) != HALA_OK) return HALA_ERR;
    RT_FAIL("Vertex position is not finite.");
  }
  std::map<uint32_t, Deformer::Params> keyed;
  for (const auto& kv : k.deformers)
    if (!step || kv.second->moving) keyed[kv.first] = mix_params(*kv.second, tau);
  int e;
  if (step) {
    std::vector<DeformPose> items;
    for (const auto& kv : keyed) {
      auto d = r->deform.by_prim.find(kv.first);
      if (d != r->deform.by_prim.end()) items.push_back(DeformPose{d->second.get(), &kv.second});
    }
    e = deform_pose(r, items, nullptr);
    if (e == HALA_OK && !items.empty()) *moved = true;
  } else {
    // the refit: primitives whose vertex keys were cleared, or that hala_rt_update_vertices edited while steps were reading the arena, get
    // the host copy — ahead of k_deform, which poses over it where such a primitive has a deformer by now.  (The list is kept until the
    // refit succeeds: uploading again is harmless.)
    ShutterState& sh = r->shutter;
    std::vector<uint32_t> again;  // deformers that are posed with the recorded parameters whether or not they are dirty
    for (const auto& kv : prev.vertices) sh.stale.push_back(kv.first);
    std::sort(sh.stale.begin(), sh.stale.end());
    sh.stale.erase(std::unique(sh.stale.begin(), sh.stale.end()), sh.stale.end());
    for (uint32_t prim : sh.stale) {
      if (prim >= r->hs.prims.size() || k.vertices.count(prim)) continue;
      if (upload_host_copy(r, prim) != HALA_OK) return HALA_ERR;
      *moved = true;
      auto d = r->deform.by_prim.find(prim);  // its deformer's pose went with the range
      if (d != r->deform.by_prim.end() && d->second->posed) again.push_back(prim);
    }
    // a deformer whose keys were cleared or replaced since the last refit stands at some step's pose: the recorded pose is due
    for (const auto& kv : prev.deformers) {
      auto now = k.deformers.find(kv.first);
      if (now == k.deformers.end() || now->second != kv.second) again.push_back(kv.first);
    }
    e = deform_refit(r, keyed, again, moved);
  }
  if (e != HALA_OK) {
    const std::string msg = get_last_error();
    if (restore_vertices(r, k, prev, prev_tau) != HALA_OK) return HALA_ERR;
    RT_FAIL(msg);
  }
  return HALA_OK;
}

// `locals` with the keyed nodes at `tau`
static std::vector<Mat4> mix_node_keys(std::vector<Mat4> locals, const ShutterKeys& k, float tau) {
  for (const auto& kv : k.nodes) {
    if (kv.first >= locals.size()) continue;
    for (int i = 0; i < 16; ++i) locals[kv.first].m[i] = shutter_mix(kv.second.open[i], kv.second.close[i], tau);
  }
  return locals;
}

// hala_rt_refit's geometry part: the tree to what the caller recorded, the keyed nodes at `tau`; the recorded flags go once it stands
static int refit_recorded(hala_rt_renderer* r, const ShutterKeys& k, float tau, bool moved) {
  r->vertices_dirty = r->vertices_dirty || moved;
  if (refit_geometry(r, RefitInputs{mix_node_keys(r->hs.locals(), k, tau), r->hs.materials, r->vertices_dirty, r->materials_dirty_any, /* policy */ true}) != HALA_OK) return HALA_ERR;
  r->vertices_dirty = false; r->materials_dirty_any = false; r->nodes_dirty = false; r->materials_dirty = false; r->build_options_dirty = false;
  return HALA_OK;
}

int shutter_refit(hala_rt_renderer* r) {
  ShutterState& sh = r->shutter;
  bool moved = false;
  if (!sh.rec.any() && !sh.act.any() && sh.stale.empty()) {  // no key anywhere: the refit as it always was
    sh.act = sh.rec;
    sh.step = kShutterNoStep; sh.time = 0.0f;
    if (deform_refit(r, {}, {}, &moved) != HALA_OK) return HALA_ERR;
    return refit_recorded(r, sh.rec, 0.0f, moved);
  }
  const float tau = sh.rec.time(0);
  if (pose_device(r, sh.rec, tau, false, sh.act, sh.time, &moved) != HALA_OK) return HALA_ERR;
  sh.stale.clear();
  if (refit_recorded(r, sh.rec, tau, moved) != HALA_OK) return HALA_ERR;
  sh.act = sh.rec;
  sh.step = sh.act.any() ? 0u : kShutterNoStep;
  sh.time = tau;
  sh.locals.clear(); sh.materials.clear();
  if (sh.act.active()) {  // what a step fits to
    sh.locals = r->hs.locals();
    sh.materials = r->hs.materials;
  }
  return HALA_OK;
}

int shutter_step(hala_rt_renderer* r, uint32_t j) {
  RtRange range("halart::shutter_step");
  ShutterState& sh = r->shutter;
  if (ensure_device(r) != HALA_OK) return HALA_ERR;  // joins both frame slots: one tree is read by everything in flight
  RT_HIP(hipStreamSynchronize(r->stream));
  if (sh.locals.size() != r->hs.nodes.size()) RT_FAIL("internal: the shutter's node snapshot does not belong to the scene");
  const float tau = sh.act.time(j);
  // the edits recorded since the refit wait for the next one: the step fits to the state the refit found, and the recorded flags stay
  bool moved = false;
  if (pose_device(r, sh.act, tau, true, sh.act, sh.time, &moved) != HALA_OK) return HALA_ERR;
  if (refit_geometry(r, RefitInputs{mix_node_keys(sh.locals, sh.act, tau), sh.materials, moved, false}) != HALA_OK) return HALA_ERR;
  sh.step = j; sh.time = tau; ++sh.steps;
  return HALA_OK;
}

}  // namespace rt

extern "C" {

void hala_shutter_default_params(hala_shutter_params* out) {
  if (!out) return;
  memset(out, 0, sizeof(*out));
  out->shutter_open = 0.0f; out->shutter_close = 1.0f; out->time_stride = 1u;
}

int hala_rt_set_shutter(hala_rt_renderer* r, const hala_shutter_params* p) {
  if (!r) RT_FAIL("The renderer handle is null!");
  ShutterKeys& k = r->shutter.rec;
  if (!p) { k.on = false; k.open = 0.0f; k.close = 1.0f; k.stride = 1u; return HALA_OK; }
  if (!(p->shutter_open >= 0.0f) || !(p->shutter_close <= 1.0f) || !(p->shutter_open <= p->shutter_close))
    RT_FAIL("hala_rt_set_shutter: the shutter interval needs 0 <= shutter_open <= shutter_close <= 1.");
  if (p->time_stride < 1u || p->time_stride > kShutterMaxStride) RT_FAIL("hala_rt_set_shutter: time_stride must be in 1.." + std::to_string(kShutterMaxStride) + ".");
  for (uint32_t v : p->reserved) if (v != 0u) RT_FAIL("hala_rt_set_shutter: reserved fields must be 0.");
  if (r->temporal.enabled) RT_FAIL("hala_rt_set_shutter: the shutter is not available with temporal reprojection on (hala_rt_set_temporal(r, NULL) first).");
  if (r->adaptive.enabled) RT_FAIL("hala_rt_set_shutter: the shutter is not available with adaptive sampling on (hala_rt_set_adaptive_sampling(r, NULL) first).");
  k.on = true; k.open = p->shutter_open; k.close = p->shutter_close; k.stride = p->time_stride;
  return HALA_OK;
}

int hala_rt_get_shutter_status(hala_rt_renderer* r, hala_shutter_status* out) {
  if (!r || !out) RT_FAIL("Invalid argument.");
  const ShutterState& sh = r->shutter;
  memset(out, 0, sizeof(*out));
  out->enabled = sh.act.on ? 1u : 0u;
  out->time_stride = sh.act.stride;
  out->step = sh.step;
  out->time = sh.time;
  out->steps = sh.steps;
  return HALA_OK;
}

int hala_rt_set_node_keys(hala_rt_renderer* r, uint32_t node_index, const float open[16], const float close[16]) {
  if (!r) RT_FAIL("The renderer handle is null!");
  if (!r->committed) RT_FAIL("The top level acceleration structure is none!");
  if (node_index >= r->hs.nodes.size()) RT_FAIL("The node does not exist.");
  if ((open == nullptr) != (close == nullptr)) RT_FAIL("hala_rt_set_node_keys: both keys, or both NULL to clear them.");
  ShutterKeys& k = r->shutter.rec;
  if (!open) { k.nodes.erase(node_index); k.recount(); return HALA_OK; }
  if (!all_finite(open, 16) || !all_finite(close, 16)) RT_FAIL("A node key is not finite.");
  ShutterNodeKeys nk;
  memcpy(nk.open, open, 64); memcpy(nk.close, close, 64);
  nk.moving = memcmp(open, close, 64) != 0;
  k.nodes[node_index] = nk;
  k.recount();
  r->sync_host_mirror();  // RENDER_SPEC §20: before a local changes
  memcpy(r->hs.nodes[node_index].local.m, open, 64);
  r->nodes_dirty = true;
  return HALA_OK;
}

int hala_rt_set_deformer_keys(hala_rt_renderer* r, uint32_t mesh_index, uint32_t primitive_index, const float* weights_open, const float* weights_close,
                              uint32_t weight_count, const float* palette_open, const float* palette_close, uint32_t joint_count) {
  if (!r) RT_FAIL("The renderer handle is null!");
  if (!r->committed) RT_FAIL("The top level acceleration structure is none!");
  uint32_t prim = 0;
  if (find_primitive(r, mesh_index, primitive_index, &prim) != HALA_OK) return HALA_ERR;
  auto it = r->deform.by_prim.find(prim);
  if (it == r->deform.by_prim.end()) RT_FAIL("The primitive has no deformer.");
  Deformer& d = *it->second;
  if ((weights_open == nullptr) != (weights_close == nullptr) || (palette_open == nullptr) != (palette_close == nullptr))
    RT_FAIL("hala_rt_set_deformer_keys: both keys of a part, or both NULL.");
  ShutterKeys& k = r->shutter.rec;
  if (!weights_open && !palette_open) {
    if (k.deformers.erase(prim)) d.dirty = true;  // the open pose stays pending
    k.recount();
    return HALA_OK;
  }
  if (weights_open && weight_count != d.target_count)
    RT_FAIL("The weight count differs from the deformer's target count (" + std::to_string(d.target_count) + ").");
  if (palette_open && joint_count != d.joint_count)
    RT_FAIL("The joint count differs from the deformer's joint count (" + std::to_string(d.joint_count) + ").");
  if (weights_open && (!all_finite(weights_open, weight_count) || !all_finite(weights_close, weight_count))) RT_FAIL("A morph weight is not finite.");
  const size_t np = (size_t)joint_count * 12u;
  if (palette_open && (!all_finite(palette_open, np) || !all_finite(palette_close, np))) RT_FAIL("A joint matrix is not finite.");
  std::shared_ptr<ShutterDeformKeys> dk(new ShutterDeformKeys());
  dk->open = d.pending; dk->close = d.pending;  // a part without keys keeps the recorded pose at both ends
  if (weights_open) { dk->open.weights.assign(weights_open, weights_open + weight_count); dk->close.weights.assign(weights_close, weights_close + weight_count); }
  if (palette_open) { dk->open.palette.assign(palette_open, palette_open + np); dk->close.palette.assign(palette_close, palette_close + np); }
  dk->moving = dk->open.weights.size() * 4 && memcmp(dk->open.weights.data(), dk->close.weights.data(), dk->open.weights.size() * 4) != 0;
  dk->moving = dk->moving || (np && memcmp(dk->open.palette.data(), dk->close.palette.data(), dk->open.palette.size() * 4) != 0);
  d.pending = dk->open;
  d.dirty = true;
  k.deformers[prim] = dk;
  k.recount();
  return HALA_OK;
}

int hala_rt_set_vertex_keys(hala_rt_renderer* r, uint32_t mesh_index, uint32_t primitive_index, const hala_vertex* open, const hala_vertex* close,
                            uint32_t vertex_count) {
  if (!r) RT_FAIL("The renderer handle is null!");
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!r->committed) RT_FAIL("The top level acceleration structure is none!");
  uint32_t prim = 0;
  if (find_primitive(r, mesh_index, primitive_index, &prim) != HALA_OK) return HALA_ERR;
  if ((open == nullptr) != (close == nullptr)) RT_FAIL("hala_rt_set_vertex_keys: both keys, or both NULL to clear them.");
  ShutterState& sh = r->shutter;
  if (!open) {  // the vertices stay the open key (the host copy; the refit uploads it)
    if (sh.rec.vertices.erase(prim)) { sh.stale.push_back(prim); r->vertices_dirty = true; }
    sh.rec.recount();
    return HALA_OK;
  }
  if (deform_registered(r, prim)) RT_FAIL("The primitive has a deformer: clear it first (hala_rt_clear_deformer), or key the deformer (hala_rt_set_deformer_keys).");
  HostPrimitive& p = r->hs.prims[prim];
  if (vertex_count != p.vertices.size()) RT_FAIL("The vertex count differs from the primitive's (" + std::to_string(p.vertices.size()) + ").");
  for (const hala_vertex* key : {open, close})
    for (uint32_t v = 0; v < vertex_count; ++v)
      if (!all_finite(key[v].position, 3)) RT_FAIL("Vertex position is not finite.");
  std::shared_ptr<ShutterVertexKeys> vk(new ShutterVertexKeys());
  vk->vertex_count = vertex_count;
  vk->moving = vertex_count && memcmp(open, close, (size_t)vertex_count * sizeof(hala_vertex)) != 0;
  RT_HIP(vk->d_open.upload(open, vertex_count, r->stream));
  RT_HIP(vk->d_close.upload(close, vertex_count, r->stream));
  RT_HIP(hipStreamSynchronize(r->stream));  // the caller's arrays may go; earlier frames are done with the arena
  // as hala_rt_update_vertices(open): the host copy, and the arena unless steps are reading it
  memcpy(p.vertices.data(), open, (size_t)vertex_count * sizeof(hala_vertex));
  r->vertices_dirty = true;
  if (sh.act.active()) sh.stale.push_back(prim);
  else if (upload_host_copy(r, prim) != HALA_OK) return HALA_ERR;
  sh.rec.vertices[prim] = vk;
  sh.rec.recount();
  return HALA_OK;
}

}  // extern "C"
