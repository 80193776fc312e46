// rt_nodes.hip — node batches (docs/RENDER_SPEC.md 20; include/halart.h "Node batches"): a set of nodes bound once and posed from one
// array of local transforms per frame, in host or device memory.  hala_rt_refit_nodes leaves the renderer where
// hala_rt_update_node_transform per bound node + hala_rt_refit would: on the device path the kernels of node_batch.hip compute the
// hierarchy and the instance transforms and the one refit sequence runs on them (refit_trees, published); whenever that cannot guarantee the
// same state the call writes the locals into the host scene and runs hala_rt_refit's own code (the host path), and says why in the status.
#include "renderer_state.h"

namespace rt {

enum : uint32_t { kPathNone = 0, kPathDevice = 1, kPathHost = 2 };

// The bind-time analysis, from the committed scene and the trees as they stand: the affected nodes (the bound ones and everything below
// them) grouped by their depth within the affected set, the affected instances with what the classification expects of them, and whether
// a camera or a light rides along.  Uploaded once; build_bvh makes it stale (NodeBatchState::analysed).
static int analyse(hala_rt_renderer* r) {
  NodeBatchState& nb = r->nodes;
  const HostScene& hs = r->hs;
  const size_t nn = hs.nodes.size();
  std::vector<int32_t> level(nn, -1);
  for (uint32_t n : nb.bound) level[n] = 0;
  uint32_t levels = 0;
  nb.affected_nodes = 0; nb.moves_camera_or_light = false;
  for (size_t k = 0; k < nn; ++k) {  // parents come before their children (HostScene::assign)
    const int32_t p = hs.nodes[k].parent;
    if (p >= 0 && level[(size_t)p] >= 0) level[k] = level[(size_t)p] + 1;
    if (level[k] < 0) continue;
    ++nb.affected_nodes;
    levels = std::max(levels, (uint32_t)level[k] + 1u);
    nb.moves_camera_or_light = nb.moves_camera_or_light || hs.nodes[k].camera_index != HALA_INVALID_INDEX || hs.nodes[k].light_index != HALA_INVALID_INDEX;
  }
  nb.level_first.assign(levels + 1u, 0u);
  for (size_t k = 0; k < nn; ++k) if (level[k] >= 0) nb.level_first[(size_t)level[k] + 1u]++;
  for (uint32_t l = 0; l < levels; ++l) nb.level_first[l + 1u] += nb.level_first[l];
  std::vector<NodeBatchNode> entries(nb.affected_nodes);
  std::vector<uint32_t> at(nb.level_first.begin(), nb.level_first.end() - 1);
  for (size_t k = 0; k < nn; ++k) if (level[k] >= 0) entries[at[(size_t)level[k]]++] = NodeBatchNode{(uint32_t)k, hs.nodes[k].parent};
  // the instances of the affected nodes
  std::vector<uint8_t> considered;
  instancing_candidates(r, &considered);
  std::vector<uint32_t> md_slot(hs.instances.size(), kAbsent);
  if (const hala_rt_renderer::Tree* w = r->world_tree())
    for (size_t k = 0; k < w->insts.size(); ++k) md_slot[w->insts[k]] = (uint32_t)k;
  std::vector<NodeBatchInst> insts;
  nb.moves_flattened = false;
  for (size_t i = 0; i < hs.instances.size(); ++i) {
    if (level[hs.instance_node[i]] < 0) continue;
    const uint32_t instanced = i < r->inst_instanced.size() && r->inst_instanced[i] ? 1u : 0u;
    insts.push_back(NodeBatchInst{(uint32_t)i, hs.instance_node[i], (considered[i] ? 1u : 0u) | (instanced << 1), md_slot[i]});
    nb.moves_flattened = nb.moves_flattened || md_slot[i] != kAbsent;
  }
  nb.affected_instances = (uint32_t)insts.size();
  RT_HIP(nb.d_bound.upload(nb.bound.data(), nb.bound.size(), r->stream));
  RT_HIP(nb.d_levels.upload(entries.data(), entries.size(), r->stream));
  RT_HIP(nb.d_insts.upload(insts.data(), insts.size(), r->stream));
  RT_HIP(nb.d_mismatch.resize(1));
  RT_HIP(nb.d_in.resize(nb.bound.size() * 16u));
  RT_HIP(nb.d_locals.resize(nn * 16u));
  RT_HIP(nb.d_worlds.resize(nn * 16u));
  if (!nb.h_stage) RT_HIP(hipHostMalloc(reinterpret_cast<void**>(&nb.h_stage), nb.bound.size() * 64u, hipHostMallocDefault));
  if (!nb.h_word) RT_HIP(hipHostMalloc(reinterpret_cast<void**>(&nb.h_word), 4, hipHostMallocDefault));
  RT_HIP(hipStreamSynchronize(r->stream));  // the vectors above go out of scope
  nb.analysed = true;
  return HALA_OK;
}

// why the device path cannot guarantee the state of the ordinary sequence (0: it can)
static uint32_t host_reason(const hala_rt_renderer* r) {
  const ShutterState& sh = r->shutter;  // (first: setting a key is an edit too, and this is the reason that tells more)
  if (sh.rec.any() || sh.act.any() || !sh.stale.empty()) return HALA_NODE_REFIT_SHUTTER_KEYS;
  bool pending = r->nodes_dirty || r->materials_dirty || r->materials_dirty_any || r->vertices_dirty || r->build_options_dirty;
  for (const auto& kv : r->deform.by_prim) pending = pending || kv.second->dirty;
  if (pending) return HALA_NODE_REFIT_PENDING_EDIT;
  if (r->nodes.moves_camera_or_light) return HALA_NODE_REFIT_CAMERA_OR_LIGHT;
  if (r->two_level && r->levels.mode != 1u) return HALA_NODE_REFIT_HOST_LEVELS;
  return 0u;
}

static void restart(hala_rt_renderer* r, uint32_t path, uint32_t reason) {  // the end of hala_rt_refit
  r->invalidate(Changed::Refit);
  r->reset_accumulation();
  NodeBatchState& nb = r->nodes;
  nb.last_path = path; nb.last_reason = reason;
  if (path == kPathDevice) ++nb.device_refits; else ++nb.host_refits;
}

// hala_rt_update_node_transform per bound node, then hala_rt_refit (behind its join and its wait, which the caller has done)
static int host_path(hala_rt_renderer* r, const float* locals, uint32_t reason) {
  NodeBatchState& nb = r->nodes;
  r->sync_host_mirror();  // from the locals the trees stand at, before they change
  for (size_t k = 0; k < nb.bound.size(); ++k) memcpy(r->hs.nodes[nb.bound[k]].local.m, locals + 16u * k, 64);
  r->nodes_dirty = true;
  if (shutter_refit(r) != HALA_OK) return HALA_ERR;
  restart(r, kPathHost, reason);
  return HALA_OK;
}

}  // namespace rt

extern "C" {

int hala_rt_bind_nodes(hala_rt_renderer* r, const uint32_t* node_indices, uint32_t count) {
  if (!r) RT_FAIL("The renderer handle is null!");
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!r->committed) RT_FAIL("The top level acceleration structure is none!");
  if (count && !node_indices) RT_FAIL("Invalid argument.");
  std::vector<uint8_t> seen(r->hs.nodes.size(), 0);
  for (uint32_t k = 0; k < count; ++k) {  // everything is checked before anything changes: a refused call leaves the binding as it was
    const uint32_t n = node_indices[k];
    if (n >= r->hs.nodes.size()) RT_FAIL("The node does not exist.");
    if (seen[n]) RT_FAIL("hala_rt_bind_nodes: node " + std::to_string(n) + " is given twice.");
    if (r->shutter.rec.nodes.count(n)) RT_FAIL("The node has shutter keys: clear them first (hala_rt_set_node_keys with both keys NULL).");
    seen[n] = 1;
  }
  RT_HIP(hipStreamSynchronize(r->stream));  // a kernel of the last call may still read the tables
  r->sync_host_mirror();
  r->nodes.release();
  if (!count) return HALA_OK;
  r->nodes.bound.assign(node_indices, node_indices + count);
  if (analyse(r) != HALA_OK) { r->nodes.release(); return HALA_ERR; }
  return HALA_OK;
}

int hala_rt_refit_nodes(hala_rt_renderer* r, const float* locals, int where) {
  RtRange range("halart::refit_nodes");
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!r->committed) RT_FAIL("The top level acceleration structure is none!");
  NodeBatchState& nb = r->nodes;
  if (nb.bound.empty()) RT_FAIL("hala_rt_refit_nodes: no nodes are bound (hala_rt_bind_nodes).");
  if (!locals || (where != 0 && where != 1)) RT_FAIL("Invalid argument.");
  for (uint32_t n : nb.bound)
    if (r->shutter.rec.nodes.count(n)) RT_FAIL("The node has shutter keys: clear them first (hala_rt_set_node_keys with both keys NULL).");
  RT_HIP(hipStreamSynchronize(r->stream));
  if (!nb.analysed && analyse(r) != HALA_OK) return HALA_ERR;  // a refit rebuilt the trees since the bind
  const uint32_t count = (uint32_t)nb.bound.size(), node_count = (uint32_t)r->hs.nodes.size();
  const size_t bytes = (size_t)count * 64u;
  const uint32_t reason = host_reason(r);
  if (reason) {
    if (where == 1) {
      RT_HIP(hipMemcpyAsync(nb.h_stage, locals, bytes, hipMemcpyDeviceToHost, r->stream));
      RT_HIP(hipStreamSynchronize(r->stream));
    }
    return host_path(r, where == 1 ? nb.h_stage : locals, reason);
  }
  // ---- the device path ----
  if (!nb.tables_current) {  // a host refit moved the transforms since: the tables of all locals and worlds again, from the (current) host copy
    r->sync_host_mirror();
    std::vector<float> tab((size_t)node_count * 32u);
    for (uint32_t k = 0; k < node_count; ++k) {
      memcpy(&tab[(size_t)k * 16u], r->hs.nodes[k].local.m, 64);
      memcpy(&tab[((size_t)node_count + k) * 16u], r->hs.nodes[k].world.m, 64);
    }
    RT_HIP(hipMemcpyAsync(nb.d_locals.ptr, tab.data(), (size_t)node_count * 64u, hipMemcpyHostToDevice, r->stream));
    RT_HIP(hipMemcpyAsync(nb.d_worlds.ptr, tab.data() + (size_t)node_count * 16u, (size_t)node_count * 64u, hipMemcpyHostToDevice, r->stream));
    RT_HIP(hipStreamSynchronize(r->stream));  // `tab` goes out of scope
    nb.tables_current = true;
  }
  const float* d_in = locals;
  if (where == 0) {
    memcpy(nb.h_stage, locals, bytes);
    RT_HIP(hipMemcpyAsync(nb.d_in.ptr, nb.h_stage, bytes, hipMemcpyHostToDevice, r->stream));
    d_in = nb.d_in.ptr;
  } else {  // the host's copy of the locals follows the caller's array; awaited with the look below
    RT_HIP(hipMemcpyAsync(nb.h_stage, locals, bytes, hipMemcpyDeviceToHost, r->stream));
  }
  RT_HIP(hipMemsetAsync(nb.d_mismatch.ptr, 0, 4, r->stream));
  launch_node_locals(d_in, nb.d_bound.ptr, count, nb.d_locals.ptr, node_count, r->stream);
  for (uint32_t l = 0; l < nb.levels(); ++l)
    launch_node_worlds(nb.d_levels.ptr + nb.level_first[l], nb.level_first[l + 1u] - nb.level_first[l], nb.d_locals.ptr, nb.d_worlds.ptr, node_count, r->stream);
  const hala_rt_renderer::Tree* w = r->world_tree();
  const bool policy = r->quality.mode != HALA_REFIT_POLICY_OFF;
  launch_instance_transforms(nb.d_insts.ptr, nb.affected_instances, nb.d_worlds.ptr, node_count, r->d_instances.ptr, (uint32_t)r->d_instances.count,
                             w ? w->d_md.ptr : nullptr, w ? (uint32_t)w->d_md.count : 0u, nb.d_mismatch.ptr, policy, r->stream);
  RT_HIP(hipGetLastError());
  // the one look, before anything is built on the new transforms
  RT_HIP(hipMemcpyAsync(nb.h_word, nb.d_mismatch.ptr, 4, hipMemcpyDeviceToHost, r->stream));
  RT_HIP(hipStreamSynchronize(r->stream));
  if (*nb.h_word & kNodeBatchMismatch) return host_path(r, nb.h_stage, HALA_NODE_REFIT_CLASSIFICATION);  // (refit_geometry publishes every instance record again)
  for (uint32_t k = 0; k < count; ++k) memcpy(r->hs.nodes[nb.bound[k]].local.m, nb.h_stage + 16u * (size_t)k, 64);
  nb.mirror_stale = true;
  {  // what hala_rt_refit does when no key is anywhere (shutter_refit)
    ShutterState& sh = r->shutter;
    sh.act = sh.rec;
    sh.step = kShutterNoStep; sh.time = 0.0f;
  }
  // The tree that holds flattened instances, [0], moved if one of them did.  RENDER_SPEC 4.6: with a policy the kernels have compared the
  // transforms as the ordinary sequence would, so the refit fits and measures what that one would, and builds anew when that is due — the
  // ordinary sequence's end, reported as the host path with its own reason.  Without one the bind-time analysis answers: an affected
  // instance lies in the tree (in a one-level tree: always; a refit of unmoved content reproduces its bytes)
  const uint32_t moved_bit = r->two_level ? kNodeBatchMovedWorldTree : kNodeBatchMoved;
  std::vector<uint32_t> moved;
  if (policy ? (*nb.h_word & moved_bit) != 0u : (!r->two_level || nb.moves_flattened)) moved.push_back(0u);
  bool rebuilt = false;
  if (refit_trees(r, moved, true, true, &rebuilt) != HALA_OK) return HALA_ERR;
  if (rebuilt) restart(r, kPathHost, HALA_NODE_REFIT_POLICY_REBUILD);
  else restart(r, kPathDevice, 0u);
  return HALA_OK;
}

int hala_rt_get_node_refit_status(hala_rt_renderer* r, hala_node_refit_status* out) {
  if (!r || !out) RT_FAIL("Invalid argument.");
  const NodeBatchState& nb = r->nodes;
  memset(out, 0, sizeof(*out));
  out->bound_nodes = (uint32_t)nb.bound.size();
  if (!nb.bound.empty()) { out->affected_nodes = nb.affected_nodes; out->affected_instances = nb.affected_instances; out->levels = nb.levels(); }
  out->last_path = nb.last_path; out->last_reason = nb.last_reason;
  out->device_refits = nb.device_refits; out->host_refits = nb.host_refits;
  return HALA_OK;
}

}  // extern "C"
