// rig.h — the host-side evaluation of docs/RENDER_SPEC.md 19 (rig.cpp): a hala_rig_desc, a clip and a time -> the pose.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/halart.h"

namespace rt {

// a pose as hala_rig_sample_clip lays it out
struct RigPose {
  uint32_t clip = HALA_INVALID_INDEX;
  float time = 0.0f;
  std::vector<float> locals;     // node_count x 16, column-major
  std::vector<float> weights;    // hala_rig_desc::weight_floats, at hala_rig_binding::weight_first
  std::vector<float> palettes;   // hala_rig_desc::palette_floats, at hala_rig_binding::palette_first
  std::vector<uint8_t> touched;  // per node: a translation / rotation / scale channel of the clip wrote its local transform
};

// A deep copy of a description's small tables — nodes, skins, bindings without their per-vertex arrays (NULL here: the deformers hold
// them), clips — that outlives the caller's arrays (hala_rt_set_rig).
struct RigCopy {
  hala_rig_desc desc{};
  std::vector<hala_rig_node> nodes;
  std::vector<uint32_t> node_of_gltf;
  std::vector<hala_rig_skin> skins;
  std::vector<hala_rig_binding> bindings;
  std::vector<hala_rig_clip> clips;
  std::vector<std::vector<uint32_t>> u32s;
  std::vector<std::vector<float>> f32s;
  std::vector<std::vector<hala_rig_sampler>> samplers;
  std::vector<std::vector<hala_rig_channel>> channels;
  std::vector<std::string> names;
  void assign(const hala_rig_desc& g);  // (of a description rig_validate accepted)
  void clear() { *this = RigCopy(); }
};

// hala_rt_set_rig's state: the copy, the registered primitive of each binding (index into HostScene::prims), what the last
// hala_rt_pose_rig / hala_rt_key_rig recorded, and the keys hala_rt_key_rig set (to clear them again)
struct RigState {
  bool set = false;
  RigCopy copy;
  std::vector<uint32_t> prims;
  std::vector<uint64_t> deformer_ids;  // Deformer::id of what hala_rt_set_rig registered there
  RigPose pose[2];
  uint32_t poses = 0;  // 1 after hala_rt_pose_rig, 2 after hala_rt_key_rig
  std::vector<uint32_t> keyed_nodes;
  std::vector<uint8_t> posed_nodes;  // per node: a pose or a key of this rig wrote its local transform
  bool keyed_deformers = false;
  void off() { *this = RigState(); }
};

// "" or what is wrong: an index outside the array it names, a table that is NULL, a width that does not fit its path
std::string rig_validate(const hala_rig_desc* rig);
// "" or the message; checks the description's indices first, so a malformed one reads nowhere out of bounds (validated: rig_validate
// has accepted this very description already — the renderer's own copy — and the walk over it is skipped)
std::string rig_sample(const hala_rig_desc* rig, uint32_t clip, float time, RigPose* out, bool validated = false);

}  // namespace rt
