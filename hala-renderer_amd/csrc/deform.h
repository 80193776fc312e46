// deform.h — GPU-resident deformers of docs/RENDER_SPEC.md 17: morph targets and a four-influence skin per primitive, their tables on
// the device, the parameters the host records per frame, and the host side of the kernels of deform.hip and deform_normals.hip.  A call
// of the posing function (rt_deform.hip) poses any number of deformers, from one up, with one launch of each kernel: a segment per
// deformer, a map from workgroups to segments, all of it in one staged buffer that is copied once.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <memory>
#include <vector>

#include "hala_types.h"
#include "host_util.h"

namespace rt {

constexpr uint32_t kMaxMorphTargets = HALA_MAX_MORPH_TARGETS;
constexpr uint32_t kMaxJoints = HALA_MAX_JOINTS;
constexpr uint32_t kDeformThreads = 256;  // one lane per vertex

// what k_deform reads and writes of one primitive
struct DeformTables {
  const hala_vertex* rest;  // the rest pose, vertex_count records
  hala_vertex* out;         // the primitive's range of the vertex arena
  const float* dp;          // position deltas [target][vertex][3]; null: no targets
  const float* dn;          // normal deltas, same shape, or null
  const float* dt;          // tangent deltas, same shape, or null
  const uint2* joints;      // four uint16 per vertex; null: no skin
  const float4* weights;    // four floats per vertex
  const float* palette;     // joint_count row-major 3 x 4 matrices, in the staged buffer
  uint32_t vertex_count, joint_count;
  uint32_t* flag;           // the deformer's own overflow word: set to 1 when a posed position is not finite
};
// a target whose weight is not 0; a deformer's are packed in ascending order (RENDER_SPEC 17) and read with scalar loads
struct DeformActiveEntry { uint32_t index; float weight; };
struct DeformSegment {
  DeformTables t;
  uint32_t active_first, active_count;  // into the packed active-target list of the launch
};
struct DeformBlock { uint32_t segment, first_vertex; };  // 8 B per workgroup: its segment and the first of its 256 items (vertices or triangles)
static_assert(sizeof(DeformSegment) % 8 == 0 && sizeof(DeformBlock) == 8 && sizeof(DeformActiveEntry) == 8, "the staged sections are 8-byte records");

// "Recomputed normals" (RENDER_SPEC 17; deform_normals.hip): what the face pass and the vertex pass read and write of one primitive
struct NormalsTables {
  const uint32_t* indices;   // the primitive's triangles in the index arena, 3 per triangle, relative to `vertices`
  hala_vertex* vertices;     // the primitive's range of the vertex arena, as k_deform just wrote it
  float4* faces;             // one 16-B face record per triangle (x, y, z, 0): written by the face pass, read by the vertex pass
  const uint32_t* class_of;  // [vertex]
  const uint32_t* offsets;   // [class + 1] into `entries`
  const uint32_t* entries;   // triangle numbers, per class in ascending 3 * triangle + corner
  uint32_t triangle_count, vertex_count;
};
static_assert(sizeof(NormalsTables) == 56, "the staged sections are 8-byte records");

// The registered deformer of one primitive.  `applied` and `posed` say what the arena holds (kept by deform_pose, rt_deform.hip);
// `pending` and `dirty` are what the caller recorded for the next refit (written by the entry points and by that refit alone).
struct Deformer {
  uint32_t prim = 0, vertex_count = 0, target_count = 0, joint_count = 0;
  uint64_t id = 0;  // unique among the deformers of one renderer (DeformState::next_id): tells a replacement on the same primitive apart
  DeviceArray<hala_vertex> d_rest;
  DeviceArray<float> d_dp, d_dn, d_dt;
  DeviceArray<uint2> d_joints;
  DeviceArray<float4> d_weights;
  bool has_dn = false, has_dt = false;
  // Recomputed normals (hala_rt_set_deformer_normals).  normals_mode is what the caller asked for and the next pose uses;
  // normals_applied says whether the arena holds recomputed normals, which is what a put-back after an overflow reproduces.  The tables
  // exist while either is set (a switch back to mode 0 frees them once a pose without them has been applied).
  uint32_t normals_mode = 0, triangle_count = 0, class_count = 0;
  bool normals_applied = false;
  DeviceArray<uint32_t> d_class_of, d_class_offsets, d_class_entries;
  DeviceArray<float4> d_faces;
  bool has_normals_tables() const { return d_class_of.ptr != nullptr; }
  void release_normals_tables() { d_class_of.release(); d_class_offsets.release(); d_class_entries.release(); d_faces.release(); class_count = 0; }
  struct Params { std::vector<float> weights, palette; };
  Params applied, pending;
  bool dirty = false;  // `pending` was recorded since the last refit that posed it
  bool posed = false;  // the arena holds k_deform(applied) and not the rest pose as uploaded
};

struct DeformState {
  std::map<uint32_t, std::unique_ptr<Deformer>> by_prim;  // key: index into HostScene::prims
  DeviceArray<uint32_t> d_flags;                           // one overflow word per deformer of a call of deform_pose
  std::vector<unsigned char> h_stage;                      // what the launches of one call read (segments, block maps, active targets,
  DeviceArray<unsigned char> d_stage;                      // palettes) as laid out on the host, and its device copy
  uint64_t launches = 0, segments = 0;                     // launches of k_deform and deformers they posed, since hala_rt_create
  uint64_t batch_launches = 0;                             // those among them that posed two or more deformers
  uint64_t normals_launches = 0;                           // launches of the two normals kernels, since hala_rt_create
  uint64_t next_id = 0;
  bool lost = false;                                       // a device error interrupted deform_pose: the arena is undefined
  void off() { by_prim.clear(); d_flags.release(); d_stage.release(); lost = false; }
};

// k_deform, one lane per vertex, one launch on `s` for every segment: device pointers, block_count workgroups, LDS for the largest
// palette of the launch
void launch_deform(const DeformSegment* segments, const DeformBlock* blocks, const DeformActiveEntry* active, uint32_t block_count,
                   uint32_t max_joint_count, hipStream_t s);
// deform_normals.hip: the face pass and the vertex pass of every segment, two launches on `s` (face_blocks / vertex_blocks map
// workgroups to (segment, first triangle / first vertex))
void launch_deform_normals(const NormalsTables* segments, const DeformBlock* face_blocks, uint32_t face_block_count,
                           const DeformBlock* vertex_blocks, uint32_t vertex_block_count, hipStream_t s);

}  // namespace rt
