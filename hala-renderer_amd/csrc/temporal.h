// temporal.h — temporal reprojection of docs/RENDER_SPEC.md 16: the history a capture keeps, the table a resolve reads and the host
// side of its launch (temporal.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "hala_types.h"
#include "host_util.h"

namespace rt {

// what the projection of RENDER_SPEC 16 reads of a packed camera (hala_gpu_camera without its padding), 64 B
struct TemporalCamera {
  float position[3]; float tan_half;
  float right[3];    float xmag;
  float up[3];       float ymag;
  float forward[3];  uint32_t type;  // 0 perspective, 1 orthographic
};

// The table of one resolve, in device memory behind one pointer: this head, then one TemporalInst per instance, then one mark word per
// material.  Every lane of a wave reads the same head (scalar loads) and the record of its own pixel's instance.
struct TemporalHead {
  TemporalCamera prev, cur;  // the captured camera and view 0's camera now
  float width, height, aspect, max_history;
  float tol, min_weight;
  uint32_t inst_count, mat_count;
};
struct TemporalInst {
  float d[12];      // D = W_prev . W_cur^-1, rows of a 3 x 4 matrix
  uint32_t marked;  // 0 rigid motion by d; 1 no history (W_cur singular, or vertices edited and not followed); 2 vertex motion
  uint32_t pad[3];
};
static_assert(sizeof(TemporalCamera) == 64 && sizeof(TemporalHead) == 160 && sizeof(TemporalInst) == 64, "the table is read as 16-B quads");

struct TemporalState {
  bool enabled = false;
  hala_temporal_params p{};
  // the history (RENDER_SPEC 16 "State"); row-major W x H
  bool has_history = false;
  DeviceArray<float4> hc, hp, hi;
  hala_gpu_camera cam{};
  float tan_half = 0.0f;
  std::vector<float> world;  // 16 floats per instance, column-major object -> world, as captured
  // edited since the capture (hala_rt_update_vertices / hala_rt_update_material)
  std::vector<uint8_t> inst_marked, mat_marked;
  // RENDER_SPEC 16 "Vertex motion" (hala_rt_set_temporal_vertex_motion): tris_by_id of a one-level tree as the last capture found it.
  // Allocated by the first capture with the feature on; a history captured with it off has none.
  bool vertex_motion = false, has_snapshot = false;
  DeviceArray<Tri> snapshot;
  // RENDER_SPEC 16 "History clamp" (hala_rt_set_temporal_clamp): two launch arguments of the resolve, no state on the device
  bool clamp = false;
  hala_temporal_clamp_params cp{};
  // the outputs of the last resolve: temporal, motion
  DeviceArray<float4> out[2];
  bool resolved = false;
  // The table on the device.  A resolve rebuilds it (one 3 x 3 inverse in double per instance) and uploads it only while table_dirty:
  // set by whatever changes an input of it — a capture, a refit (instance transforms, view 0's camera), a mark, new parameters, another
  // view list, a dropped history.  Every other resolve launches straight away.
  DeviceArray<uint32_t> table;
  bool table_dirty = true;
  bool table_vertex = false;  // some instance of the table carries mark 2: the resolve launches the vertex-motion instantiation

  void drop_snapshot() { has_snapshot = false; table_dirty = true; snapshot.release(); }
  void drop_history() {
    has_history = false; drop_snapshot();
    std::fill(inst_marked.begin(), inst_marked.end(), 0); std::fill(mat_marked.begin(), mat_marked.end(), 0);
  }
  void release() {
    enabled = false; has_history = false; resolved = false; vertex_motion = false; clamp = false; drop_snapshot();
    for (DeviceArray<float4>* a : {&hc, &hp, &hi, &out[0], &out[1]}) a->release();
    table.release(); world.clear(); inst_marked.clear(); mat_marked.clear();
  }
};

// "" or the reason the parameters are refused (no device call)
std::string temporal_check_params(const hala_temporal_params* p);
std::string temporal_check_clamp_params(const hala_temporal_clamp_params* p);

// D = W_prev . W_cur^-1 in double, rounded once (RENDER_SPEC 16 "Motion of an instance"); w_prev / w_cur: 16 floats, column-major.
// Returns false when W_cur is singular (d is then the identity).
bool temporal_motion(const float* w_prev, const float* w_cur, float d[12]);

TemporalCamera temporal_camera(const hala_gpu_camera& c, float tan_half);

// one thread per pixel of the row-major w x h frame; table: TemporalHead, TemporalInst x inst_count, mark words x mat_count.
// tris / snap: tri_count triangles in id order, now and as captured, when an instance of the table carries mark 2; else null.
// clamp: the checked parameters of RENDER_SPEC 16 "History clamp", or null (off)
void launch_temporal_resolve(const float4* accum, const float4* pos, const uint4* ids, const float4* hc, const float4* hp, const uint4* hi,
                             const uint32_t* table, uint32_t w, uint32_t h, uint32_t n, bool has_history, float4* temporal, float4* motion,
                             const Tri* tris, const Tri* snap, uint32_t tri_count, const hala_temporal_clamp_params* clamp, hipStream_t s);

}  // namespace rt
