// shutter.h — shutter motion blur of docs/RENDER_SPEC.md 18: two keys per holder (a node's local transform, a deformer's parameters, a
// primitive's vertices), one time per frame of the accumulation, the state at that time per float.  The rules of time and
// interpolation live here for the host (node and deformer keys) and the device (k_shutter_lerp of shutter.hip: vertex keys).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <memory>
#include <vector>

#include "deform.h"
#include "hala_types.h"
#include "host_scene.h"
#include "host_util.h"

namespace rt {

constexpr uint32_t kShutterThreads = 256;       // one lane per dword of the 44-B vertex stream
constexpr uint32_t kShutterNoStep = 0xffffffffu;
constexpr uint32_t kShutterMaxStride = 65536;

// RENDER_SPEC 18 "State": m = (a == b) ? a : a + (tau * (b - a)), each operation rounded (-ffp-contract=off: no fma).  The first branch
// keeps static keys bit-identical, -0.0 included.
__host__ __device__ inline float shutter_mix(float a, float b, float tau) { return a == b ? a : a + (tau * (b - a)); }

// RENDER_SPEC 18 "Time": the base-2 radical inverse of the step, 24 bits (exact in float, in [0, 1)), scaled into the shutter interval
inline uint32_t shutter_bitreverse(uint32_t v) {
  v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
  v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
  v = ((v >> 4) & 0x0f0f0f0fu) | ((v & 0x0f0f0f0fu) << 4);
  v = ((v >> 8) & 0x00ff00ffu) | ((v & 0x00ff00ffu) << 8);
  return (v >> 16) | (v << 16);
}
inline float shutter_time(float open, float close, uint32_t step) {
  const float u = (float)(shutter_bitreverse(step) >> 8) * 5.9604644775390625e-08f;
  return open + (u * (close - open));
}

// what k_shutter_lerp reads and writes of one primitive
struct ShutterLerp {
  const float* __restrict__ open;   // the two keys: vertex_count 44-B records each
  const float* __restrict__ close;
  float* __restrict__ out;          // the primitive's range of the vertex arena
  size_t words;        // vertex_count * 11
  float tau;
  uint32_t* flag;      // set to 1 when an interpolated position is not finite
};
void launch_shutter_lerp(const ShutterLerp& t, hipStream_t s);

struct ShutterNodeKeys { float open[16], close[16]; bool moving; };  // moving: the two keys differ in some byte
struct ShutterDeformKeys { Deformer::Params open, close; bool moving = false; };
struct ShutterVertexKeys {  // both keys stay on the device: 88 B per vertex
  uint32_t vertex_count = 0;
  bool moving = false;
  DeviceArray<hala_vertex> d_open, d_close;
};

// One set of keys and shutter parameters.  A holder whose two keys are the same bytes does not move: it is kept (the refusals hold) but
// does not make the shutter active.
struct ShutterKeys {
  bool on = false;
  float open = 0.0f, close = 1.0f;
  uint32_t stride = 1;
  std::map<uint32_t, ShutterNodeKeys> nodes;                                // key: node index
  std::map<uint32_t, std::shared_ptr<const ShutterDeformKeys>> deformers;   // key: index into HostScene::prims
  std::map<uint32_t, std::shared_ptr<const ShutterVertexKeys>> vertices;    // key: index into HostScene::prims
  uint32_t moving = 0;  // holders whose keys differ (recount)
  void recount() {
    moving = 0;
    for (const auto& kv : nodes) moving += kv.second.moving ? 1u : 0u;
    for (const auto& kv : deformers) moving += kv.second->moving ? 1u : 0u;
    for (const auto& kv : vertices) moving += kv.second->moving ? 1u : 0u;
  }
  bool any() const { return !nodes.empty() || !deformers.empty() || !vertices.empty(); }
  bool active() const { return on && close != open && moving != 0u; }
  float time(uint32_t step) const { return on ? shutter_time(open, close, step) : 0.0f; }
};

}  // namespace rt
