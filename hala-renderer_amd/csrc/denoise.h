// denoise.h — the a-trous denoiser of docs/RENDER_SPEC.md 10: device buffers and the host side of its launches (denoise.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "hala_types.h"
#include "host_util.h"

namespace rt {

// Per pixel: the guide (unit normal, albedo.x), then a ping-pong pair of (E, albedo.y) and (g(E), albedo.z) — 48 B read per tap,
// the albedo riding along in the fourth lanes so that every tap is three 16-B loads.  `out` is the RGBA32F result.
struct DenoiseBuffers {
  DeviceArray<float4> guide, e[2], g[2], out;
  uint32_t width = 0, height = 0;
  hipError_t ensure(uint32_t w, uint32_t h);  // (re)allocates when the size changes
};

// "" or the reason the parameters are refused (no device call)
std::string denoise_check_params(const hala_denoise_params* p);
// the prepass and the N passes, stream-ordered; accum / albedo / normal are row-major RGBA32F images of b.width x b.height
hipError_t denoise_enqueue(DenoiseBuffers& b, const float4* accum, const float4* albedo, const float4* normal, const hala_denoise_params& p,
                           hipStream_t s);

}  // namespace rt
