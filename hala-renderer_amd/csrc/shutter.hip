// shutter.hip — docs/RENDER_SPEC.md 18: k_shutter_lerp writes a primitive's range of the vertex arena from its two device-resident
// vertex keys at the time of the step, right ahead of the refit kernels that read it.  The state per float is shutter_mix (shutter.h):
// `(a == b) ? a : a + (tau * (b - a))`, each operation rounded (-ffp-contract=off: no fma), so that tests/shutter_ref.py reproduces the
// vertices bit for bit.
//
// The records carry no coupling between lanes, so the 44-B stream is walked as dwords: one lane per dword, neighbouring lanes on
// neighbouring dwords (a wave's 64 dwords are one contiguous 256-B run of each key and of the arena), no LDS.  Nine of every eleven
// dwords — position, normal, tangent — are interpolated; the two of tex_coord are the open key's, and the close key is not read
// for them.  Per vertex: 44 B + 36 B read, 44 B written.
//
// An interpolated position (dwords 0-2 of a record) that is not finite raises the flag the way k_deform does: one ballot per wave, one
// atomic only when a lane offends.
#include <hip/hip_runtime.h>

#include "shutter.h"

namespace rt {

namespace {

constexpr uint32_t kRecordWords = sizeof(hala_vertex) / 4;  // 11
static_assert(sizeof(hala_vertex) == 44, "k_shutter_lerp walks 11 dwords per vertex");

__global__ __launch_bounds__(kShutterThreads) void k_shutter_lerp(const ShutterLerp t) {
  const size_t i = (size_t)blockIdx.x * kShutterThreads + threadIdx.x;
  bool bad = false;
  if (i < t.words) {
    // dword of the record: 0-2 position, 3-5 normal, 6-8 tangent, 9-10 tex_coord.  i mod 11 in 32 bits: i = 256 block + lane
    const uint32_t c = ((blockIdx.x % kRecordWords) * (kShutterThreads % kRecordWords) + threadIdx.x) % kRecordWords;
    float m = t.open[i];
    if (c < 9u) {
      m = shutter_mix(m, t.close[i], t.tau);
      bad = c < 3u && !isfinite(m);
    }
    t.out[i] = m;
  }
  const unsigned long long offenders = __ballot(bad);
  if (offenders && (threadIdx.x & 63u) == (uint32_t)__ffsll((long long)offenders) - 1u) atomicOr(t.flag, 1u);
}

}  // namespace

void launch_shutter_lerp(const ShutterLerp& t, hipStream_t s) {
  if (!t.words) return;
  const size_t blocks = (t.words + kShutterThreads - 1) / kShutterThreads;  // (at most 2^32 vertices x 11 / 256: below 2^31)
  hipLaunchKernelGGL(k_shutter_lerp, dim3((uint32_t)blocks), dim3(kShutterThreads), 0, s, t);
}

}  // namespace rt
