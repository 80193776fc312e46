// adaptive.h — adaptive sampling of docs/RENDER_SPEC.md 11: device state and the host side of its launches (adaptive.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "hala_types.h"
#include "host_util.h"

namespace rt {

// Everything is allocated by the first hala_rt_set_adaptive_sampling that enables the feature (ensure) and freed when it is turned off.
struct AdaptiveState {
  bool enabled = false;
  hala_adaptive_params p{};
  uint32_t total_blocks = 0;    // 8 x 8 pixel blocks of the frame (unsharded slot order, RENDER_SPEC §9)
  uint32_t active_blocks = 0;   // host copy, as the last check left it
  uint32_t active_pixels = 0;   // in-frame pixels of the active blocks
  uint32_t last_snapshot = 0;   // s
  uint32_t cur = 0;             // lists[cur] holds the active blocks in ascending order
  DeviceArray<float4> snapshot;      // S: RGBA32F, W*H, row-major
  DeviceArray<uint32_t> block_count; // per block: c_b once converged, 0 while active
  DeviceArray<uint32_t> lists[2];
  DeviceArray<uint32_t> counts;      // k_adaptive_compact: [0] active blocks, [1] their in-frame pixels
  uint32_t* host_counts = nullptr;   // pinned copy of counts
  ~AdaptiveState() { release(); }
  hipError_t ensure(uint32_t blocks, size_t pixels);
  void release();
  // a new accumulation: every block active (the device side is re-armed by begin, at frame_index 0)
  void restart(uint32_t pixels) { active_blocks = total_blocks; active_pixels = pixels; last_snapshot = 0; cur = 0; }
};

// "" or the reason the parameters are refused (no device call)
std::string adaptive_check_params(const hala_adaptive_params* p);
// RENDER_SPEC 11 schedule, in samples n after an update
inline bool adaptive_is_check(const hala_adaptive_params& p, uint64_t n) { return n >= p.min_samples && (n - p.min_samples) % p.interval == 0; }
// frames from n to the next snapshot or check frame (>= 1): hala_rt_update_batch ends its chunks there
uint64_t adaptive_frames_to_event(const hala_adaptive_params& p, uint64_t n);
// frame_index 0: every block active, no count recorded
hipError_t adaptive_begin(AdaptiveState& a, hipStream_t s);
// the check at n (after the update that made it n) and the compaction into the other list; the two counts land in host_counts once the
// stream has reached them (the caller synchronises, then calls adaptive_finish_check)
hipError_t adaptive_enqueue_check(AdaptiveState& a, const float4* accum, uint32_t width, uint32_t height, uint32_t blocks_x, float exposure,
                                  uint32_t n, hipStream_t s);
void adaptive_finish_check(AdaptiveState& a, uint32_t n);

}  // namespace rt
