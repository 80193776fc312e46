// adaptive.hip — docs/RENDER_SPEC.md 11: adaptive sampling over the 8 x 8 pixel blocks of the unsharded slot order.  A check compares
// the running mean of every pixel of an active block with the snapshot taken at the previous check; a block whose every in-frame pixel
// passes stops being traced, and the compaction rebuilds the list of active blocks that slot_to_pixel (shading.h) reads.  Every
// operation is the one the spec writes, in its order (-ffp-contract=off: no fma), so that tests/adaptive_ref.py reproduces each decision.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "adaptive.h"

namespace rt {

namespace {

constexpr uint32_t kBlock = 8;              // RENDER_SPEC 11: the 8 x 8 blocks of §9 (rt_outputs.hip refuses other RT_PIXEL_BLOCK builds)
constexpr uint32_t kCheckThreads = 256;     // four blocks per workgroup, one per wave
constexpr uint32_t kCompactThreads = 1024;  // one workgroup scans every block: 130 K blocks at 3840 x 2160 are 128 passes

__global__ void __launch_bounds__(256) k_adaptive_begin(uint32_t* __restrict__ list, uint32_t* __restrict__ block_count, uint32_t total) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= total) return;
  list[b] = b;
  block_count[b] = 0u;
}

// One wave per active block, lane i on the block's pixel i (row-major inside the block).  The block converges iff every in-frame lane
// passes (a NaN error fails `e < threshold`); out-of-frame lanes of a border block do not vote.
__global__ void __launch_bounds__(kCheckThreads) k_adaptive_check(const float4* __restrict__ accum, float4* __restrict__ snap,
                                                                  const uint32_t* __restrict__ list, uint32_t* __restrict__ block_count,
                                                                  uint32_t active, uint32_t width, uint32_t height, uint32_t blocks_x,
                                                                  float exposure, float k, float threshold, uint32_t n) {
  const uint32_t w = blockIdx.x * (kCheckThreads / 64u) + (threadIdx.x >> 6);
  if (w >= active) return;  // whole wave
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t b = list[w];
  const uint32_t by = b / blocks_x, bx = b - by * blocks_x;
  const uint32_t px = bx * kBlock + (lane & 7u), py = by * kBlock + (lane >> 3);
  const bool in = px < width && py < height;
  const size_t at = (size_t)py * width + px;
  bool pass = true;
  float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (in) {
    a = accum[at];
    const float4 s = snap[at];
    const float ix = a.x * exposure, iy = a.y * exposure, iz = a.z * exposure;
    const float sx = s.x * exposure, sy = s.y * exposure, sz = s.z * exposure;
    const float d = (fabsf(ix - sx) + fabsf(iy - sy)) + fabsf(iz - sz);
    const float l = (ix + iy) + iz;
    const float e = (d * k) / (1e-4f + sqrtf(l > 0.0f ? l : 0.0f));
    pass = e < threshold;
  }
  const bool converged = __ballot(!pass) == 0ull;
  if (converged) {
    if (lane == 0u) block_count[b] = n;
  } else if (in) {
    snap[at] = a;  // the next check measures from here
  }
}

// The active blocks (count 0) in ascending block order, their number and their in-frame pixels.  One workgroup: per pass of 1024 blocks
// a ballot per wave, the wave totals in LDS, and each active block's position = blocks before this pass + earlier waves + earlier lanes.
__global__ void __launch_bounds__(kCompactThreads) k_adaptive_compact(const uint32_t* __restrict__ block_count, uint32_t total, uint32_t width,
                                                                      uint32_t height, uint32_t blocks_x, uint32_t* __restrict__ list,
                                                                      uint32_t* __restrict__ counts) {
  constexpr uint32_t kWaves = kCompactThreads / 64u;
  __shared__ uint32_t s_wave[kWaves];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t base = 0, pixels = 0;
  for (uint32_t first = 0; first < total; first += kCompactThreads) {
    const uint32_t b = first + threadIdx.x;
    const bool act = b < total && block_count[b] == 0u;
    const unsigned long long m = __ballot(act);
    if (lane == 0u) s_wave[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = base, all = 0;
    for (uint32_t v = 0; v < kWaves; ++v) {
      const uint32_t c = s_wave[v];
      before += v < wave ? c : 0u;
      all += c;
    }
    if (act) {
      list[before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = b;
      const uint32_t by = b / blocks_x, bx = b - by * blocks_x;
      pixels += min(kBlock, width - bx * kBlock) * min(kBlock, height - by * kBlock);
    }
    base += all;
    __syncthreads();  // s_wave is rewritten by the next pass
  }
  for (int off = 32; off > 0; off >>= 1) pixels += (uint32_t)__shfl_down((int)pixels, off);
  if (lane == 0u) s_wave[wave] = pixels;
  __syncthreads();
  if (threadIdx.x == 0u) {
    uint32_t sum = 0;
    for (uint32_t v = 0; v < kWaves; ++v) sum += s_wave[v];
    counts[0] = base;
    counts[1] = sum;
  }
}

}  // namespace

hipError_t AdaptiveState::ensure(uint32_t blocks, size_t pixels) {
  hipError_t e = snapshot.resize(pixels);
  if (e == hipSuccess) e = block_count.resize(blocks);
  if (e == hipSuccess) e = lists[0].resize(blocks);
  if (e == hipSuccess) e = lists[1].resize(blocks);
  if (e == hipSuccess) e = counts.resize(2);
  if (e == hipSuccess && !host_counts) e = hipHostMalloc(reinterpret_cast<void**>(&host_counts), 2 * sizeof(uint32_t), hipHostMallocDefault);
  if (e != hipSuccess) { release(); return e; }
  total_blocks = blocks;
  return hipSuccess;
}

void AdaptiveState::release() {
  snapshot.release(); block_count.release(); lists[0].release(); lists[1].release(); counts.release();
  if (host_counts) (void)hipHostFree(host_counts);
  host_counts = nullptr;
}

std::string adaptive_check_params(const hala_adaptive_params* p) {
  if (!p) return "The adaptive sampling parameters are null.";
  if (!std::isfinite(p->threshold) || !(p->threshold > 0.0f)) return "Invalid adaptive sampling threshold (finite and > 0).";
  if (p->min_samples < 2u || p->min_samples > 65536u) return "Invalid adaptive sampling min_samples (2 ... 65536).";
  if (p->interval < 1u || p->interval > 65536u) return "Invalid adaptive sampling interval (1 ... 65536).";
  for (uint32_t v : p->reserved) if (v != 0u) return "Invalid adaptive sampling parameters (reserved fields must be 0).";
  return "";
}

uint64_t adaptive_frames_to_event(const hala_adaptive_params& p, uint64_t n) {
  const uint64_t h = p.min_samples / 2u;
  if (n < h) return h - n;
  if (n < p.min_samples) return p.min_samples - n;
  return p.interval - (n - p.min_samples) % p.interval;
}

hipError_t adaptive_begin(AdaptiveState& a, hipStream_t s) {
  hipLaunchKernelGGL(k_adaptive_begin, dim3((a.total_blocks + 255u) / 256u), dim3(256), 0, s, a.lists[0].ptr, a.block_count.ptr, a.total_blocks);
  return hipGetLastError();
}

hipError_t adaptive_enqueue_check(AdaptiveState& a, const float4* accum, uint32_t width, uint32_t height, uint32_t blocks_x, float exposure,
                                  uint32_t n, hipStream_t s) {
  const uint32_t sn = a.last_snapshot;
  const float k = sqrtf((float)sn / (float)(n - sn));  // RENDER_SPEC 11: once per check, on the host
  constexpr uint32_t per = kCheckThreads / 64u;
  hipLaunchKernelGGL(k_adaptive_check, dim3((a.active_blocks + per - 1u) / per), dim3(kCheckThreads), 0, s, accum, a.snapshot.ptr,
                     a.lists[a.cur].ptr, a.block_count.ptr, a.active_blocks, width, height, blocks_x, exposure, k, a.p.threshold, n);
  hipLaunchKernelGGL(k_adaptive_compact, dim3(1), dim3(kCompactThreads), 0, s, a.block_count.ptr, a.total_blocks, width, height, blocks_x,
                     a.lists[a.cur ^ 1u].ptr, a.counts.ptr);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(a.host_counts, a.counts.ptr, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
  return e;
}

void adaptive_finish_check(AdaptiveState& a, uint32_t n) {
  a.cur ^= 1u;
  a.active_blocks = a.host_counts[0];
  a.active_pixels = a.host_counts[1];
  a.last_snapshot = n;
}

}  // namespace rt

using namespace rt;

static_assert(sizeof(hala_adaptive_params) == 32 && sizeof(hala_adaptive_status) == 32, "adaptive records are 32 B");

void hala_adaptive_default_params(hala_adaptive_params* out) {
  if (!out) return;
  memset(out, 0, sizeof(*out));
  out->threshold = 0.2f;
  out->min_samples = 16;
  out->interval = 16;
}
