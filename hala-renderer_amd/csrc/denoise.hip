// denoise.hip — docs/RENDER_SPEC.md 10: edge-avoiding a-trous wavelet filter (Dammertz et al., HPG 2010) over the running means,
// guided by the first-hit albedo and normal AOVs.  One prepass packs the guides and the (demodulated) colour, then N gather passes
// ping-pong between two buffers; the last one multiplies the albedo back and writes RGBA32F.  Every operation is the one the spec
// writes, in its order (-ffp-contract=off: no fma), so that tests/denoise_ref.py reproduces the result bit for bit.
//
// Tap gathering: each lane gathers its 25 taps straight from global memory (three 16-B loads per tap).  A pass touches 80 B per
// pixel of unique data (166 MB at 1920x1080), which stays resident in the 256-MiB Infinity Cache from one pass to the next, and the
// 16 x 16 workgroups make the taps of the short steps L1 / L2 hits (DESIGN.md "Denoising" has the measured time).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "denoise.h"

namespace rt {

namespace {

constexpr uint32_t kTile = 16;                  // 16 x 16 pixels per workgroup
constexpr float kMinAlbedo = 1.0f / 256.0f;      // demodulation floor of RENDER_SPEC 10

__device__ __forceinline__ float dn_lum(float x, float y, float z) { return (0.212671f * x + 0.715160f * y) + 0.072169f * z; }
// `a > b ? a : b` (NaN -> b), the form the numpy twin uses
__device__ __forceinline__ float dn_max(float a, float b) { return a > b ? a : b; }

__global__ void __launch_bounds__(256) k_denoise_prepass(const float4* __restrict__ accum, const float4* __restrict__ albedo,
                                                         const float4* __restrict__ normal, uint32_t n, uint32_t demodulate,
                                                         float4* __restrict__ guide, float4* __restrict__ e_out, float4* __restrict__ g_out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 c = accum[i], a = albedo[i], nm = normal[i];
  const float l2 = nm.x * nm.x + nm.y * nm.y + nm.z * nm.z;
  float nx = 0.0f, ny = 0.0f, nz = 0.0f;
  if (l2 > 0.0f) {
    const float inv = 1.0f / sqrtf(l2);
    nx = nm.x * inv; ny = nm.y * inv; nz = nm.z * inv;
  }
  float ex = c.x, ey = c.y, ez = c.z;
  if (demodulate) { ex = c.x / dn_max(a.x, kMinAlbedo); ey = c.y / dn_max(a.y, kMinAlbedo); ez = c.z / dn_max(a.z, kMinAlbedo); }
  const float t = 1.0f / (1.0f + dn_lum(ex, ey, ez));
  guide[i] = make_float4(nx, ny, nz, a.x);
  e_out[i] = make_float4(ex, ey, ez, a.y);
  g_out[i] = make_float4(ex * t, ey * t, ez * t, a.z);
}

// one a-trous pass at step `step`; kLast: write E * ad with alpha 1 to `out` instead of the next (E, g(E)) pair
template <bool kLast>
__global__ void __launch_bounds__(256) k_denoise_atrous(const float4* __restrict__ guide, const float4* __restrict__ e_in,
                                                        const float4* __restrict__ g_in, uint32_t width, uint32_t height, int step,
                                                        float ia, float ic, uint32_t log2_power, uint32_t demodulate,
                                                        float4* __restrict__ e_out, float4* __restrict__ g_out, float4* __restrict__ out) {
  const int x = (int)(blockIdx.x * kTile + threadIdx.x), y = (int)(blockIdx.y * kTile + threadIdx.y);
  const int w = (int)width, h = (int)height;
  if (x >= w || y >= h) return;
  const uint32_t p = (uint32_t)y * width + (uint32_t)x;
  const float4 gp = guide[p], ep = e_in[p], cp = g_in[p];
  const bool p_zero = gp.x == 0.0f && gp.y == 0.0f && gp.z == 0.0f;
  constexpr float kH[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
  float sx = 0.0f, sy = 0.0f, sz = 0.0f, sw = 0.0f;
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
    const int qy = y + step * dy;
    if (qy < 0 || qy >= h) continue;  // out-of-frame taps are skipped
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const int qx = x + step * dx;
      if (qx < 0 || qx >= w) continue;
      const float hh = kH[dx + 2] * kH[dy + 2];
      float wt, qex, qey, qez;
      if (dx == 0 && dy == 0) {
        wt = hh; qex = ep.x; qey = ep.y; qez = ep.z;  // k = 1
      } else {
        const uint32_t q = (uint32_t)qy * width + (uint32_t)qx;
        const float4 gq = guide[q], eq = e_in[q], cq = g_in[q];
        float d = gp.x * gq.x + gp.y * gq.y + gp.z * gq.z;
        d = dn_max(d, 0.0f);
        if (p_zero && gq.x == 0.0f && gq.y == 0.0f && gq.z == 0.0f) d = 1.0f;
        for (uint32_t k = 0; k < log2_power; ++k) d = d * d;  // wn = d^P
        const float a0 = gp.w - gq.w, a1 = ep.w - eq.w, a2 = cp.w - cq.w;
        const float wa = 1.0f / (1.0f + (a0 * a0 + a1 * a1 + a2 * a2) * ia);
        const float c0 = cp.x - cq.x, c1 = cp.y - cq.y, c2 = cp.z - cq.z;
        const float wc = 1.0f / (1.0f + (c0 * c0 + c1 * c1 + c2 * c2) * ic);
        wt = hh * ((d * wa) * wc);
        qex = eq.x; qey = eq.y; qez = eq.z;
      }
      sx = sx + qex * wt; sy = sy + qey * wt; sz = sz + qez * wt;
      sw = sw + wt;
    }
  }
  const float ex = sx / sw, ey = sy / sw, ez = sz / sw;
  if (kLast) {
    if (demodulate)
      out[p] = make_float4(ex * dn_max(gp.w, kMinAlbedo), ey * dn_max(ep.w, kMinAlbedo), ez * dn_max(cp.w, kMinAlbedo), 1.0f);
    else
      out[p] = make_float4(ex, ey, ez, 1.0f);
  } else {
    const float t = 1.0f / (1.0f + dn_lum(ex, ey, ez));
    e_out[p] = make_float4(ex, ey, ez, ep.w);
    g_out[p] = make_float4(ex * t, ey * t, ez * t, cp.w);
  }
}

}  // namespace

hipError_t DenoiseBuffers::ensure(uint32_t w, uint32_t h) {
  if (w == width && h == height && out.ptr) return hipSuccess;
  const size_t n = (size_t)w * h;
  width = height = 0;
  for (DeviceArray<float4>* a : {&guide, &e[0], &e[1], &g[0], &g[1], &out}) {
    const hipError_t err = a->resize(n);
    if (err != hipSuccess) return err;
  }
  width = w; height = h;
  return hipSuccess;
}

std::string denoise_check_params(const hala_denoise_params* p) {
  if (!p) return "The denoise parameters are null.";
  if (p->iterations < 1 || p->iterations > 8) return "Invalid denoise iterations " + std::to_string(p->iterations) + ": expected 1..8.";
  const auto sigma_ok = [](float s) { return s >= 1e-6f && s <= 1e6f; };  // NaN fails
  if (!sigma_ok(p->sigma_color)) return "Invalid denoise sigma_color: expected a finite value in [1e-6, 1e6].";
  if (!sigma_ok(p->sigma_albedo)) return "Invalid denoise sigma_albedo: expected a finite value in [1e-6, 1e6].";
  const uint32_t np = p->normal_power;
  if (np < 1 || np > 128 || (np & (np - 1)) != 0) return "Invalid denoise normal_power " + std::to_string(np) + ": expected a power of two in 1..128.";
  if (p->demodulate > 1) return "Invalid denoise demodulate flag: expected 0 or 1.";
  if (p->reserved[0] || p->reserved[1] || p->reserved[2]) return "The reserved words of the denoise parameters must be zero.";
  return "";
}

hipError_t denoise_enqueue(DenoiseBuffers& b, const float4* accum, const float4* albedo, const float4* normal, const hala_denoise_params& p,
                           hipStream_t s) {
  const uint32_t w = b.width, h = b.height, n = w * h;
  uint32_t log2_power = 0;
  while ((1u << log2_power) < p.normal_power) ++log2_power;
  const float ia = 1.0f / (p.sigma_albedo * p.sigma_albedo);
  const float inv_c = 1.0f / (p.sigma_color * p.sigma_color);
  k_denoise_prepass<<<(n + 255) / 256, 256, 0, s>>>(accum, albedo, normal, n, p.demodulate, b.guide.ptr, b.e[0].ptr, b.g[0].ptr);
  const dim3 grid((w + kTile - 1) / kTile, (h + kTile - 1) / kTile), block(kTile, kTile);
  for (uint32_t i = 0; i < p.iterations; ++i) {
    const float ic = (float)(1u << (2u * i)) * inv_c;  // the colour tolerance halves with each pass
    const uint32_t src = i & 1u, dst = src ^ 1u;
    if (i + 1 == p.iterations)
      k_denoise_atrous<true><<<grid, block, 0, s>>>(b.guide.ptr, b.e[src].ptr, b.g[src].ptr, w, h, 1 << i, ia, ic, log2_power, p.demodulate,
                                                    nullptr, nullptr, b.out.ptr);
    else
      k_denoise_atrous<false><<<grid, block, 0, s>>>(b.guide.ptr, b.e[src].ptr, b.g[src].ptr, w, h, 1 << i, ia, ic, log2_power, p.demodulate,
                                                     b.e[dst].ptr, b.g[dst].ptr, nullptr);
  }
  return hipGetLastError();
}

}  // namespace rt

using namespace rt;

static_assert(sizeof(hala_denoise_params) == 32, "hala_denoise_params is 32 B");

void hala_denoise_default_params(hala_denoise_params* out) {
  if (!out) return;
  memset(out, 0, sizeof(*out));
  out->iterations = 5;
  out->sigma_color = 0.5f;
  out->sigma_albedo = 0.1f;
  out->normal_power = 32;
  out->demodulate = 1;
}

int hala_denoise_images(int device_ordinal, const float* color, const float* albedo, const float* normal, uint32_t width, uint32_t height,
                        const hala_denoise_params* p, float* dst) {
  const std::string bad = denoise_check_params(p);
  if (!bad.empty()) RT_FAIL(bad);
  if (!color || !albedo || !normal || !dst) RT_FAIL("Invalid argument: an image pointer is null.");
  if (width == 0 || height == 0 || width > 65536 || height > 65536 || (uint64_t)width * height > (1ull << 28))
    RT_FAIL("Invalid image size " + std::to_string(width) + " x " + std::to_string(height) + ".");
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) RT_FAIL("No HIP device is available: libhalart has no CPU path.");
  RT_HIP(hipSetDevice(device_ordinal));
  const size_t n = (size_t)width * height;
  DeviceArray<float4> d_in[3];
  const float* src[3] = {color, albedo, normal};
  for (int k = 0; k < 3; ++k) RT_HIP(d_in[k].upload(reinterpret_cast<const float4*>(src[k]), n, nullptr));
  DenoiseBuffers b;
  RT_HIP(b.ensure(width, height));
  RT_HIP(denoise_enqueue(b, d_in[0].ptr, d_in[1].ptr, d_in[2].ptr, *p, nullptr));
  RT_HIP(hipMemcpy(dst, b.out.ptr, n * sizeof(float4), hipMemcpyDeviceToHost));
  return HALA_OK;
}
