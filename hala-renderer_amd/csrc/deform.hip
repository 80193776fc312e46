// deform.hip — docs/RENDER_SPEC.md 17: morph targets and skinning on the GPU.  k_deform poses the vertices of one primitive from its
// rest pose into the vertex arena, just ahead of the refit that reads them: one lane per vertex, 256-thread workgroups, wave64.  Every
// `*` and `+` is the one the spec writes, each rounded (-ffp-contract=off: no fma), so that tests/deform_ref.py reproduces the
// vertices bit for bit.
//
// Memory per vertex: 44 B of the rest record read and 44 B of the posed record written, 12 B per active target and attribute that has
// deltas (a wave's 64 vertices of one target are one contiguous 768-B run), 8 B of joint indices and 16 B of weights when there is a
// skin.  The joint palette (at most 256 x 48 B) is staged in LDS once per workgroup; each lane reads its four matrices from there as
// 16-B quads.  The active targets come in by value and are walked by a wave-uniform loop (scalar loads).
//
// The 44-B records are an array of structures and are read and written in place: 11 dword accesses per lane, 44 B apart from the
// neighbour's, a wave's 64 records being one contiguous 2816-B run that the caches serve whole.  The other form — the workgroup moves
// its run of 256 records with dword accesses in which neighbouring lanes touch neighbouring dwords, through LDS, where a lane picks
// its record at a stride of 11 dwords — was built and measured slower (two barriers and two trips through LDS per record): DESIGN.md 17.
//
// A posed position that is not finite raises the flag: one ballot per wave, one atomic only when a lane offends.
#include <hip/hip_runtime.h>

#include "deform.h"

namespace rt {

namespace {

#define DF_LDS __attribute__((address_space(3)))
typedef float df_f32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kRecordWords = sizeof(hala_vertex) / 4;  // 11
static_assert(sizeof(hala_vertex) == 44, "k_deform moves 11 dwords per vertex");

struct Row { float x, y, z, w; };

__device__ __forceinline__ void morph(float* a, const float* deltas, size_t at, float w) {
  // p = p + (w_t * delta) per component
  const float dx = deltas[at], dy = deltas[at + 1], dz = deltas[at + 2];
  a[0] = a[0] + (w * dx); a[1] = a[1] + (w * dy); a[2] = a[2] + (w * dz);
}

__device__ __forceinline__ float affine(const Row& m, const float* p) { return ((m.x * p[0] + m.y * p[1]) + m.z * p[2]) + m.w; }
__device__ __forceinline__ float linear(const Row& m, const float* p) { return (m.x * p[0] + m.y * p[1]) + m.z * p[2]; }

__global__ __launch_bounds__(kDeformThreads) void k_deform(const DeformTables t, const DeformActive a) {
  extern __shared__ df_f32x4 smem[];  // the palette: 48 B per joint
  DF_LDS df_f32x4* palette = (DF_LDS df_f32x4*)smem;
  const uint32_t tid = threadIdx.x;
  const uint32_t v = blockIdx.x * kDeformThreads + tid;
  const uint32_t n = t.vertex_count;

  if (t.joint_count) {  // (uniform)
    DF_LDS float* pal = (DF_LDS float*)palette;
    for (uint32_t k = tid; k < t.joint_count * 12u; k += kDeformThreads) pal[k] = t.palette[k];
    __syncthreads();
  }

  bool bad = false;
  if (v < n) {
    float r[kRecordWords];  // position, normal, tangent, tex_coord
    const float* src = reinterpret_cast<const float*>(t.rest + v);
    for (uint32_t k = 0; k < kRecordWords; ++k) r[k] = src[k];
    for (uint32_t i = 0; i < a.count; ++i) {
      const size_t at = ((size_t)a.index[i] * n + v) * 3u;
      const float w = a.weight[i];
      morph(r, t.dp, at, w);
      if (t.dn) morph(r + 3, t.dn, at, w);
      if (t.dt) morph(r + 6, t.dt, at, w);
    }
    if (t.joint_count) {
      const uint2 jw = t.joints[v];
      const float4 w4 = t.weights[v];
      const uint32_t j[4] = {jw.x & 0xffffu, jw.x >> 16, jw.y & 0xffffu, jw.y >> 16};
      const float w[4] = {w4.x, w4.y, w4.z, w4.w};
      Row m[3] = {{0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f}};
      for (uint32_t k = 0; k < 4; ++k)
        for (uint32_t row = 0; row < 3; ++row) {
          const df_f32x4 q = palette[j[k] * 3u + row];
          m[row].x = m[row].x + (w[k] * q.x); m[row].y = m[row].y + (w[k] * q.y);
          m[row].z = m[row].z + (w[k] * q.z); m[row].w = m[row].w + (w[k] * q.w);
        }
      const float p[3] = {r[0], r[1], r[2]}, nr[3] = {r[3], r[4], r[5]}, tg[3] = {r[6], r[7], r[8]};
      for (uint32_t row = 0; row < 3; ++row) {
        r[row] = affine(m[row], p);
        r[3 + row] = linear(m[row], nr);
        r[6 + row] = linear(m[row], tg);
      }
    }
    bad = !(isfinite(r[0]) && isfinite(r[1]) && isfinite(r[2]));
    float* dst = reinterpret_cast<float*>(t.out + v);
    for (uint32_t k = 0; k < kRecordWords; ++k) dst[k] = r[k];
  }
  const unsigned long long offenders = __ballot(bad);
  if (offenders && (tid & 63u) == (uint32_t)__ffsll((long long)offenders) - 1u) atomicOr(t.flag, 1u);
}

}  // namespace

void launch_deform(const DeformTables& t, const DeformActive& a, hipStream_t s) {
  if (!t.vertex_count) return;
  const uint32_t blocks = (t.vertex_count + kDeformThreads - 1) / kDeformThreads;
  hipLaunchKernelGGL(k_deform, dim3(blocks), dim3(kDeformThreads), (size_t)t.joint_count * 48, s, t, a);
}

}  // namespace rt
