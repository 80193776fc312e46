// deform.hip — docs/RENDER_SPEC.md 17: morph targets and skinning on the GPU.  k_deform poses the vertices of every dirty deformer of
// a refit, one or many, from their rest poses into the vertex arena, just ahead of the refit that reads them: one launch, a segment per
// deformer, a workgroup inside one segment, one lane per vertex, 256-thread workgroups, wave64.  Every `*` and `+` is the one the spec
// writes, each rounded (-ffp-contract=off: no fma), so that tests/deform_ref.py reproduces the vertices bit for bit.
//
// Memory per vertex: 44 B of the rest record read and 44 B of the posed record written, 12 B per active target and attribute that has
// deltas (a wave's 64 vertices of one target are one contiguous 768-B run), 8 B of joint indices and 16 B of weights when there is a
// skin.  The joint palette (at most 256 x 48 B) is staged in LDS once per workgroup; each lane reads its four matrices from there as
// 16-B quads.  The segment's active targets are walked by a wave-uniform loop (scalar loads).
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
// Device memory, said so: a pointer that k_deform reads from its segment table is generic to the compiler, which would address it with
// flat instructions.
#define DF_GLOBAL __attribute__((address_space(1)))
typedef float df_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t df_u32x2 __attribute__((ext_vector_type(2)));

constexpr uint32_t kRecordWords = sizeof(hala_vertex) / 4;  // 11
static_assert(sizeof(hala_vertex) == 44, "k_deform moves 11 dwords per vertex");

struct Row { float x, y, z, w; };

__device__ __forceinline__ void morph(float* a, const DF_GLOBAL float* deltas, size_t at, float w) {
  // p = p + (w_t * delta) per component
  const float dx = deltas[at], dy = deltas[at + 1], dz = deltas[at + 2];
  a[0] = a[0] + (w * dx); a[1] = a[1] + (w * dy); a[2] = a[2] + (w * dz);
}

__device__ __forceinline__ float affine(const Row& m, const float* p) { return ((m.x * p[0] + m.y * p[1]) + m.z * p[2]) + m.w; }
__device__ __forceinline__ float linear(const Row& m, const float* p) { return (m.x * p[0] + m.y * p[1]) + m.z * p[2]; }

// RENDER_SPEC 17 for vertex `v` of the primitive `t` describes.  `active` lists its active_count active targets (wave-uniform);
// `palette` is the primitive's palette in LDS.  -> whether the posed position is not finite
__device__ __forceinline__ bool pose_vertex(const DeformTables& t, uint32_t active_count, const DeformActiveEntry* __restrict__ active, DF_LDS df_f32x4* palette,
                                            uint32_t v) {
  const uint32_t n = t.vertex_count;
  float r[kRecordWords];  // position, normal, tangent, tex_coord
  const DF_GLOBAL float* src = (const DF_GLOBAL float*)(t.rest + v);
  const DF_GLOBAL float* dp = (const DF_GLOBAL float*)t.dp;
  const DF_GLOBAL float* dn = (const DF_GLOBAL float*)t.dn;
  const DF_GLOBAL float* dt = (const DF_GLOBAL float*)t.dt;
  for (uint32_t k = 0; k < kRecordWords; ++k) r[k] = src[k];
  for (uint32_t i = 0; i < active_count; ++i) {
    const uint32_t index = active[i].index;
    const float w = active[i].weight;
    const size_t at = ((size_t)index * n + v) * 3u;
    morph(r, dp, at, w);
    if (dn) morph(r + 3, dn, at, w);
    if (dt) morph(r + 6, dt, at, w);
  }
  if (t.joint_count) {
    const df_u32x2 jw = ((const DF_GLOBAL df_u32x2*)t.joints)[v];
    const df_f32x4 w4 = ((const DF_GLOBAL df_f32x4*)t.weights)[v];
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
  DF_GLOBAL float* dst = (DF_GLOBAL float*)(t.out + v);
  for (uint32_t k = 0; k < kRecordWords; ++k) dst[k] = r[k];
  return !(isfinite(r[0]) && isfinite(r[1]) && isfinite(r[2]));
}

// the palette of one primitive -> LDS, once per workgroup (uniform branch: every thread of the workgroup passes the barrier or none)
__device__ __forceinline__ void stage_palette(DF_LDS df_f32x4* palette, const float* src, uint32_t joint_count, uint32_t tid) {
  if (!joint_count) return;
  DF_LDS float* pal = (DF_LDS float*)palette;
  const DF_GLOBAL float* from = (const DF_GLOBAL float*)src;
  for (uint32_t k = tid; k < joint_count * 12u; k += kDeformThreads) pal[k] = from[k];
  __syncthreads();
}

// one ballot per wave, one atomic only when a lane offends
__device__ __forceinline__ void raise_flag(bool bad, uint32_t tid, uint32_t* flag) {
  const unsigned long long offenders = __ballot(bad);
  if (offenders && (tid & 63u) == (uint32_t)__ffsll((long long)offenders) - 1u)
    __hip_atomic_fetch_or((DF_GLOBAL uint32_t*)flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (atomicOr, on global memory)
}

// Workgroup b poses the 256 vertices from DeformBlock::first_vertex on of segment DeformBlock::segment; no workgroup spans two
// segments, so the segment, its tables and its active targets are uniform over the workgroup: their addresses derive from blockIdx.x
// alone and nothing the launch writes aliases them, so the loads are scalar.
__global__ __launch_bounds__(kDeformThreads) void k_deform(const DeformSegment* __restrict__ segments, const DeformBlock* __restrict__ blocks,
                                                            const DeformActiveEntry* __restrict__ active) {
  extern __shared__ df_f32x4 smem[];  // the palette of this workgroup's segment
  DF_LDS df_f32x4* palette = (DF_LDS df_f32x4*)smem;
  const uint32_t tid = threadIdx.x;
  const DeformBlock b = blocks[blockIdx.x];
  const DeformTables t = segments[b.segment].t;
  const uint32_t active_count = segments[b.segment].active_count;
  const DeformActiveEntry* __restrict__ act = active + segments[b.segment].active_first;
  const uint32_t v = b.first_vertex + tid;
  stage_palette(palette, t.palette, t.joint_count, tid);
  bool bad = false;
  if (v < t.vertex_count)
    bad = pose_vertex(t, active_count, act, palette, v);
  raise_flag(bad, tid, t.flag);
}

}  // namespace

void launch_deform(const DeformSegment* segments, const DeformBlock* blocks, const DeformActiveEntry* active, uint32_t block_count,
                   uint32_t max_joint_count, hipStream_t s) {
  if (!block_count) return;
  hipLaunchKernelGGL(k_deform, dim3(block_count), dim3(kDeformThreads), (size_t)max_joint_count * 48, s, segments, blocks, active);
}

}  // namespace rt
