// node_batch.hip — the device half of hala_rt_refit_nodes (docs/RENDER_SPEC.md 20): the caller's array of local transforms scattered
// into the table of all node locals, the world matrices of the affected nodes level by level, and the transforms of the affected
// instances with the test that decides whether an instance can be intersected in object space.  The arithmetic is the host's
// (host_scene.cpp: mul; rt_trees.hip: world_to_object), operation for operation: __fmul_rn / __fadd_rn keep the four-term sums in the
// host's order and unfused whatever the compiler is told, the division is IEEE.  The host looks at one word afterwards.
#include "node_batch.h"

#include "rt_math.h"

namespace rt {

namespace {

RT_DI void copy64(float* dst, const float* src) {  // one 64-B matrix, four 16-B moves (both 16-B aligned)
  const float4* s = reinterpret_cast<const float4*>(src);
  float4* d = reinterpret_cast<float4*>(dst);
#pragma unroll
  for (int k = 0; k < 4; ++k) d[k] = s[k];
}

// 16 threads per matrix would leave the stores narrow; a matrix per thread keeps them 16 B wide and the tables are small
__global__ void __launch_bounds__(256) k_node_locals(const float* __restrict__ in, const uint32_t* __restrict__ bound, uint32_t count,
                                                      float* __restrict__ locals, uint32_t node_count) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= count) return;
  const uint32_t node = bound[k];
  if (node >= node_count) return;  // (the host refused such an index at bind time)
  alignas(16) float m[16];  // the caller's array is only known to be 4-B aligned
#pragma unroll
  for (int i = 0; i < 16; ++i) m[i] = in[(size_t)k * 16u + i];
  copy64(locals + (size_t)node * 16u, m);
}

__global__ void __launch_bounds__(256) k_node_worlds(const NodeBatchNode* __restrict__ level, uint32_t n, const float* __restrict__ locals,
                                                      float* __restrict__ worlds, uint32_t node_count) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  const NodeBatchNode e = level[k];
  if (e.node >= node_count || (e.parent >= 0 && (uint32_t)e.parent >= node_count)) return;
  alignas(16) float b[16], out[16];
  copy64(b, locals + (size_t)e.node * 16u);
  if (e.parent < 0) {
    copy64(worlds + (size_t)e.node * 16u, b);
    return;
  }
  alignas(16) float a[16];
  copy64(a, worlds + (size_t)e.parent * 16u);  // written by the launch of the level above, or current since the bind
  // host_scene.cpp::mul — column c of the product = ((A.x * b.x + A.y * b.y) + A.z * b.z) + A.w * b.w
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int row = 0; row < 4; ++row) {
      float acc = __fmul_rn(a[0 + row], b[4 * c + 0]);
      acc = __fadd_rn(acc, __fmul_rn(a[4 + row], b[4 * c + 1]));
      acc = __fadd_rn(acc, __fmul_rn(a[8 + row], b[4 * c + 2]));
      acc = __fadd_rn(acc, __fmul_rn(a[12 + row], b[4 * c + 3]));
      out[4 * c + row] = acc;
    }
  copy64(worlds + (size_t)e.node * 16u, out);
}

RT_DI bool finite_f(float v) { return fabsf(v) <= 3.402823466e+38f; }  // false for NaN and the infinities

// rt_trees.hip::world_to_object's verdict: can the transform be inverted in float, with every entry of the result finite
RT_DI bool invertible(const float* m) {
  const f3 c0 = mk3(m[0], m[1], m[2]), c1 = mk3(m[4], m[5], m[6]), c2 = mk3(m[8], m[9], m[10]);
  const f3 k0 = cross3(c1, c2), k1 = cross3(c2, c0), k2 = cross3(c0, c1);
  const float det = dot3(c0, k0);
  if (!(det != 0.0f) || !finite_f(det)) return false;
  const float inv = 1.0f / det;  // IEEE division, correctly rounded under the library's flags, like the host's
  const float v[12] = {k0.x * inv, k0.y * inv, k0.z * inv, k1.x * inv, k1.y * inv, k1.z * inv, k2.x * inv, k2.y * inv, k2.z * inv, m[12], m[13], m[14]};
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 12; ++k) ok = ok && finite_f(v[k]);
  return ok;
}

__global__ void __launch_bounds__(256) k_instance_transforms(const NodeBatchInst* __restrict__ items, uint32_t n, const float* __restrict__ worlds,
                                                              uint32_t node_count, hala_gpu_mesh_data* __restrict__ instances, uint32_t instance_count,
                                                              hala_gpu_mesh_data* __restrict__ world_md, uint32_t world_md_count,
                                                              uint32_t* __restrict__ mismatch, uint32_t detect_moved) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  const NodeBatchInst it = items[k];
  if (it.inst >= instance_count || it.node >= node_count) return;
  alignas(16) float m[16];
  copy64(m, worlds + (size_t)it.node * 16u);
  if (detect_moved) {  // RENDER_SPEC 4.6: what refit_geometry's comparison of the transforms would find, bit for bit
    const uint4* was = reinterpret_cast<const uint4*>(instances[it.inst].transform);
    const uint4* is = reinterpret_cast<const uint4*>(m);
    bool same = true;
#pragma unroll
    for (int q = 0; q < 4; ++q) same = same && was[q].x == is[q].x && was[q].y == is[q].y && was[q].z == is[q].z && was[q].w == is[q].w;
    if (!same) atomicOr(mismatch, it.md_slot < world_md_count ? (kNodeBatchMoved | kNodeBatchMovedWorldTree) : kNodeBatchMoved);
  }
  copy64(instances[it.inst].transform, m);  // the other 32 bytes of the record stand
  if (it.md_slot < world_md_count) copy64(world_md[it.md_slot].transform, m);
  const uint32_t now = (it.check & 1u) && invertible(m) ? 1u : 0u;
  if (now != ((it.check >> 1) & 1u)) atomicOr(mismatch, kNodeBatchMismatch);
}

inline uint32_t blocks(uint32_t n) { return (n + 255u) / 256u; }

}  // namespace

void launch_node_locals(const float* in, const uint32_t* bound, uint32_t count, float* locals, uint32_t node_count, hipStream_t s) {
  if (count) hipLaunchKernelGGL(k_node_locals, dim3(blocks(count)), dim3(256), 0, s, in, bound, count, locals, node_count);
}
void launch_node_worlds(const NodeBatchNode* level, uint32_t n, const float* locals, float* worlds, uint32_t node_count, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_node_worlds, dim3(blocks(n)), dim3(256), 0, s, level, n, locals, worlds, node_count);
}
void launch_instance_transforms(const NodeBatchInst* items, uint32_t n, const float* worlds, uint32_t node_count, hala_gpu_mesh_data* instances,
                                uint32_t instance_count, hala_gpu_mesh_data* world_md, uint32_t world_md_count, uint32_t* mismatch, bool detect_moved,
                                hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_instance_transforms, dim3(blocks(n)), dim3(256), 0, s, items, n, worlds, node_count, instances, instance_count, world_md,
                            world_md_count, mismatch, detect_moved ? 1u : 0u);
}

}  // namespace rt
