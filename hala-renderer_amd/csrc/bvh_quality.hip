// bvh_quality.hip — the tree cost of RENDER_SPEC §4.6: one pass over a range of 64-B nodes (§4.1b) that adds up, per child, its box's
// share of the root box's half-area — the surface-area estimate of N_node and N_tri for a long ray that nothing stops.  The shares are
// turned into integers (units of 2^-32) before they are added, so the two sums do not depend on how the reduction is shaped and equal the
// numpy twin's (tests/tree_quality_ref.py) bit for bit.  Compiled like everything else with -ffp-contract=off: three products, two sums.
#include <algorithm>

#include "kernels.h"

namespace rt {
namespace {

constexpr uint32_t kCostBlock = 256;                      // 4 waves
constexpr uint32_t kCostNodesPerBlock = kCostBlock / 4u;  // one lane per (node, child slot): 16 nodes per wave64
constexpr uint32_t kCostMaxBlocks = kTreeCostPartialWords / 2u;  // 4 per CU: the pass is a stream, the rest of the range goes round the loop

__device__ __forceinline__ float quantum_of(uint32_t exps, int a) { return __uint_as_float(((exps >> (8 * a)) & 0xffu) << 23); }
// (d_x * d_y + d_y * d_z) + d_z * d_x
__device__ __forceinline__ float half_area(float dx, float dy, float dz) {
  const float xy = dx * dy, yz = dy * dz, zx = dz * dx;
  return (xy + yz) + zx;
}
__device__ __forceinline__ bool present(uint32_t ref) { return ref != kAbsent; }

// h_root of the tree whose root is `root` (§4.6 "Root"): the extent of its present children's planes, per axis
__device__ float root_half_area(const BvhNode4& root) {
  float d[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    int lo = 255, hi = 0;
    bool any = false;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (!present(root.ref[c])) continue;
      any = true;
      lo = min(lo, (int)((root.qlo[a] >> (8 * c)) & 0xffu));
      hi = max(hi, (int)((root.qhi[a] >> (8 * c)) & 0xffu));
    }
    d[a] = any ? (float)(hi - lo) * quantum_of(root.exps, a) : 0.0f;
  }
  return half_area(d[0], d[1], d[2]);
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, off, 64), hi = __shfl_xor((uint32_t)(v >> 32), off, 64);
    v += ((unsigned long long)hi << 32) | lo;
  }
  return v;
}

// the two sums of one workgroup's thread 0 (valid in thread 0 only)
__device__ __forceinline__ void block_sum(unsigned long long& a, unsigned long long& b) {
  __shared__ unsigned long long s_part[2][kCostBlock / 64u];
  a = wave_sum(a);
  b = wave_sum(b);
  if ((threadIdx.x & 63u) == 0u) { s_part[0][threadIdx.x >> 6] = a; s_part[1][threadIdx.x >> 6] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = 0ull; b = 0ull;
#pragma unroll
    for (uint32_t k = 0; k < kCostBlock / 64u; ++k) { a += s_part[0][k]; b += s_part[1][k]; }
  }
}

// partials[2 * block], [2 * block + 1] = this workgroup's share of the inner children's and of the leaf children's sum.  nodes: the tree's
// root; count >= 1 nodes.  Plain stores, one pair per workgroup, added up by k_tree_cost_sum: with one atomicAdd per workgroup and sum
// into a single pair of words the pass took 38.9 us on the 127 394-node tree of configs[3] (1 991 workgroups queueing at one L2 line),
// in this form 5.6 us + 1 to 6 us for the sum (profiles/tree_quality_kernel_trace.txt)
__global__ void __launch_bounds__(kCostBlock) k_tree_cost(const BvhNode4* __restrict__ nodes, uint32_t count, unsigned long long* __restrict__ partials) {
  __shared__ float s_root;
  if (threadIdx.x == 0) s_root = root_half_area(nodes[0]);
  __syncthreads();
  const float h_root = s_root;
  const bool valid = h_root > 0.0f;  // false for NaN as well
  const uint32_t slot = threadIdx.x & 3u, quad = threadIdx.x >> 2;
  unsigned long long node_q = 0ull, tri_q = 0ull;
  if (valid) {  // (uniform)
    const uint4* __restrict__ lines = reinterpret_cast<const uint4*>(nodes);
    for (uint32_t base = blockIdx.x * kCostNodesPerBlock; base < count; base += gridDim.x * kCostNodesPerBlock) {
      const uint32_t n = base + quad;
      const bool in = n < count;
      // lane `slot` of the quad holds words 4 * slot .. 4 * slot + 3 of the node: the wave reads 1 KiB in one piece
      uint4 w = make_uint4(0u, 0u, 0u, kAbsent);
      if (in) w = lines[(size_t)n * 4u + slot];
      const int q0 = (int)(threadIdx.x & 63u & ~3u);
      const uint32_t exps = __shfl(w.w, q0, 64);
      const uint32_t qlo0 = __shfl(w.x, q0 + 1, 64), qlo1 = __shfl(w.y, q0 + 1, 64), qlo2 = __shfl(w.z, q0 + 1, 64), qhi0 = __shfl(w.w, q0 + 1, 64);
      const uint32_t qhi1 = __shfl(w.x, q0 + 2, 64), qhi2 = __shfl(w.y, q0 + 2, 64);
      const uint32_t r0 = __shfl(w.x, q0 + 3, 64), r1 = __shfl(w.y, q0 + 3, 64), r2 = __shfl(w.z, q0 + 3, 64), r3 = __shfl(w.w, q0 + 3, 64);
      const uint32_t ref = slot == 0u ? r0 : (slot == 1u ? r1 : (slot == 2u ? r2 : r3));
      if (!in || !present(ref)) continue;  // (the shuffles are behind us: every lane took part)
      const uint32_t sh = 8u * slot;
      const float dx = (float)((int)((qhi0 >> sh) & 0xffu) - (int)((qlo0 >> sh) & 0xffu)) * quantum_of(exps, 0);
      const float dy = (float)((int)((qhi1 >> sh) & 0xffu) - (int)((qlo1 >> sh) & 0xffu)) * quantum_of(exps, 1);
      const float dz = (float)((int)((qhi2 >> sh) & 0xffu) - (int)((qlo2 >> sh) & 0xffu)) * quantum_of(exps, 2);
      const float rho = half_area(dx, dy, dz) / h_root;
      const unsigned long long q = rho >= 0.0f ? (unsigned long long)(fminf(rho, 4.0f) * 4294967296.0f) : 0ull;
      if (ref & kLeafRef) tri_q += q * (unsigned long long)(((ref >> 28) & 7u) + 1u);
      else node_q += q;
    }
  }
  block_sum(node_q, tri_q);
  if (threadIdx.x == 0) { partials[2u * blockIdx.x] = node_q; partials[2u * blockIdx.x + 1u] = tri_q; }
}

// one workgroup: out[0] = node_q, out[1] = tri_q, out[2] = valid from the `blocks` pairs k_tree_cost wrote.  Integer sums: their order
// does not show in the result
__global__ void __launch_bounds__(kCostBlock) k_tree_cost_sum(const BvhNode4* __restrict__ nodes, const unsigned long long* __restrict__ partials, uint32_t blocks,
                                                               unsigned long long* __restrict__ out) {
  unsigned long long node_q = 0ull, tri_q = 0ull;
  for (uint32_t k = threadIdx.x; k < blocks; k += kCostBlock) { node_q += partials[2u * k]; tri_q += partials[2u * k + 1u]; }
  block_sum(node_q, tri_q);
  if (threadIdx.x == 0) {
    const bool valid = root_half_area(nodes[0]) > 0.0f;
    out[0] = valid ? node_q + (1ull << 32) : 0ull;  // the root itself is visited
    out[1] = valid ? tri_q : 0ull;
    out[2] = valid ? 1ull : 0ull;
  }
}

}  // namespace

void launch_tree_cost(const BvhNode4* root, uint32_t node_count, unsigned long long* partials, unsigned long long* out3, hipStream_t s) {
  if (!node_count) return;
  const uint32_t blocks = std::min(kCostMaxBlocks, (node_count + kCostNodesPerBlock - 1u) / kCostNodesPerBlock);
  hipLaunchKernelGGL(k_tree_cost, dim3(blocks), dim3(kCostBlock), 0, s, root, node_count, partials);
  hipLaunchKernelGGL(k_tree_cost_sum, dim3(1), dim3(kCostBlock), 0, s, root, partials, blocks, out3);
}

}  // namespace rt
