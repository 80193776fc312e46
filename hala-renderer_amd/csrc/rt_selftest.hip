// rt_selftest.hip — hala_rt_selftest_math: the exact-math helpers of rt_math.h (rcp_rn, sqrt_rn) against the plain IEEE expressions they
// stand for, over any range of the 2^32 binary32 bit patterns.  A unary float function has few enough inputs to be proven by enumeration;
// tests/test_exact_math.py runs all of them.  hala_rt_selftest_collapse: the collapse of bvh_build.hip on a binary tree the caller hands over
// (tests/test_collapse_cost.py against tests/collapse_ref.py).  hala_rt_selftest_hierarchy: one of its hierarchy builders on boxes the
// caller hands over (tests/test_hierarchy_builders.py against tests/hierarchy_ref.py).
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/halart.h"
#include "host_util.h"
#include "kernels.h"
#include "rt_math.h"

namespace rt {

template <int WHICH>
RT_DI float selftest_helper(float x) { return WHICH == 0 ? rcp_rn(x) : sqrt_rn(x); }
template <int WHICH>
RT_DI float selftest_reference(float x) { return WHICH == 0 ? 1.0f / x : sqrtf(x); }

// lane i takes patterns[i] (a list) or first + i (a range; the caller keeps first + count within 2^32).  Either output may be null.
template <int WHICH>
__global__ void k_selftest_math(uint32_t first, uint64_t count, const uint32_t* patterns, uint32_t* helper_bits, uint32_t* reference_bits,
                                unsigned long long* mismatches, uint32_t* first_bad) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  uint32_t bad = 0u, lowest = 0xffffffffu;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
    const uint32_t b = patterns ? patterns[i] : first + (uint32_t)i;
    const float x = __uint_as_float(b);
    const float h = selftest_helper<WHICH>(x), r = selftest_reference<WHICH>(x);
    if (helper_bits) helper_bits[i] = __float_as_uint(h);
    if (reference_bits) reference_bits[i] = __float_as_uint(r);
    if (__float_as_uint(h) != __float_as_uint(r) && !(h != h && r != r)) {  // two NaNs count as equal
      bad += 1u;
      lowest = b < lowest ? b : lowest;
    }
  }
  if (bad) {
    atomicAdd(mismatches, (unsigned long long)bad);
    atomicMin(first_bad, lowest);
  }
}

static int selftest_math(int which, uint32_t first, uint64_t count, const uint32_t* patterns, uint32_t* helper_bits, uint32_t* reference_bits,
                         uint64_t* mismatches, uint32_t* first_bad) {
  if (which != 0 && which != 1) RT_FAIL("hala_rt_selftest_math: which must be 0 (reciprocal) or 1 (square root).");
  if (!patterns && (uint64_t)first + count > (1ull << 32)) RT_FAIL("hala_rt_selftest_math: first + count exceeds 2^32.");
  if (patterns && count > (1ull << 28)) RT_FAIL("hala_rt_selftest_math_values: more than 2^28 patterns.");
  uint64_t bad = 0;
  uint32_t low = 0xffffffffu;
  if (count) {
    DeviceArray<unsigned long long> d_bad;
    DeviceArray<uint32_t> d_low, d_in, d_helper, d_ref;
    const unsigned long long zero = 0ull;
    RT_HIP(d_bad.upload(&zero, 1, nullptr));
    RT_HIP(d_low.upload(&low, 1, nullptr));
    if (patterns) {
      RT_HIP(d_in.upload(patterns, (size_t)count, nullptr));
      if (helper_bits) RT_HIP(d_helper.resize((size_t)count));
      if (reference_bits) RT_HIP(d_ref.resize((size_t)count));
    }
    const uint32_t block = 256u;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((count + block - 1u) / block, 16384u);
    if (which == 0) k_selftest_math<0><<<grid, block>>>(first, count, d_in.ptr, d_helper.ptr, d_ref.ptr, d_bad.ptr, d_low.ptr);
    else k_selftest_math<1><<<grid, block>>>(first, count, d_in.ptr, d_helper.ptr, d_ref.ptr, d_bad.ptr, d_low.ptr);
    RT_HIP(hipGetLastError());
    unsigned long long got = 0ull;
    RT_HIP(hipMemcpy(&got, d_bad.ptr, sizeof(got), hipMemcpyDeviceToHost));
    RT_HIP(hipMemcpy(&low, d_low.ptr, sizeof(low), hipMemcpyDeviceToHost));
    if (d_helper.ptr) RT_HIP(hipMemcpy(helper_bits, d_helper.ptr, (size_t)count * 4u, hipMemcpyDeviceToHost));
    if (d_ref.ptr) RT_HIP(hipMemcpy(reference_bits, d_ref.ptr, (size_t)count * 4u, hipMemcpyDeviceToHost));
    bad = got;
  }
  if (mismatches) *mismatches = bad;
  if (first_bad) *first_bad = low;
  return HALA_OK;
}

// The kernels index by what the tree says: nothing is uploaded before every reference, parent and range has been followed here.
static int selftest_collapse(const CollapseSelftest& job) {
  const uint32_t n = job.n;
  if (n < 2u || n > (1u << 20)) RT_FAIL("hala_rt_selftest_collapse: the tree must have 2 .. 2^20 leaves.");
  if (job.leaf_max < 1u || job.leaf_max > 8u || job.leaf_max >= n) RT_FAIL("hala_rt_selftest_collapse: leaf_max must be 1 .. 8 and below the leaf count.");
  if (!job.left || !job.right || !job.node_parent || !job.leaf_parent || !job.first || !job.last || !job.node_boxes || !job.leaf_boxes)
    RT_FAIL("hala_rt_selftest_collapse: an input array is null!");
  if (!all_finite(job.node_boxes, (size_t)(n - 1u) * 6u) || !all_finite(job.leaf_boxes, (size_t)n * 6u))
    RT_FAIL("hala_rt_selftest_collapse: a box is not finite.");
  const uint32_t leaf_bit = 0x80000000u;
  std::vector<uint8_t> node_seen(n - 1u, 0), leaf_seen(n, 0);
  std::vector<uint32_t> todo{0u};
  if (job.node_parent[0] != 0xffffffffu) RT_FAIL("hala_rt_selftest_collapse: node 0 must be the root.");
  node_seen[0] = 1;
  uint32_t nodes = 0, leaves = 0;
  while (!todo.empty()) {
    const uint32_t i = todo.back();
    todo.pop_back();
    ++nodes;
    uint32_t lo[2], hi[2];
    const uint32_t ref[2] = {job.left[i], job.right[i]};
    for (int side = 0; side < 2; ++side) {
      const uint32_t c = ref[side] & ~leaf_bit;
      if (ref[side] & leaf_bit) {
        if (c >= n || leaf_seen[c] || job.leaf_parent[c] != i) RT_FAIL("hala_rt_selftest_collapse: a leaf reference is out of range, repeated or has another parent.");
        leaf_seen[c] = 1; ++leaves;
        lo[side] = hi[side] = c;
      } else {
        if (c >= n - 1u || node_seen[c] || job.node_parent[c] != i) RT_FAIL("hala_rt_selftest_collapse: a node reference is out of range, repeated or has another parent.");
        node_seen[c] = 1; todo.push_back(c);
        lo[side] = job.first[c]; hi[side] = job.last[c];
      }
    }
    if (job.first[i] != lo[0] || job.last[i] != hi[1] || hi[0] + 1u != lo[1] || lo[0] > hi[0] || lo[1] > hi[1] || hi[1] >= n)
      RT_FAIL("hala_rt_selftest_collapse: a node's sorted positions are not those of its children, left then right.");
  }
  if (nodes != n - 1u || leaves != n) RT_FAIL("hala_rt_selftest_collapse: the root does not reach every node and leaf.");
  const std::string e = collapse_selftest(job);
  if (!e.empty()) RT_FAIL(e);
  return HALA_OK;
}

// The builders take any finite boxes; what they cannot take (an empty box, a pad that shrinks) is refused here, before any device call.
static int selftest_hierarchy(const HierarchySelftest& job) {
  const uint32_t n = job.n;
  if (n < 2u || n > (1u << 20)) RT_FAIL("hala_rt_selftest_hierarchy: there must be 2 .. 2^20 boxes.");
  if (!job.boxes || !job.sorted_ids || !job.left || !job.right || !job.first || !job.last || !job.node_parent || !job.leaf_parent || !job.node_boxes)
    RT_FAIL("hala_rt_selftest_hierarchy: an array is null!");
  if (!all_finite(job.boxes, (size_t)n * 6u)) RT_FAIL("hala_rt_selftest_hierarchy: a box is not finite.");
  for (size_t k = 0; k < n; ++k)
    for (int c = 0; c < 3; ++c)
      if (job.boxes[6 * k + c] > job.boxes[6 * k + 3 + c]) RT_FAIL("hala_rt_selftest_hierarchy: a box has min > max.");
  if (!std::isfinite(job.pad) || job.pad < 0.0f) RT_FAIL("hala_rt_selftest_hierarchy: pad must be finite and not negative.");
  if (job.builder < 1u || job.builder > 3u) RT_FAIL("hala_rt_selftest_hierarchy: builder must be 1 (SAH), 2 (PLOC) or 3 (LBVH).");
  if (job.ploc_tail > 2u || job.ploc_look_every > 64u) RT_FAIL("hala_rt_selftest_hierarchy: ploc_tail must be 0 .. 2 and ploc_look_every 0 .. 64.");
  const std::string e = hierarchy_selftest(job);
  if (!e.empty()) RT_FAIL(e);
  return HALA_OK;
}

}  // namespace rt

extern "C" {

int hala_rt_selftest_hierarchy(uint32_t count, const float* boxes, float pad, uint32_t builder, uint32_t ploc_tail, uint32_t ploc_look_every,
                               uint32_t* sorted_ids, uint32_t* left, uint32_t* right, uint32_t* first, uint32_t* last, uint32_t* node_parent,
                               uint32_t* leaf_parent, float* node_boxes) {
  return rt::selftest_hierarchy(rt::HierarchySelftest{count, boxes, pad, builder, ploc_tail, ploc_look_every, sorted_ids, left, right, first, last,
                                                      node_parent, leaf_parent, node_boxes});
}

int hala_rt_selftest_collapse(uint32_t leaves, uint32_t leaf_max, const uint32_t* left, const uint32_t* right, const uint32_t* node_parent,
                              const uint32_t* leaf_parent, const uint32_t* first, const uint32_t* last, const float* node_boxes,
                              const float* leaf_boxes, float* costs, uint32_t* choices, uint32_t* keep, uint32_t* refs4, uint32_t* node_count,
                              uint32_t* levels) {
  return rt::selftest_collapse(rt::CollapseSelftest{leaves, leaf_max, left, right, node_parent, leaf_parent, first, last, node_boxes, leaf_boxes, costs,
                                                    choices, keep, refs4, node_count, levels});
}

int hala_rt_selftest_math(int which, uint32_t first, uint64_t count, uint64_t* mismatches, uint32_t* first_bad) {
  return rt::selftest_math(which, first, count, nullptr, nullptr, nullptr, mismatches, first_bad);
}
int hala_rt_selftest_math_values(int which, const uint32_t* patterns, uint32_t count, uint32_t* helper_bits, uint32_t* reference_bits,
                                 uint64_t* mismatches, uint32_t* first_bad) {
  if (count && !patterns) RT_FAIL("hala_rt_selftest_math_values: the pattern list is null!");
  return rt::selftest_math(which, 0u, count, patterns, helper_bits, reference_bits, mismatches, first_bad);
}

}  // extern "C"
