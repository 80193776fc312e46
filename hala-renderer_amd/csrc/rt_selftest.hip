// rt_selftest.hip — hala_rt_selftest_math: the exact-math helpers of rt_math.h (rcp_rn, sqrt_rn) against the plain IEEE expressions they
// stand for, over any range of the 2^32 binary32 bit patterns.  A unary float function has few enough inputs to be proven by enumeration;
// tests/test_exact_math.py runs all of them.
#include <algorithm>

#include "../../include/halart.h"
#include "host_util.h"
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

}  // namespace rt

extern "C" {

int hala_rt_selftest_math(int which, uint32_t first, uint64_t count, uint64_t* mismatches, uint32_t* first_bad) {
  return rt::selftest_math(which, first, count, nullptr, nullptr, nullptr, mismatches, first_bad);
}
int hala_rt_selftest_math_values(int which, const uint32_t* patterns, uint32_t count, uint32_t* helper_bits, uint32_t* reference_bits,
                                 uint64_t* mismatches, uint32_t* first_bad) {
  if (count && !patterns) RT_FAIL("hala_rt_selftest_math_values: the pattern list is null!");
  return rt::selftest_math(which, 0u, count, patterns, helper_bits, reference_bits, mismatches, first_bad);
}

}  // extern "C"
