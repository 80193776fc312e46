// bvh_node_pack.h — the one place that turns up to four child boxes into a 64-B compressed node (RENDER_SPEC §4.1b).  Host and device:
// the GPU builders (bvh_build.hip: k_refit_level, k_emit_single4) and the host-built instance levels (bvh_tlas.cpp) emit the same bytes
// for the same boxes.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "hala_types.h"

namespace rt {

#define RT_HDI __host__ __device__ __forceinline__

struct Box6 {
  float mn[3], mx[3];
};
RT_HDI Box6 box_union(const Box6& a, const Box6& b) {
  Box6 r;
#pragma unroll
  for (int k = 0; k < 3; ++k) { r.mn[k] = fminf(a.mn[k], b.mn[k]); r.mx[k] = fmaxf(a.mx[k], b.mx[k]); }
  return r;
}

struct Child4 { Box6 box; uint32_t ref; };

// quantum exponent of one axis: the smallest power of two s = 2^e with extent / s <= 255 (never below 2^-100).  Read from the double's
// bits: q = m * 2^e with m in [0.5, 1), so 2^e > q or m == 0.5 — what frexp returns for every q a float extent can produce (the
// smallest positive one is 2^-149 / 255 > 2^-157: a normal double, its exponent field is never 0).
RT_HDI int quantum_exponent(float lo, float hi) {
  const double q = ((double)hi - (double)lo) / 255.0;
  if (!(q > 0.0)) return -100;
  const int e = (int)((__builtin_bit_cast(long long, q) >> 52) & 0x7ff) - 1022;
  return e < -100 ? -100 : (e > 100 ? 100 : e);
}

// n >= 1 children, in slot order; the slots behind them are absent
RT_HDI BvhNode4 pack_node4(const Child4* ch, int n) {
  BvhNode4 nd{};
  Box6 all = ch[0].box;
  for (int c = 1; c < n; ++c) all = box_union(all, ch[c].box);
  int e[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    nd.pmin[a] = all.mn[a];
    e[a] = quantum_exponent(all.mn[a], all.mx[a]);
    nd.exps |= (uint32_t)(e[a] + 127) << (8 * a);
  }
  for (int c = 0; c < 4; ++c) {
    if (c >= n) { nd.ref[c] = kAbsent; continue; }
    nd.ref[c] = ch[c].ref;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double s = __builtin_bit_cast(double, (long long)(e[a] + 1023) << 52), base = (double)all.mn[a];
      double lo = floor(((double)ch[c].box.mn[a] - base) / s), hi = ceil(((double)ch[c].box.mx[a] - base) / s);
      if (base + lo * s > (double)ch[c].box.mn[a]) lo -= 1.0;  // rounding of the subtraction must not shrink the box
      if (base + hi * s < (double)ch[c].box.mx[a]) hi += 1.0;
      lo = fmin(fmax(lo, 0.0), 255.0); hi = fmin(fmax(hi, 0.0), 255.0);
      nd.qlo[a] |= (uint32_t)lo << (8 * c);
      nd.qhi[a] |= (uint32_t)hi << (8 * c);
    }
  }
  return nd;
}

}  // namespace rt
