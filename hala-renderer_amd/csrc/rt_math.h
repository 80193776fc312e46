// rt_math.h — device-side scalar float32 building blocks of docs/RENDER_SPEC.md §2 for the HIP kernels.
//
// Determinism contract: compiled with -ffp-contract=off, every expression below is a fixed sequence of IEEE
// binary32 operations (+ - * / sqrt and explicit __fmaf_rn), so a kernel's result is a pure function of its
// inputs and independent of traversal/scheduling order.  tests/ hold these kernels to the CPU oracle bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rt {

struct f3 {
  float x, y, z;
};

#define RT_DI __device__ __forceinline__

RT_DI f3 mk3(float x, float y, float z) { return f3{x, y, z}; }
RT_DI f3 splat3(float s) { return f3{s, s, s}; }
RT_DI f3 ld3(const float* p) { return f3{p[0], p[1], p[2]}; }
RT_DI f3 operator+(f3 a, f3 b) { return f3{a.x + b.x, a.y + b.y, a.z + b.z}; }
RT_DI f3 operator-(f3 a, f3 b) { return f3{a.x - b.x, a.y - b.y, a.z - b.z}; }
RT_DI f3 operator*(f3 a, f3 b) { return f3{a.x * b.x, a.y * b.y, a.z * b.z}; }
RT_DI f3 operator*(f3 a, float s) { return f3{a.x * s, a.y * s, a.z * s}; }
RT_DI f3 operator-(f3 a) { return f3{-a.x, -a.y, -a.z}; }

// 1.0f / x and sqrtf(x), bit for bit, in fewer issue slots.  hipcc's correctly rounded `/` is a dozen vector instructions (two
// v_div_scale, v_rcp_f32, a chain of fma, v_div_fmas, v_div_fixup); one Newton step on v_rcp_f32, with the residual taken by an fma, already
// rounds correctly wherever x, 1/x and the residual stay normal.  That is decided by enumeration, not by argument:
// hala_rt_selftest_math runs all 2^32 inputs through the helper and through the plain expression (tests/test_exact_math.py), and
// profiles/exact_math.txt holds the sweep of the unguarded forms from which the windows below were read.  Inputs outside the window
// (zeros, denormals, infinities, NaNs, quotients that are denormal) take the plain expression, behind a branch that a wave skips unless
// one of its lanes needs it.
//
// rcp_rn: the unguarded form differs from 1.0f / x for biased exponents 0, 253 (all but +-2^126), 254 and for +-inf, and for no other
// input, all-ones mantissas included: the window is 2^-126 <= |x| < 2^126.  The shift drops the sign; one unsigned compare tests both ends.
// v_rcp_f32 counted double, the fast path is 6 issue slots (v_rcp_f32, v_lshl_add_u32, v_cmp_gt_u32, two fma) against 12.
RT_DI float rcp_rn(float x) {
  const float r0 = __builtin_amdgcn_rcpf(x);
  const float e = __fmaf_rn(-x, r0, 1.0f);
  float r = __fmaf_rn(e, r0, r0);
  if (__builtin_expect(((__float_as_uint(x) << 1) - 0x01000000u) >= 0xfc000000u, 0)) r = 1.0f / x;
  return r;
}
// sqrt_rn: y = v_rsq_f32(x), g = x y, then one step on the residual x - g g (exact in the fma) with slope y / 2.  The unguarded form
// differs from sqrtf(x) for biased exponents 0 ... 24 (the residual, about 2^-24 x, leaves the normal range), for +inf, and for no other
// input (negative inputs give NaN on both sides); the window starts a little above that, at 2^-95, and ends below +inf: one subtraction
// and one unsigned compare, which negative inputs fail as well.  8 issue slots against the 17 of hipcc's correctly rounded sqrtf.
RT_DI float sqrt_rn(float x) {
  const float y = __builtin_amdgcn_rsqf(x);
  const float g = x * y;
  const float h = 0.5f * y;
  const float d = __fmaf_rn(-g, g, x);
  float s = __fmaf_rn(d, h, g);
  if (__builtin_expect((__float_as_uint(x) - 0x10000000u) >= 0x6f800000u, 0)) s = sqrtf(x);
  return s;
}

// §2.1
RT_DI float dot3(f3 a, f3 b) { return __fmaf_rn(a.z, b.z, __fmaf_rn(a.y, b.y, a.x * b.x)); }
RT_DI f3 cross3(f3 a, f3 b) {
  return f3{__fmaf_rn(a.y, b.z, -(a.z * b.y)), __fmaf_rn(a.z, b.x, -(a.x * b.z)), __fmaf_rn(a.x, b.y, -(a.y * b.x))};
}
RT_DI f3 madd3(f3 d, float t, f3 o) { return f3{__fmaf_rn(d.x, t, o.x), __fmaf_rn(d.y, t, o.y), __fmaf_rn(d.z, t, o.z)}; }
RT_DI f3 normalize3(f3 a) {
  float inv = rcp_rn(sqrt_rn(dot3(a, a)));
  return a * inv;
}
RT_DI float maxf(float a, float b) { return a > b ? a : b; }
RT_DI float minf(float a, float b) { return a < b ? a : b; }
// IEEE-754 minNum / maxNum with -0 < +0: ONE v_min_f32 / v_max_f32 (the select forms above cost a compare and a
// select each); used where the spec says so (RENDER_SPEC §4.3b: the slab tests of the compressed BVH4 nodes)
RT_DI float hw_minf(float a, float b) { return __builtin_fminf(a, b); }
RT_DI float hw_maxf(float a, float b) { return __builtin_fmaxf(a, b); }
RT_DI float clampf(float x, float lo, float hi) { return minf(maxf(x, lo), hi); }
RT_DI float max3f(f3 a) { return maxf(a.x, maxf(a.y, a.z)); }

constexpr float kPi = 3.14159265358979323846f;
constexpr float kInvPi = 0.31830988618379067154f;
constexpr float kInvTwoPi = 0.15915494309189533577f;
constexpr float kHalfPi = 1.57079632679489661923f;
constexpr float kTwoPiSq = 19.7392088021787172376f;

// §2.2 polynomial trigonometry
RT_DI float sin_poly(float a) {
  float a2 = a * a;
  float p = -2.50521083854417187751e-8f;
  p = __fmaf_rn(p, a2, 2.75573192239858906526e-6f);
  p = __fmaf_rn(p, a2, -1.98412698412698412698e-4f);
  p = __fmaf_rn(p, a2, 8.33333333333333333333e-3f);
  p = __fmaf_rn(p, a2, -1.66666666666666666667e-1f);
  p = __fmaf_rn(p, a2, 1.0f);
  return a * p;
}
RT_DI float cos_poly(float a) {
  float a2 = a * a;
  float p = 2.08767569878680989792e-9f;
  p = __fmaf_rn(p, a2, -2.75573192239858906526e-7f);
  p = __fmaf_rn(p, a2, 2.48015873015873015873e-5f);
  p = __fmaf_rn(p, a2, -1.38888888888888888889e-3f);
  p = __fmaf_rn(p, a2, 4.16666666666666666667e-2f);
  p = __fmaf_rn(p, a2, -0.5f);
  p = __fmaf_rn(p, a2, 1.0f);
  return p;
}
RT_DI void sincos_2pi(float u, float* s, float* c) {
  float x = u * 4.0f;
  int q = (int)x;
  float f = x - (float)q;
  float a = f * kHalfPi;
  float sa = sin_poly(a), ca = cos_poly(a);
  q &= 3;
  *s = q == 0 ? sa : (q == 1 ? ca : (q == 2 ? -sa : -ca));
  *c = q == 0 ? ca : (q == 1 ? -sa : (q == 2 ? -ca : sa));
}
// e^x for x <= 0 (RENDER_SPEC §2.2): 2^(x log2 e) = 2^n 2^f, n = floor, f in [0,1); 2^f = e^(f ln 2) by its Taylor polynomial
// to the 8th power (relative error < 3e-8 before rounding); the scale by 2^n is exact.  Arguments >= 0 (and NaN) give 1.
RT_DI float exp_neg_poly(float x) {
  if (!(x < 0.0f)) return 1.0f;
  float y = x * 1.44269504088896340736f;
  if (y < -126.0f) return 0.0f;
  float n = floorf(y);
  float g = (y - n) * 0.69314718055994530942f;
  float p = 2.48015873015873015873e-5f;
  p = __fmaf_rn(p, g, 1.98412698412698412698e-4f);
  p = __fmaf_rn(p, g, 1.38888888888888888889e-3f);
  p = __fmaf_rn(p, g, 8.33333333333333333333e-3f);
  p = __fmaf_rn(p, g, 4.16666666666666666667e-2f);
  p = __fmaf_rn(p, g, 1.66666666666666666667e-1f);
  p = __fmaf_rn(p, g, 0.5f);
  p = __fmaf_rn(p, g, 1.0f);
  p = __fmaf_rn(p, g, 1.0f);
  return p * __uint_as_float((uint32_t)((int)n + 127) << 23);
}
// ln x for a positive normal float (RENDER_SPEC §7.1f): x = m 2^e with m in [sqrt(1/2), sqrt 2); z = (m-1)/(m+1);
// ln m = 2z (1 + z^2/3 + z^4/5 + z^6/7 + z^8/9) (|z| <= 0.172: truncation < 2e-9); ln x = fma(e, ln 2, ln m).
RT_DI float log_poly(float x) {
  const uint32_t b = __float_as_uint(x);
  int e = (int)(b >> 23) - 127;
  float m = __uint_as_float((b & 0x007fffffu) | 0x3f800000u);
  if (m > 1.41421356237f) { m = m * 0.5f; e += 1; }
  const float z = (m - 1.0f) / (m + 1.0f);
  const float z2 = z * z;
  float p = 0.11111111111111111f;
  p = __fmaf_rn(p, z2, 0.14285714285714285f);
  p = __fmaf_rn(p, z2, 0.2f);
  p = __fmaf_rn(p, z2, 0.33333333333333333f);
  p = __fmaf_rn(p, z2, 1.0f);
  return __fmaf_rn((float)e, 0.69314718055994530942f, (2.0f * z) * p);
}
RT_DI float acos_poly(float x) {
  float ax = fabsf(x);
  if (ax > 1.0f) ax = 1.0f;
  float p = -0.0012624911f;
  p = __fmaf_rn(p, ax, 0.0066700901f);
  p = __fmaf_rn(p, ax, -0.0170881256f);
  p = __fmaf_rn(p, ax, 0.0308918810f);
  p = __fmaf_rn(p, ax, -0.0501743046f);
  p = __fmaf_rn(p, ax, 0.0889789874f);
  p = __fmaf_rn(p, ax, -0.2145988016f);
  p = __fmaf_rn(p, ax, 1.5707963050f);
  float r = sqrt_rn(1.0f - ax) * p;
  return x < 0.0f ? kPi - r : r;
}
RT_DI float atan_poly01(float z) {
  float z2 = z * z;
  float p = 0.0028662257f;
  p = __fmaf_rn(p, z2, -0.0161657367f);
  p = __fmaf_rn(p, z2, 0.0429096138f);
  p = __fmaf_rn(p, z2, -0.0752896400f);
  p = __fmaf_rn(p, z2, 0.1065626393f);
  p = __fmaf_rn(p, z2, -0.1420889944f);
  p = __fmaf_rn(p, z2, 0.1999355085f);
  p = __fmaf_rn(p, z2, -0.3333314528f);
  p = __fmaf_rn(p, z2, 1.0f);
  return z * p;
}
RT_DI float atan2_poly(float y, float x) {
  float ax = fabsf(x), ay = fabsf(y);
  float mx = maxf(ax, ay), mn = minf(ax, ay);
  if (mx == 0.0f) return 0.0f;
  float a = atan_poly01(mn / mx);
  if (ay > ax) a = kHalfPi - a;
  if (x < 0.0f) a = kPi - a;
  return y < 0.0f ? -a : a;
}

// §2.3 RNG
RT_DI uint32_t pcg_hash(uint32_t v) {
  uint32_t state = v * 747796405u + 2891336453u;
  uint32_t word = ((state >> ((state >> 28u) + 4u)) ^ state) * 277803737u;
  return (word >> 22u) ^ word;
}
RT_DI uint32_t rng_init(uint32_t pixel_id, uint32_t frame_index) {
  return pcg_hash(pixel_id + pcg_hash(frame_index * 0x9E3779B9u + 0x85EBCA6Bu));
}
RT_DI float rng_next(uint32_t& s) {
  uint32_t x = pcg_hash(s);
  s += 1u;
  return (float)(x >> 8) * (1.0f / 16777216.0f);
}

// §2.4 frames and sampling
RT_DI void onb(f3 n, f3* t, f3* b) {
  float sign = copysignf(1.0f, n.z);
  float a = -1.0f / (sign + n.z);
  float bb = n.x * n.y * a;
  *t = f3{1.0f + sign * n.x * n.x * a, sign * bb, -sign * n.x};
  *b = f3{bb, sign + n.y * n.y * a, -n.y};
}
RT_DI f3 to_world(f3 l, f3 t, f3 b, f3 n) {
  return f3{__fmaf_rn(n.x, l.z, __fmaf_rn(b.x, l.y, t.x * l.x)), __fmaf_rn(n.y, l.z, __fmaf_rn(b.y, l.y, t.y * l.x)),
            __fmaf_rn(n.z, l.z, __fmaf_rn(b.z, l.y, t.z * l.x))};
}
RT_DI f3 cosine_hemisphere(float u1, float u2) {
  float r = sqrt_rn(u1);
  float s, c;
  sincos_2pi(u2, &s, &c);
  return f3{r * c, r * s, sqrt_rn(maxf(0.0f, 1.0f - u1))};
}
// Henyey-Greenstein direction around the unit vector d (RENDER_SPEC §7.1f)
RT_DI f3 hg_sample(f3 d, float g, float u1, float u2) {
  g = minf(maxf(g, -0.99f), 0.99f);
  float ct;
  if (fabsf(g) < 1e-3f) ct = 1.0f - 2.0f * u1;
  else {
    const float q = (1.0f - g * g) / ((1.0f - g) + (2.0f * g) * u1);
    ct = ((1.0f + g * g) - q * q) / (2.0f * g);
  }
  ct = minf(maxf(ct, -1.0f), 1.0f);
  const float st = sqrt_rn(maxf(0.0f, 1.0f - ct * ct));
  float s, c;
  sincos_2pi(u2, &s, &c);
  f3 t, b;
  onb(d, &t, &b);
  return to_world(f3{st * c, st * s, ct}, t, b, d);
}
// Henyey-Greenstein phase function (= the pdf of hg_sample) for the cosine c between the propagation direction and the new one
RT_DI float hg_phase(float g, float c) {
  g = minf(maxf(g, -0.99f), 0.99f);
  if (fabsf(g) < 1e-3f) return 0.07957747154594767f;  // 1 / (4 pi)
  c = minf(maxf(c, -1.0f), 1.0f);
  const float g2 = g * g;
  const float x = (1.0f + g2) - (2.0f * g) * c;
  return (1.0f - g2) / (12.566370614359172f * (x * sqrt_rn(x)));
}
RT_DI float luminance(f3 c) { return 0.212671f * c.x + 0.715160f * c.y + 0.072169f * c.z; }
RT_DI float power_heuristic(float a, float b) {
  float a2 = a * a;
  return a2 / (a2 + b * b);
}

// §4.3 ray preparation shared by both traversal kernels
RT_DI float safe_inv(float d) {
  float dd = fabsf(d) < 1e-20f ? copysignf(1e-20f, d) : d;
  return rcp_rn(dd);
}

// Streaming stores (queue entries, hit records): written once, read by the next launch at the earliest — nontemporal stores keep
// them from displacing what the traversal and shading gathers want in L2 (+1.4 ... 2.2 % on the headline).  The 12-B per-path
// records stay ordinary stores: three scalar nontemporal stores each measured slower.
typedef float v4f_nt __attribute__((ext_vector_type(4)));
RT_DI void st4(float4* p, float4 v) { __builtin_nontemporal_store(v4f_nt{v.x, v.y, v.z, v.w}, reinterpret_cast<v4f_nt*>(p)); }

// wave64 helpers ------------------------------------------------------------------------------------------
RT_DI uint32_t lane_id() { return threadIdx.x & 63u; }
RT_DI uint32_t wave_sum(uint32_t v) {
  for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_down((int)v, off);
  return v;  // valid in lane 0
}
RT_DI uint32_t mbcnt64(unsigned long long m) {  // number of set bits of m below this lane
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// LDS is addressed through explicit address-space-3 pointers to builtin vectors: a generic pointer kept in a struct makes hipcc emit
// flat_load / flat_store (both memory pipes, both wait counters) instead of ds_read / ds_write.
#define RT_LDS __attribute__((address_space(3)))

}  // namespace rt
