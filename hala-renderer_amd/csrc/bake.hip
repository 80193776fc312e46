// bake.hip — bake maps (RENDER_SPEC 4.11): one instance rasterised into its own texture space.  Every texel of a W x H map whose centre a
// triangle of the instance covers in UV space becomes an occlusion sample (RENDER_SPEC 4.10) at the surface point and normal found there;
// the occlusion kernels of occlusion.hip then answer the sample buffer as they answer any other, and a dilation pass fills the gutters.
// Nothing here walks the tree: the inputs are the shading records (UVs, vertex normals, instance) and the triangle records in global-id
// order.  Five kernels:
//   k_bake_count   one lane per triangle: how many 8 x 8 texel blocks its clipped bounding box spans (a prefix sum over them follows)
//   k_bake_cover   one (triangle, block) pair per wave step, one texel per lane: the coverage test, atomicMin of the global id
//   k_bake_sample  one lane per texel: owner -> edge values again -> (u, v), point, normal -> the 32-B sample and the 16-B texel record
//   k_bake_blocks  one wave per 8 x 8 block: its 64 ownership bits as one word (what the dilation rejects empty windows by)
//   k_bake_dilate  one lane per texel: an ownerless texel takes the record of the nearest owned texel of its window
// Bake atlases (RENDER_SPEC 4.12) put several instances into one map, each through a chart (scale, offset, flags): k_bake_atlas_count /
// _cover / _sample are the first three kernels with the chart between the UVs and the corners, and k_bake_list_count / k_bake_list turn
// the ownership words into the list of owned texels that the listed occlusion pass of occlusion.hip traces.
// Transfer bakes (RENDER_SPEC 4.13) use the rasteriser as it is and k_bake_dilate_transfer, the dilation on their 32-B records.
// The owner map is tiled 8 x 8 (a block is 256 B: two lines, one atomic instruction per wave step); its layout is not observable.
// The library is built with -ffp-contract=off: the only fused operations are the ones written as __fmaf_rn, here the three of `point`
// and those inside dot3 / cross3 / transform_normal (shading.h, rt_math.h), which the spec names.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "kernels.h"
#include "shading.h"
#include "variants.h"

namespace rt {

struct f2 { float x, y; };
// RENDER_SPEC 4.11: every difference and every product rounded, one subtraction, no fma
RT_DI float bake_e(f2 a, f2 b, f2 p) { return (b.x - a.x) * (p.y - a.y) - (b.y - a.y) * (p.x - a.x); }
// ... with the endpoints in canonical order, so that the two triangles of a shared edge compute the same number with opposite sign
RT_DI float bake_edge(f2 a, f2 b, f2 p) {
  const bool swap = a.x > b.x || (a.x == b.x && a.y > b.y);
  return swap ? -bake_e(b, a, p) : bake_e(a, b, p);
}
struct BakeTri { f2 a, b, c; float area; };
RT_DI BakeTri bake_tri(const SceneView& sv, const BakeView& bv, uint32_t gid) {
  const float4* sp = reinterpret_cast<const float4*>(sv.shade_tris + gid);
  const float4 s4 = sp[4], s5 = sp[5];  // line 2 of the shading record: uv[3][2], then the tangents
  const float w = (float)bv.width, h = (float)bv.height;
  BakeTri t;
  t.a = f2{s4.x * w, s4.y * h}; t.b = f2{s4.z * w, s4.w * h}; t.c = f2{s5.x * w, s5.y * h};
  t.area = bake_edge(t.a, t.b, t.c);
  return t;
}
// RENDER_SPEC 4.12: the corners through the chart of the triangle's instance (the shading record's s0.w), one fma and then one product per
// component; an instance without a chart gets area 0, which covers nothing and counts no pairs.  *flags: the chart's.
RT_DI BakeTri bake_tri_atlas(const SceneView& sv, const BakeView& bv, const BakeChartDev* __restrict__ charts, uint32_t gid) {
  const float4* sp = reinterpret_cast<const float4*>(sv.shade_tris + gid);
  const float4* cp = reinterpret_cast<const float4*>(charts + __float_as_uint(sp[0].w));
  const float4 so = cp[0], fc = cp[1];  // (scale, offset), (-, charted, -, -)
  BakeTri t;
  if (__float_as_uint(fc.y) == 0u) {
    t.a = t.b = t.c = f2{0.0f, 0.0f}; t.area = 0.0f;
    return t;
  }
  const float4 s4 = sp[4], s5 = sp[5];
  const float w = (float)bv.width, h = (float)bv.height;
  t.a = f2{__fmaf_rn(s4.x, so.x, so.z) * w, __fmaf_rn(s4.y, so.y, so.w) * h};
  t.b = f2{__fmaf_rn(s4.z, so.x, so.z) * w, __fmaf_rn(s4.w, so.y, so.w) * h};
  t.c = f2{__fmaf_rn(s5.x, so.x, so.z) * w, __fmaf_rn(s5.y, so.y, so.w) * h};
  t.area = bake_edge(t.a, t.b, t.c);
  return t;
}
RT_DI bool bake_covers(const BakeTri& t, f2 p, float* w1, float* w2) {
  const float w0 = bake_edge(t.b, t.c, p);
  *w1 = bake_edge(t.c, t.a, p); *w2 = bake_edge(t.a, t.b, p);
  return (t.area > 0.0f && w0 >= 0.0f && *w1 >= 0.0f && *w2 >= 0.0f) || (t.area < 0.0f && w0 <= 0.0f && *w1 <= 0.0f && *w2 <= 0.0f);
}
// The 8 x 8 blocks a triangle's pairs run over.  An optimisation only: it must never leave out a texel the rounded test accepts, and the
// rounded test accepts centres outside the triangle, beyond the tips of thin triangles most of all.  The bound (eps = 2^-24, ext = the
// larger side of the corners' box, unclamped, |area| the edge value of the corners: twice the triangle's):
//   an edge value at P carries at most 4 eps (|d1 d2| + |d3 d4|) <= 8 eps * (edge's larger component) * R of error, R the largest
//   component of P - anchor, so P passes a half-plane it is outside of only within tau = 8 eps R of that edge's LINE, and R <= ext + D
//   for a P that is D outside the box;
//   a centre outside the triangle fails one or two half-planes.  Within tau of one line with its foot on the edge it is within tau of the
//   triangle; otherwise it is within tau of two lines that cross at a corner, or within tau of one beyond a corner and inside the other,
//   and then within 2 tau / sin(angle) of that corner, where sin(angle) = |area| / (the two sides' lengths) >= |area| / (2 ext^2);
//   so D <= 32 eps ext^2 (ext + D) / |area| = (k / 2) (ext + D) with k = 64 eps ext^2 / |area| (the exact area is within 8 eps ext^2 of
//   the rounded one, which k's spare factor 2 absorbs), and D <= k ext whenever k < 1/2.
// The box is the corners' box widened by 2 k ext (and by the half texel of a centre and a quarter for the float roundings of the box
// itself) while k < 1/2; from there on — a needle whose thinness is within 2^-17 of its length squared, coordinates that overflow, a
// NaN k, and sides below 2^-40 texels, where products go subnormal and eps bounds nothing — every block of the map.  Every clamp is made
// in float, ahead of the conversion.  A zero or NaN area covers nothing (a NaN coordinate makes the area NaN).
struct BakeBox { uint32_t bx0, by0, nbx, nby; };
RT_DI BakeBox bake_box(const BakeTri& t, const BakeView& bv) {
  BakeBox bb{0u, 0u, 0u, 0u};
  if (!(t.area > 0.0f || t.area < 0.0f)) return bb;
  const float minx = fminf(fminf(t.a.x, t.b.x), t.c.x), maxx = fmaxf(fmaxf(t.a.x, t.b.x), t.c.x);
  const float miny = fminf(fminf(t.a.y, t.b.y), t.c.y), maxy = fmaxf(fmaxf(t.a.y, t.b.y), t.c.y);
  const float ext = fmaxf(maxx - minx, maxy - miny);
  const float k = ext * ext * (1.0f / 262144.0f) / fabsf(t.area);
  uint32_t x0 = 0u, x1 = bv.width - 1u, y0 = 0u, y1 = bv.height - 1u;
  if (ext >= 0x1p-40f && k < 0.5f) {
    const float pad = 2.0f * k * ext + 0.75f;
    const float lx = fmaxf(minx - pad, 0.0f), hx = fminf(maxx + pad, (float)bv.width), ly = fmaxf(miny - pad, 0.0f), hy = fminf(maxy + pad, (float)bv.height);
    if (!(lx <= hx && ly <= hy)) return bb;  // off the map
    x0 = min((uint32_t)lx, x1); x1 = min((uint32_t)hx, x1);
    y0 = min((uint32_t)ly, y1); y1 = min((uint32_t)hy, y1);
  }
  bb.bx0 = x0 >> 3; bb.nbx = (x1 >> 3) - bb.bx0 + 1u;
  bb.by0 = y0 >> 3; bb.nby = (y1 >> 3) - bb.by0 + 1u;
  return bb;
}
RT_DI uint32_t bake_tiled(const BakeView& bv, uint32_t x, uint32_t y) { return (((y >> 3) * bv.blocks_x + (x >> 3)) << 6) + ((y & 7u) << 3) + (x & 7u); }

// counts[i] for i < n, and a 0 at n: the exclusive sum over n + 1 entries leaves the number of pairs at [n]
__global__ void __launch_bounds__(256) k_bake_count(SceneView sv, BakeView bv, unsigned long long* __restrict__ counts) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > bv.tri_count) return;
  unsigned long long c = 0ull;
  if (i < bv.tri_count) {
    const BakeBox bb = bake_box(bake_tri(sv, bv, bv.first_tri + i), bv);
    c = (unsigned long long)bb.nbx * bb.nby;
  }
  counts[i] = c;
}

// Every wave takes an equal run of consecutive pairs: it finds the triangle of its first pair by bisection of the offsets and walks on
// from there, so a triangle's record is read once per run and the blocks of a run are neighbours.  The number of pairs is known on the
// device alone (no host synchronisation): the grid is fixed, the run length follows from it.
__global__ void __launch_bounds__(256) k_bake_cover(SceneView sv, BakeView bv, const unsigned long long* __restrict__ off, uint32_t* __restrict__ owner) {
  const uint32_t lane = lane_id();
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, waves = (gridDim.x * blockDim.x) >> 6;
  const unsigned long long total = off[bv.tri_count];
  const unsigned long long run = (total + waves - 1ull) / waves;
  unsigned long long p = (unsigned long long)wave * run;
  const unsigned long long end = p + run < total ? p + run : total;
  if (p >= end) return;
  uint32_t lo = 0u, hi = bv.tri_count;  // off[lo] <= p < off[hi]
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (off[mid] <= p) lo = mid; else hi = mid;
  }
  uint32_t t = lo;
  unsigned long long t_begin = off[t], t_end = off[t + 1u];
  BakeTri tri = bake_tri(sv, bv, bv.first_tri + t);
  BakeBox bb = bake_box(tri, bv);
  for (; p < end; ++p) {
    if (p >= t_end) {
      do { ++t; t_begin = t_end; t_end = off[t + 1u]; } while (p >= t_end);  // (t < tri_count: p < total = off[tri_count])
      tri = bake_tri(sv, bv, bv.first_tri + t);
      bb = bake_box(tri, bv);
    }
    const uint32_t k = (uint32_t)(p - t_begin);
    const uint32_t row = k / bb.nbx, bx = bb.bx0 + (k - row * bb.nbx), by = bb.by0 + row;
    const uint32_t x = (bx << 3) + (lane & 7u), y = (by << 3) + (lane >> 3);
    if (x >= bv.width || y >= bv.height) continue;
    float w1, w2;
    if (bake_covers(tri, f2{(float)x + 0.5f, (float)y + 0.5f}, &w1, &w2)) atomicMin(owner + (((size_t)by * bv.blocks_x + bx) << 6) + lane, bv.first_tri + t);
  }
}

// One lane per texel, a wave per 64 consecutive texels of the row-major map.  A sample is two 16-B words, (point, bias) and (normal,
// reach): the wave exchanges them so that each of its two store instructions writes 1 KiB without a gap.
__global__ void __launch_bounds__(256) k_bake_sample(SceneView sv, BakeView bv, const uint32_t* __restrict__ owner, float4* __restrict__ samples,
                                                     uint4* __restrict__ texels) {
  const uint32_t count = bv.width * bv.height;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, lane = lane_id();
  float4 pb = make_float4(0.0f, 0.0f, 0.0f, 0.0f), nr = pb;  // the all-zero sample: invalid by RENDER_SPEC 4.10
  uint4 rec = make_uint4(0u, 0u, kAbsent, kAbsent);
  if (i < count) {
    const uint32_t y = i / bv.width, x = i - y * bv.width;
    const uint32_t gid = owner[bake_tiled(bv, x, y)];
    if (gid != kAbsent) {
      const BakeTri tri = bake_tri(sv, bv, gid);
      float w1, w2;
      (void)bake_covers(tri, f2{(float)x + 0.5f, (float)y + 0.5f}, &w1, &w2);
      const float inv = 1.0f / tri.area;
      const float u = w1 * inv, v = w2 * inv;
      const float4* tp = reinterpret_cast<const float4*>(sv.tris_by_id + gid);
      const float4 t0 = tp[0], t1 = tp[1], t2 = tp[2];
      const f3 v0 = mk3(t0.x, t0.y, t0.z), e1 = mk3(t1.x, t1.y, t1.z), e2 = mk3(t2.x, t2.y, t2.z);
      const f3 point = madd3(e2, v, madd3(e1, u, v0));  // RENDER_SPEC 4.8's q
      f3 n;
      if (bv.flags & HALA_BAKE_SHADING_NORMAL) {  // RENDER_SPEC 6 step 4, in the form of make_surface (shading.h)
        const float4* sp = reinterpret_cast<const float4*>(sv.shade_tris + gid);
        const float4 s0 = sp[0], s1 = sp[1], s2 = sp[2], s3 = sp[3];
        const float w0 = 1.0f - u - v;
        const f3 nl = madd3(mk3(s3.x, s3.y, s3.z), v, madd3(mk3(s2.x, s2.y, s2.z), u, mk3(s1.x, s1.y, s1.z) * w0));
        n = normalize3(transform_normal(sv.primitives[__float_as_uint(s0.w)].transform, nl));
      } else n = cross3(e1, e2);
      if (bv.flags & HALA_BAKE_FLIP_NORMAL) n = -n;
      pb = make_float4(point.x, point.y, point.z, bv.bias);
      nr = make_float4(n.x, n.y, n.z, bv.reach);
      rec = make_uint4(__float_as_uint(u), __float_as_uint(v), gid, i);
    }
    if (texels) texels[i] = rec;
  }
  // word j of the wave's 128 goes to lane j & 63 of store j >> 6: it is word j & 1 of the sample of lane j >> 1
  const size_t base = (size_t)(i - lane) * 2u;
#pragma unroll
  for (uint32_t h = 0; h < 2u; ++h) {
    const int src = (int)((lane >> 1) + 32u * h);
    const float4 a = make_float4(__shfl(pb.x, src), __shfl(pb.y, src), __shfl(pb.z, src), __shfl(pb.w, src));
    const float4 b = make_float4(__shfl(nr.x, src), __shfl(nr.y, src), __shfl(nr.z, src), __shfl(nr.w, src));
    const size_t j = base + 64u * h + lane;
    const bool odd = (lane & 1u) != 0u;  // (per component: a select between two float4 went through scratch)
    if (j < (size_t)count * 2u) samples[j] = make_float4(odd ? b.x : a.x, odd ? b.y : a.y, odd ? b.z : a.z, odd ? b.w : a.w);
  }
}

// RENDER_SPEC 4.12: the three kernels above with the corners of bake_tri_atlas, in the sample the flags of the owner's chart, and in the
// coverage a walk that bisects across long runs of triangles without pairs; nothing else differs.  They are kernels of their own and
// not a template flag over shared bodies: with the bodies shared, the compiler's report for the 4.11 kernels changed (k_bake_cover
// 38 -> 42 VGPRs), and those are to compile as they did.
__global__ void __launch_bounds__(256) k_bake_atlas_count(SceneView sv, BakeView bv, const BakeChartDev* __restrict__ charts,
                                                          unsigned long long* __restrict__ counts) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > bv.tri_count) return;
  unsigned long long c = 0ull;
  if (i < bv.tri_count) {
    const BakeBox bb = bake_box(bake_tri_atlas(sv, bv, charts, bv.first_tri + i), bv);
    c = (unsigned long long)bb.nbx * bb.nby;
  }
  counts[i] = c;
}

__global__ void __launch_bounds__(256) k_bake_atlas_cover(SceneView sv, BakeView bv, const BakeChartDev* __restrict__ charts,
                                                          const unsigned long long* __restrict__ off, uint32_t* __restrict__ owner) {
  const uint32_t lane = lane_id();
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, waves = (gridDim.x * blockDim.x) >> 6;
  const unsigned long long total = off[bv.tri_count];
  const unsigned long long run = (total + waves - 1ull) / waves;
  unsigned long long p = (unsigned long long)wave * run;
  const unsigned long long end = p + run < total ? p + run : total;
  if (p >= end) return;
  uint32_t lo = 0u, hi = bv.tri_count;  // off[lo] <= p < off[hi]
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (off[mid] <= p) lo = mid; else hi = mid;
  }
  uint32_t t = lo;
  unsigned long long t_begin = off[t], t_end = off[t + 1u];
  BakeTri tri = bake_tri_atlas(sv, bv, charts, bv.first_tri + t);
  BakeBox bb = bake_box(tri, bv);
  for (; p < end; ++p) {
    if (p >= t_end) {
      // (t < tri_count: p < total = off[tri_count]).  The span holds the triangles of uncharted instances, which have no pairs: a
      // wave that walked over 880 000 of them one dependent load at a time took 85 ms, so after a few steps it bisects
      uint32_t steps = 0u;
      do { ++t; t_begin = t_end; t_end = off[t + 1u]; } while (p >= t_end && ++steps < 8u);
      if (p >= t_end) {
        lo = t + 1u; hi = bv.tri_count;  // off[lo] <= p < off[hi]
        while (hi - lo > 1u) {
          const uint32_t mid = (lo + hi) >> 1;
          if (off[mid] <= p) lo = mid; else hi = mid;
        }
        t = lo; t_begin = off[t]; t_end = off[t + 1u];
      }
      tri = bake_tri_atlas(sv, bv, charts, bv.first_tri + t);
      bb = bake_box(tri, bv);
    }
    const uint32_t k = (uint32_t)(p - t_begin);
    const uint32_t row = k / bb.nbx, bx = bb.bx0 + (k - row * bb.nbx), by = bb.by0 + row;
    const uint32_t x = (bx << 3) + (lane & 7u), y = (by << 3) + (lane >> 3);
    if (x >= bv.width || y >= bv.height) continue;
    float w1, w2;
    if (bake_covers(tri, f2{(float)x + 0.5f, (float)y + 0.5f}, &w1, &w2)) atomicMin(owner + (((size_t)by * bv.blocks_x + bx) << 6) + lane, bv.first_tri + t);
  }
}

__global__ void __launch_bounds__(256) k_bake_atlas_sample(SceneView sv, BakeView bv, const BakeChartDev* __restrict__ charts,
                                                           const uint32_t* __restrict__ owner, float4* __restrict__ samples, uint4* __restrict__ texels) {
  const uint32_t count = bv.width * bv.height;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, lane = lane_id();
  float4 pb = make_float4(0.0f, 0.0f, 0.0f, 0.0f), nr = pb;  // the all-zero sample: invalid by RENDER_SPEC 4.10
  uint4 rec = make_uint4(0u, 0u, kAbsent, kAbsent);
  if (i < count) {
    const uint32_t y = i / bv.width, x = i - y * bv.width;
    const uint32_t gid = owner[bake_tiled(bv, x, y)];
    if (gid != kAbsent) {
      const BakeTri tri = bake_tri_atlas(sv, bv, charts, gid);
      float w1, w2;
      (void)bake_covers(tri, f2{(float)x + 0.5f, (float)y + 0.5f}, &w1, &w2);
      const float inv = 1.0f / tri.area;
      const float u = w1 * inv, v = w2 * inv;
      const float4* tp = reinterpret_cast<const float4*>(sv.tris_by_id + gid);
      const float4 t0 = tp[0], t1 = tp[1], t2 = tp[2];
      const f3 v0 = mk3(t0.x, t0.y, t0.z), e1 = mk3(t1.x, t1.y, t1.z), e2 = mk3(t2.x, t2.y, t2.z);
      const f3 point = madd3(e2, v, madd3(e1, u, v0));  // RENDER_SPEC 4.8's q
      f3 n;
      const uint32_t flags = charts[__float_as_uint(reinterpret_cast<const float4*>(sv.shade_tris + gid)[0].w)].flags;  // the chart's
      if (flags & HALA_BAKE_SHADING_NORMAL) {  // RENDER_SPEC 6 step 4, in the form of make_surface (shading.h)
        const float4* sp = reinterpret_cast<const float4*>(sv.shade_tris + gid);
        const float4 s0 = sp[0], s1 = sp[1], s2 = sp[2], s3 = sp[3];
        const float w0 = 1.0f - u - v;
        const f3 nl = madd3(mk3(s3.x, s3.y, s3.z), v, madd3(mk3(s2.x, s2.y, s2.z), u, mk3(s1.x, s1.y, s1.z) * w0));
        n = normalize3(transform_normal(sv.primitives[__float_as_uint(s0.w)].transform, nl));
      } else n = cross3(e1, e2);
      if (flags & HALA_BAKE_FLIP_NORMAL) n = -n;
      pb = make_float4(point.x, point.y, point.z, bv.bias);
      nr = make_float4(n.x, n.y, n.z, bv.reach);
      rec = make_uint4(__float_as_uint(u), __float_as_uint(v), gid, i);
    }
    if (texels) texels[i] = rec;
  }
  // word j of the wave's 128 goes to lane j & 63 of store j >> 6: it is word j & 1 of the sample of lane j >> 1
  const size_t base = (size_t)(i - lane) * 2u;
#pragma unroll
  for (uint32_t h = 0; h < 2u; ++h) {
    const int src = (int)((lane >> 1) + 32u * h);
    const float4 a = make_float4(__shfl(pb.x, src), __shfl(pb.y, src), __shfl(pb.z, src), __shfl(pb.w, src));
    const float4 b = make_float4(__shfl(nr.x, src), __shfl(nr.y, src), __shfl(nr.z, src), __shfl(nr.w, src));
    const size_t j = base + 64u * h + lane;
    const bool odd = (lane & 1u) != 0u;  // (per component: a select between two float4 went through scratch)
    if (j < (size_t)count * 2u) samples[j] = make_float4(odd ? b.x : a.x, odd ? b.y : a.y, odd ? b.z : a.z, odd ? b.w : a.w);
  }
}


// One wave per 8 x 8 block of the owner map: the block's 64 ownership bits (bit = (y & 7) * 8 + (x & 7)) as one word
__global__ void __launch_bounds__(256) k_bake_blocks(BakeView bv, const uint32_t* __restrict__ owner, unsigned long long* __restrict__ bits) {
  const uint32_t block = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (block >= bv.blocks_x * bv.blocks_y) return;  // (whole waves leave together)
  const unsigned long long owned = __ballot(owner[((size_t)block << 6) + lane_id()] != kAbsent);
  if (lane_id() == 0u) bits[block] = owned;
}

// The owned-texel list (RENDER_SPEC 4.12: what the listed occlusion pass of occlusion.hip traces).  k_bake_list_count: one lane per block,
// the popcount of its ownership word, and a 0 behind the last: the exclusive sum over blocks + 1 entries leaves the number of owned texels
// at [blocks], on the device.  k_bake_list: one wave per block, one texel per lane: an owned texel writes its row-major index at the
// block's offset + the owned texels of the block below its lane — block-major, deterministic, and a wave's 64 list entries are neighbours
// on the map; an ownerless texel of the map writes the invalid record, which no ray and no queue entry is spent on.
__global__ void __launch_bounds__(256) k_bake_list_count(BakeView bv, const unsigned long long* __restrict__ bits, uint32_t* __restrict__ counts) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, blocks = bv.blocks_x * bv.blocks_y;
  if (i > blocks) return;
  counts[i] = i < blocks ? (uint32_t)__popcll(bits[i]) : 0u;
}
__global__ void __launch_bounds__(256) k_bake_list(BakeView bv, const unsigned long long* __restrict__ bits, const uint32_t* __restrict__ off,
                                                   uint32_t* __restrict__ list, float4* __restrict__ out) {
  const uint32_t block = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = lane_id();
  if (block >= bv.blocks_x * bv.blocks_y) return;  // (whole waves leave together)
  const uint32_t by = block / bv.blocks_x, bx = block - by * bv.blocks_x;
  const uint32_t x = (bx << 3) + (lane & 7u), y = (by << 3) + (lane >> 3);
  if (x >= bv.width || y >= bv.height) return;  // (never owned: k_bake_cover leaves them out)
  const unsigned long long owned = bits[block];
  const uint32_t i = y * bv.width + x;
  if ((owned >> lane) & 1ull) list[off[block] + (uint32_t)__popcll(owned & ((1ull << lane) - 1ull))] = i;  // (< W * H: at most one entry per texel)
  else out[i] = make_float4(-1.0f, 0.0f, 0.0f, 0.0f);
}

// RENDER_SPEC 4.11, dilation: an ownerless texel looks at the owned texels within `margin` in x and in y and takes the record of the one
// with the least (squared distance, index), in integers.  Owned texels are read only and ownerless ones written only: in place.
// Most ownerless texels of a map with small charts have nothing in reach: the ownership words of the (at most 5 x 5) blocks the window
// touches, cut to the window, say so in 25 loads instead of the window's 1089 (measured, DESIGN.md 30: 12.0 -> 1.5 ms on a 4096 x 4096 map
// three quarters empty).  The others search
// rings of growing Chebyshev radius: a texel of ring r is at squared distance >= r^2, so the search ends once the best is below (r + 1)^2.
__global__ void __launch_bounds__(256) k_bake_dilate(BakeView bv, const uint32_t* __restrict__ owner, const unsigned long long* __restrict__ bits,
                                                     float4* __restrict__ out, uint4* __restrict__ texels) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= bv.width * bv.height) return;
  const int y = (int)(i / bv.width), x = (int)(i - (uint32_t)y * bv.width);
  if (owner[bake_tiled(bv, (uint32_t)x, (uint32_t)y)] != kAbsent) return;
  const int w = (int)bv.width, h = (int)bv.height, m = (int)bv.margin;
  {
    const int wx0 = max(x - m, 0), wx1 = min(x + m, w - 1), wy0 = max(y - m, 0), wy1 = min(y + m, h - 1);
    bool any = false;
    for (int by = wy0 >> 3; by <= wy1 >> 3; ++by) {
      const int r0 = max(wy0 - (by << 3), 0), r1 = min(wy1 - (by << 3), 7);  // the block's rows inside the window
      const unsigned long long rows = (r1 == 7 ? ~0ull : (1ull << ((r1 + 1) << 3)) - 1ull) & ~((1ull << (r0 << 3)) - 1ull);
      for (int bx = wx0 >> 3; bx <= wx1 >> 3; ++bx) {
        const int c0 = max(wx0 - (bx << 3), 0), c1 = min(wx1 - (bx << 3), 7);
        const unsigned long long cols = (unsigned long long)(((1u << (c1 + 1)) - 1u) & ~((1u << c0) - 1u)) * 0x0101010101010101ull;
        any = any || (bits[(size_t)by * bv.blocks_x + (size_t)bx] & rows & cols) != 0ull;
      }
    }
    if (!any) return;
  }
  uint32_t best_d = 0xffffffffu, best_i = kAbsent;
  const auto look = [&](int xx, int yy) {
    if (xx < 0 || yy < 0 || xx >= w || yy >= h) return;
    if (owner[bake_tiled(bv, (uint32_t)xx, (uint32_t)yy)] == kAbsent) return;
    const uint32_t d = (uint32_t)((xx - x) * (xx - x) + (yy - y) * (yy - y)), idx = (uint32_t)yy * bv.width + (uint32_t)xx;
    if (d < best_d || (d == best_d && idx < best_i)) { best_d = d; best_i = idx; }
  };
  for (int r = 1; r <= m; ++r) {
    if (best_d < (uint32_t)(r * r)) break;
    for (int k = -r; k <= r; ++k) { look(x + k, y - r); look(x + k, y + r); }
    for (int k = -r + 1; k < r; ++k) { look(x - r, y + k); look(x + r, y + k); }
  }
  if (best_i == kAbsent) return;
  out[i] = out[best_i];
  if (texels) texels[i].w = best_i;
}

// RENDER_SPEC 4.13, dilation: k_bake_dilate's rule and search on the 32-B records of a transfer bake (both halves of the chosen texel's
// record are copied).  A kernel of its own and not a template over the record: the 4.11 kernel is to compile as it did (the note above
// k_bake_atlas_count).
__global__ void __launch_bounds__(256) k_bake_dilate_transfer(BakeView bv, const uint32_t* __restrict__ owner, const unsigned long long* __restrict__ bits,
                                                              float4* __restrict__ out, uint4* __restrict__ texels) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= bv.width * bv.height) return;
  const int y = (int)(i / bv.width), x = (int)(i - (uint32_t)y * bv.width);
  if (owner[bake_tiled(bv, (uint32_t)x, (uint32_t)y)] != kAbsent) return;
  const int w = (int)bv.width, h = (int)bv.height, m = (int)bv.margin;
  {
    const int wx0 = max(x - m, 0), wx1 = min(x + m, w - 1), wy0 = max(y - m, 0), wy1 = min(y + m, h - 1);
    bool any = false;
    for (int by = wy0 >> 3; by <= wy1 >> 3; ++by) {
      const int r0 = max(wy0 - (by << 3), 0), r1 = min(wy1 - (by << 3), 7);  // the block's rows inside the window
      const unsigned long long rows = (r1 == 7 ? ~0ull : (1ull << ((r1 + 1) << 3)) - 1ull) & ~((1ull << (r0 << 3)) - 1ull);
      for (int bx = wx0 >> 3; bx <= wx1 >> 3; ++bx) {
        const int c0 = max(wx0 - (bx << 3), 0), c1 = min(wx1 - (bx << 3), 7);
        const unsigned long long cols = (unsigned long long)(((1u << (c1 + 1)) - 1u) & ~((1u << c0) - 1u)) * 0x0101010101010101ull;
        any = any || (bits[(size_t)by * bv.blocks_x + (size_t)bx] & rows & cols) != 0ull;
      }
    }
    if (!any) return;
  }
  uint32_t best_d = 0xffffffffu, best_i = kAbsent;
  const auto look = [&](int xx, int yy) {
    if (xx < 0 || yy < 0 || xx >= w || yy >= h) return;
    if (owner[bake_tiled(bv, (uint32_t)xx, (uint32_t)yy)] == kAbsent) return;
    const uint32_t d = (uint32_t)((xx - x) * (xx - x) + (yy - y) * (yy - y)), idx = (uint32_t)yy * bv.width + (uint32_t)xx;
    if (d < best_d || (d == best_d && idx < best_i)) { best_d = d; best_i = idx; }
  };
  for (int r = 1; r <= m; ++r) {
    if (best_d < (uint32_t)(r * r)) break;
    for (int k = -r; k <= r; ++k) { look(x + k, y - r); look(x + k, y + r); }
    for (int k = -r + 1; k < r; ++k) { look(x - r, y + k); look(x + r, y + k); }
  }
  if (best_i == kAbsent) return;
  const float4 a = out[(size_t)best_i * 2u], b = out[(size_t)best_i * 2u + 1u];
  out[(size_t)i * 2u] = a; out[(size_t)i * 2u + 1u] = b;
  if (texels) texels[i].w = best_i;
}

static BakeView bake_grid(BakeView bv) {
  bv.blocks_x = (bv.width + 7u) >> 3; bv.blocks_y = (bv.height + 7u) >> 3;
  return bv;
}
size_t bake_owner_words(const BakeView& bv) { return (size_t)((bv.width + 7u) >> 3) * ((bv.height + 7u) >> 3) * 64u; }
size_t bake_scan_bytes(uint32_t tri_count) {
  size_t bytes = 0;
  (void)rocprim::exclusive_scan(nullptr, bytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, 0ull, (size_t)tri_count + 1u,
                                rocprim::plus<unsigned long long>(), 0);
  return bytes;
}
size_t bake_list_scan_bytes(size_t blocks) {
  size_t bytes = 0;
  (void)rocprim::exclusive_scan(nullptr, bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, blocks + 1u, rocprim::plus<uint32_t>(), 0);
  return bytes;
}
// charts null: RENDER_SPEC 4.11, the instance of the view; else 4.12
static hipError_t bake_samples(const SceneView& sv, uint32_t cu_count, const BakeView& view, const BakeScratch& sc, const BakeChartDev* charts,
                               hala_occlusion_sample* samples, hala_bake_texel* texels, hipStream_t s) {
  const BakeView bv = bake_grid(view);
  const uint32_t count = bv.width * bv.height;
  hipError_t e = hipMemsetAsync(sc.owner, 0xff, bake_owner_words(bv) * 4u, s);
  if (e != hipSuccess) return e;
  if (bv.tri_count) {
    if (charts) hipLaunchKernelGGL(k_bake_atlas_count, dim3(blocks_for(bv.tri_count + 1u, 256)), dim3(256), 0, s, sv, bv, charts, sc.counts);
    else hipLaunchKernelGGL(k_bake_count, dim3(blocks_for(bv.tri_count + 1u, 256)), dim3(256), 0, s, sv, bv, sc.counts);
    size_t bytes = sc.scan_bytes;
    e = rocprim::exclusive_scan(sc.scan_tmp, bytes, sc.counts, sc.offsets, 0ull, (size_t)bv.tri_count + 1u, rocprim::plus<unsigned long long>(), s);
    if (e != hipSuccess) return e;
    // enough waves to fill the chip several times over, and no more than there can be pairs
    const unsigned long long most = (unsigned long long)bv.blocks_x * bv.blocks_y * bv.tri_count;
    const uint32_t blocks = (uint32_t)std::min<unsigned long long>((unsigned long long)cu_count * 16ull, (most + 3ull) / 4ull);
    if (charts) hipLaunchKernelGGL(k_bake_atlas_cover, dim3(std::max(blocks, 1u)), dim3(256), 0, s, sv, bv, charts, sc.offsets, sc.owner);
    else hipLaunchKernelGGL(k_bake_cover, dim3(std::max(blocks, 1u)), dim3(256), 0, s, sv, bv, sc.offsets, sc.owner);
  }
  if (charts)
    hipLaunchKernelGGL(k_bake_atlas_sample, dim3(blocks_for(count, 256)), dim3(256), 0, s, sv, bv, charts, sc.owner, reinterpret_cast<float4*>(samples),
                       reinterpret_cast<uint4*>(texels));
  else
    hipLaunchKernelGGL(k_bake_sample, dim3(blocks_for(count, 256)), dim3(256), 0, s, sv, bv, sc.owner, reinterpret_cast<float4*>(samples),
                       reinterpret_cast<uint4*>(texels));
  return hipGetLastError();
}
hipError_t launch_bake_samples(const SceneView& sv, uint32_t cu_count, const BakeView& view, const BakeScratch& sc, hala_occlusion_sample* samples,
                               hala_bake_texel* texels, hipStream_t s) {
  return bake_samples(sv, cu_count, view, sc, nullptr, samples, texels, s);
}
hipError_t launch_bake_samples_atlas(const SceneView& sv, uint32_t cu_count, const BakeView& view, const BakeScratch& sc, const BakeChartDev* charts,
                                     hala_occlusion_sample* samples, hala_bake_texel* texels, hipStream_t s) {
  return bake_samples(sv, cu_count, view, sc, charts, samples, texels, s);
}
hipError_t launch_bake_list(const BakeView& view, const BakeScratch& sc, const BakeListScratch& ls, hala_occlusion* out, hipStream_t s) {
  const BakeView bv = bake_grid(view);
  const uint32_t blocks = bv.blocks_x * bv.blocks_y;
  hipLaunchKernelGGL(k_bake_blocks, dim3(blocks_for(blocks, 4)), dim3(256), 0, s, bv, sc.owner, sc.block_bits);
  hipLaunchKernelGGL(k_bake_list_count, dim3(blocks_for(blocks + 1u, 256)), dim3(256), 0, s, bv, sc.block_bits, ls.list_counts);
  size_t bytes = sc.scan_bytes;
  const hipError_t e = rocprim::exclusive_scan(sc.scan_tmp, bytes, ls.list_counts, ls.list_offsets, 0u, (size_t)blocks + 1u, rocprim::plus<uint32_t>(), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_bake_list, dim3(blocks_for(blocks, 4)), dim3(256), 0, s, bv, sc.block_bits, ls.list_offsets, ls.list, reinterpret_cast<float4*>(out));
  return hipGetLastError();
}
void launch_bake_dilate(const BakeView& view, const BakeScratch& sc, hala_occlusion* out, hala_bake_texel* texels, hipStream_t s, bool bits_ready) {
  const BakeView bv = bake_grid(view);
  if (bv.margin == 0u) return;
  if (!bits_ready)
    hipLaunchKernelGGL(k_bake_blocks, dim3(blocks_for(bv.blocks_x * bv.blocks_y, 4)), dim3(256), 0, s, bv, sc.owner, sc.block_bits);
  hipLaunchKernelGGL(k_bake_dilate, dim3(blocks_for(bv.width * bv.height, 256)), dim3(256), 0, s, bv, sc.owner, sc.block_bits,
                     reinterpret_cast<float4*>(out), reinterpret_cast<uint4*>(texels));
}
void launch_bake_dilate_transfer(const BakeView& view, const BakeScratch& sc, hala_bake_transfer_hit* out, hala_bake_texel* texels, hipStream_t s) {
  const BakeView bv = bake_grid(view);
  if (bv.margin == 0u) return;
  hipLaunchKernelGGL(k_bake_blocks, dim3(blocks_for(bv.blocks_x * bv.blocks_y, 4)), dim3(256), 0, s, bv, sc.owner, sc.block_bits);
  hipLaunchKernelGGL(k_bake_dilate_transfer, dim3(blocks_for(bv.width * bv.height, 256)), dim3(256), 0, s, bv, sc.owner, sc.block_bits,
                     reinterpret_cast<float4*>(out), reinterpret_cast<uint4*>(texels));
}

}  // namespace rt
