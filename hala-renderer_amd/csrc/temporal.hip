// temporal.hip — docs/RENDER_SPEC.md 16: temporal reprojection of the accumulated frame across scene edits.  One frame-space kernel
// beside the integrator: k_temporal_resolve carries each pixel's mean first hit (image 4) back through the motion of its instance and the
// captured camera, gathers the four bilinear taps of the history around that point, keeps the taps whose ids and position agree, and
// blends them with the current accumulation by sample count.  Every operation is the one the spec writes, in its order
// (-ffp-contract=off: an fma only where the spec says madd / dot), so that tests/temporal_ref.py reproduces both outputs bit for bit.
//
// Memory: per pixel three 16-B loads of the current frame, the 64-B motion record of its instance, three 16-B loads per tap and two 16-B
// stores: 240 B requested and 32 B written when all four taps are in the frame.  Neighbouring pixels share their taps, so the unique traffic
// is the six images read once (96 B per pixel) plus the two written; 16 x 16 workgroups keep the taps of a wave in a few lines.  The
// cameras are wave-uniform and come in by scalar loads.  No LDS, no atomics (DESIGN.md "Temporal reprojection" has the measured time).
//
// "Vertex motion" of the same section is the kernel's second instantiation: a pixel of a deformed primitive is carried by its triangle's
// two records, now and as captured, instead of its instance's motion (tests/temporal_vertex_ref.py is its twin).
//
// "History clamp" of the same section is two more instantiations: the workgroup stages the rgb of its 16 x 16 pixels of the current
// accumulation and a halo of `radius` pixels in LDS (three planes, no new unique traffic: the kernel reads that image anyway), and a pixel
// that found its history clamps it to mean +- gamma standard errors of its (2 radius + 1)^2 neighbourhood before the blend
// (tests/temporal_clamp_ref.py is the twin of all four instantiations).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "rt_math.h"
#include "temporal.h"

namespace rt {

namespace {

constexpr uint32_t kTile = 16;  // 16 x 16 pixels per workgroup
constexpr uint32_t kAbsentId = 0xFFFFFFFFu;

// RENDER_SPEC 16 "History clamp": the staged tile is (16 + 2 radius)^2 <= 22 x 22 floats per plane.  Rows are kClampPitch = 48 floats apart:
// a ds_read_b32 is served in two halves of 32 lanes, a half is two tile rows of 16 pixels, and the banks are (address / 4) mod 32, so the
// two rows of a half must lie 16 mod 32 banks apart (22 <= pitch: 48) to cover the 32 banks once for whatever tap offset (DESIGN.md 15
// "History clamp").  3 planes x 22 rows x 48 floats = 12672 B per workgroup, which is above no occupancy limit of the kernel.
constexpr uint32_t kClampMaxRadius = 3, kClampSide = kTile + 2 * kClampMaxRadius, kClampPitch = 48, kClampPlane = kClampSide * kClampPitch;
typedef __attribute__((address_space(3))) float lds_float;  // (generic pointers to LDS compile to flat loads)

struct Projected {
  float u, v, z;  // continuous pixel coordinates (pixel centres are integers), view depth
  bool ok;
};

// RENDER_SPEC 16 "Projection": the inverse of RENDER_SPEC 5 for an unjittered sample through the lens centre
RT_DI Projected project(const TemporalCamera& cam, float width, float height, float aspect, f3 p) {
  const f3 right = ld3(cam.right), up = ld3(cam.up), fwd = ld3(cam.forward);
  const f3 v = p - ld3(cam.position);
  const float ff = dot3(fwd, fwd);
  const float vf = dot3(v, fwd);
  const float a = dot3(v, right) / dot3(right, right);
  const float b = dot3(v, up) / dot3(up, up);
  Projected o;
  o.z = vf * (1.0f / sqrtf(ff));
  float ndc_x, ndc_y;
  if (cam.type == 0u) {
    const float c = vf / ff;
    ndc_x = (a / c) / (aspect * cam.tan_half);
    ndc_y = (b / c) / cam.tan_half;
    o.ok = o.z > 0.0f;
  } else {
    ndc_x = a / cam.xmag;
    ndc_y = b / cam.ymag;
    o.ok = true;
  }
  o.u = ((ndc_x + 1.0f) * 0.5f) * width - 0.5f;
  o.v = ((1.0f - ndc_y) * 0.5f) * height - 0.5f;
  return o;
}

// RENDER_SPEC 16 "Vertex motion" steps 1-4: the barycentrics of the foot of pw on triangle g as it is now, placed on that triangle now
// (pc, the point cam_cur projects) and as captured (pp).  false: no history.
RT_DI bool vertex_points(const float4* __restrict__ tris, const float4* __restrict__ snap, uint32_t tri_count, uint32_t g, f3 pw, f3* pp, f3* pc) {
  if (g >= tri_count) return false;
  const float4 t0 = tris[3u * (size_t)g], t1 = tris[3u * (size_t)g + 1u], t2 = tris[3u * (size_t)g + 2u];
  const f3 v0 = f3{t0.x, t0.y, t0.z}, e1 = f3{t1.x, t1.y, t1.z}, e2 = f3{t2.x, t2.y, t2.z};
  const f3 q = pw - v0;
  const float d11 = dot3(e1, e1), d12 = dot3(e1, e2), d22 = dot3(e2, e2);
  const float q1 = dot3(q, e1), q2 = dot3(q, e2);
  const float det = d11 * d22 - d12 * d12;
  if (!(det > 0.0f)) return false;  // a degenerate triangle (NaN fails)
  const float u = (d22 * q1 - d12 * q2) / det, v = (d11 * q2 - d12 * q1) / det;
  const float w0 = (1.0f - u) - v;
  if (!(u >= -1.0f && v >= -1.0f && w0 >= -1.0f)) return false;  // beyond the triangle and its mirror images across its edges (NaN fails)
  const float4 s0 = snap[3u * (size_t)g], s1 = snap[3u * (size_t)g + 1u], s2 = snap[3u * (size_t)g + 2u];
  *pc = f3{__fmaf_rn(v, e2.x, __fmaf_rn(u, e1.x, v0.x)), __fmaf_rn(v, e2.y, __fmaf_rn(u, e1.y, v0.y)), __fmaf_rn(v, e2.z, __fmaf_rn(u, e1.z, v0.z))};
  *pp = f3{__fmaf_rn(v, s2.x, __fmaf_rn(u, s1.x, s0.x)), __fmaf_rn(v, s2.y, __fmaf_rn(u, s1.y, s0.y)), __fmaf_rn(v, s2.z, __fmaf_rn(u, s1.z, s0.z))};
  return isfinite(pp->x) && isfinite(pp->y) && isfinite(pp->z);
}

// VERTEX: some instance of the table carries mark 2 (RENDER_SPEC 16 "Vertex motion").  A pixel of such an instance takes the barycentrics
// of its mean hit point on triangle I.w as it is now (tris) and places them on the same triangle of the capture (snap): six more 16-B
// loads, two 48-B records that neighbouring pixels share or find next to theirs.  The false instantiation is the kernel as it was before
// vertex motion existed and is the one launched whenever no instance carries mark 2; it never reads tris, snap or tri_count.
//
// CLAMP: RENDER_SPEC 16 "History clamp" is on and a history exists.  All 256 threads of the workgroup, those outside the frame included,
// stage the tile and meet at one barrier before any of them returns; a tap is valid by its coordinates, so the entries of the tile that
// lie outside the frame are neither written nor read.  The statistics are computed by the lanes that reach the blend, from LDS, two passes
// over the taps in the order the spec writes.  The two CLAMP = false instantiations are the kernels as they were before the clamp existed.
template <bool VERTEX, bool CLAMP>
__global__ void __launch_bounds__(256) k_temporal_resolve(const float4* __restrict__ accum, const float4* __restrict__ pos, const uint4* __restrict__ ids,
                                                          const float4* __restrict__ hc, const float4* __restrict__ hp, const uint4* __restrict__ hi,
                                                          const uint32_t* __restrict__ table, uint32_t width, uint32_t height, float n,
                                                          uint32_t has_history, float4* __restrict__ temporal, float4* __restrict__ motion,
                                                          const float4* __restrict__ tris, const float4* __restrict__ snap, uint32_t tri_count,
                                                          uint32_t radius, float gamma) {
  const uint32_t x = blockIdx.x * kTile + threadIdx.x, y = blockIdx.y * kTile + threadIdx.y;
  [[maybe_unused]] lds_float* tile = nullptr;
  if constexpr (CLAMP) {
    __shared__ float staged[3 * kClampPlane];
    tile = (lds_float*)staged;
    const uint32_t side = kTile + 2u * radius;  // radius <= kClampMaxRadius (the launcher)
    const int bx = (int)(blockIdx.x * kTile) - (int)radius, by = (int)(blockIdx.y * kTile) - (int)radius;
    for (uint32_t e = threadIdx.y * kTile + threadIdx.x; e < side * side; e += kTile * kTile) {
      const uint32_t ey = e / side, ex = e - ey * side;
      const int qx = bx + (int)ex, qy = by + (int)ey;
      if (qx < 0 || qx >= (int)width || qy < 0 || qy >= (int)height) continue;
      const float4 v = accum[(uint32_t)qy * width + (uint32_t)qx];
      lds_float* at = tile + ey * kClampPitch + ex;
      at[0] = v.x; at[kClampPlane] = v.y; at[2u * kClampPlane] = v.z;
    }
    __syncthreads();
  }
  if (x >= width || y >= height) return;
  const uint32_t p = y * width + x;
  const float4 c = accum[p];
  float4 t_out = make_float4(c.x, c.y, c.z, n), m_out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const TemporalHead& hd = *reinterpret_cast<const TemporalHead*>(table);
  const TemporalInst* insts = reinterpret_cast<const TemporalInst*>(table + sizeof(TemporalHead) / 4);
  const uint32_t* mat_mark = table + sizeof(TemporalHead) / 4 + (size_t)hd.inst_count * (sizeof(TemporalInst) / 4);
  const float4 pm = pos[p];
  const uint4 id = ids[p];
  bool history = has_history != 0u && id.y != kAbsentId && pm.w > 0.0f && id.y < hd.inst_count && id.z < hd.mat_count;
  if (history) {
    const float4* rec = reinterpret_cast<const float4*>(insts + id.y);
    const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
    const uint32_t inst_mark = __float_as_uint(rec[3].x);
    const bool by_vertex = VERTEX && inst_mark == 2u;
    const uint32_t marked = (by_vertex ? 0u : inst_mark) | mat_mark[id.z];  // a material mark wins over vertex motion
    history = marked == 0u;
    if (history) {
      const f3 pw = f3{pm.x / pm.w, pm.y / pm.w, pm.z / pm.w};
      f3 pp = pw, pc = pw;  // the point under the capture, and the point cam_cur projects
      if (by_vertex) {
        history = vertex_points(tris, snap, tri_count, id.w, pw, &pp, &pc);
      } else {
        pp = f3{__fmaf_rn(r0.z, pw.z, __fmaf_rn(r0.y, pw.y, __fmaf_rn(r0.x, pw.x, r0.w))),
                __fmaf_rn(r1.z, pw.z, __fmaf_rn(r1.y, pw.y, __fmaf_rn(r1.x, pw.x, r1.w))),
                __fmaf_rn(r2.z, pw.z, __fmaf_rn(r2.y, pw.y, __fmaf_rn(r2.x, pw.x, r2.w)))};
      }
      const Projected a = project(hd.prev, hd.width, hd.height, hd.aspect, pp);
      const Projected b = project(hd.cur, hd.width, hd.height, hd.aspect, pc);
      bool carry = history && a.ok && b.ok;
      if (by_vertex && carry) {  // step 6: a mean hit point off the plane of its triangle averages several surfaces
        const f3 r = pw - pc;
        const float zc = hd.cur.type == 0u ? b.z : (2.0f * hd.cur.ymag) * sqrtf(dot3(ld3(hd.cur.up), ld3(hd.cur.up)));
        const float rl = hd.tol * zc;
        carry = (r.x * r.x + r.y * r.y) + r.z * r.z <= rl * rl;
      }
      if (carry) {
        const float mx = a.u - b.u, my = a.v - b.v;
        const float fx = (float)x + mx, fy = (float)y + my;
        m_out = make_float4(mx, my, a.z, 1.0f);
        if (fx > -1.0f && fx < hd.width && fy > -1.0f && fy < hd.height) {  // else all four taps are outside the frame (NaN fails)
          const float x0f = floorf(fx), y0f = floorf(fy);
          const float tx = fx - x0f, ty = fy - y0f;
          const int x0 = (int)x0f, y0 = (int)y0f;
          const float zt = hd.prev.type == 0u ? a.z : (2.0f * hd.prev.ymag) * sqrtf(dot3(ld3(hd.prev.up), ld3(hd.prev.up)));
          const float lim = hd.tol * zt;
          const float lim2 = lim * lim;
          float sr = 0.0f, sg = 0.0f, sb = 0.0f, sh = 0.0f, sw = 0.0f;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
            const float wx = (k & 1) ? tx : 1.0f - tx, wy = (k >> 1) ? ty : 1.0f - ty;
            const float w = wx * wy;
            if (qx < 0 || qx >= (int)width || qy < 0 || qy >= (int)height || !(w > 0.0f)) continue;
            const uint32_t q = (uint32_t)qy * width + (uint32_t)qx;
            const float4 qc = hc[q], qp = hp[q];
            const uint4 qi = hi[q];
            if (!(qc.w > 0.0f) || !(qp.w > 0.0f) || qi.y != id.y || qi.z != id.z) continue;
            const float dx = qp.x / qp.w - pp.x, dy = qp.y / qp.w - pp.y, dz = qp.z / qp.w - pp.z;
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            if (!(d2 <= lim2)) continue;
            sr = sr + qc.x * w; sg = sg + qc.y * w; sb = sb + qc.z * w; sh = sh + qc.w * w;
            sw = sw + w;
          }
          if (sw >= hd.min_weight) {  // min_weight > 0: at least one tap
            float hr = sr / sw, hg = sg / sw, hb = sb / sw;
            const float hl = sh / sw;
            if constexpr (CLAMP) {
              const int rad = (int)radius;
              const lds_float* centre = tile + (threadIdx.y + radius) * kClampPitch + (threadIdx.x + radius);
              float cnt = 0.0f, ar = 0.0f, ag = 0.0f, ab = 0.0f;
              for (int dy = -rad; dy <= rad; ++dy) {
                if ((int)y + dy < 0 || (int)y + dy >= (int)height) continue;
                for (int dx = -rad; dx <= rad; ++dx) {
                  if ((int)x + dx < 0 || (int)x + dx >= (int)width) continue;
                  const lds_float* q = centre + dy * (int)kClampPitch + dx;
                  cnt = cnt + 1.0f;
                  ar = ar + q[0]; ag = ag + q[kClampPlane]; ab = ab + q[2u * kClampPlane];
                }
              }
              const float mr = ar / cnt, mg = ag / cnt, mb = ab / cnt;
              float vr = 0.0f, vg = 0.0f, vb = 0.0f;
              for (int dy = -rad; dy <= rad; ++dy) {
                if ((int)y + dy < 0 || (int)y + dy >= (int)height) continue;
                for (int dx = -rad; dx <= rad; ++dx) {
                  if ((int)x + dx < 0 || (int)x + dx >= (int)width) continue;
                  const lds_float* q = centre + dy * (int)kClampPitch + dx;
                  const float er = q[0] - mr, eg = q[kClampPlane] - mg, eb = q[2u * kClampPlane] - mb;
                  vr = vr + er * er; vg = vg + eg * eg; vb = vb + eb * eb;
                }
              }
              const float wr = gamma * sqrtf((vr / cnt) / cnt), wg = gamma * sqrtf((vg / cnt) / cnt), wb = gamma * sqrtf((vb / cnt) / cnt);
              const float lr = mr - wr, ur = mr + wr, lg = mg - wg, ug = mg + wg, lb = mb - wb, ub = mb + wb;
              hr = hr < lr ? lr : (hr > ur ? ur : hr);  // a NaN history stays NaN; NaN bounds leave it as it is
              hg = hg < lg ? lg : (hg > ug ? ug : hg);
              hb = hb < lb ? lb : (hb > ub ? ub : hb);
            }
            const float h = hl > hd.max_history ? hd.max_history : hl;
            const float tw = h + n;
            t_out = make_float4((hr * h + c.x * n) / tw, (hg * h + c.y * n) / tw, (hb * h + c.z * n) / tw, tw);
          }
        }
      }
    }
  }
  temporal[p] = t_out;
  motion[p] = m_out;
}

}  // namespace

std::string temporal_check_params(const hala_temporal_params* p) {
  if (!p) return "The temporal parameters are null.";
  if (!(p->max_history >= 1.0f && p->max_history <= 1048576.0f)) return "Invalid temporal max_history: expected a finite value in [1, 2^20].";  // NaN fails
  if (!(p->tol >= 1e-6f && p->tol <= 1.0f)) return "Invalid temporal tol: expected a finite value in [1e-6, 1].";
  if (!(p->min_weight > 0.0f && p->min_weight <= 1.0f)) return "Invalid temporal min_weight: expected a finite value in (0, 1].";
  for (uint32_t v : p->reserved) if (v) return "The reserved words of the temporal parameters must be zero.";
  return "";
}

std::string temporal_check_clamp_params(const hala_temporal_clamp_params* p) {
  if (!p) return "The temporal clamp parameters are null.";
  if (!(p->radius >= 1u && p->radius <= kClampMaxRadius)) return "Invalid temporal clamp radius: expected 1, 2 or 3.";
  if (!(p->gamma > 0.0f && p->gamma <= 1000.0f)) return "Invalid temporal clamp gamma: expected a finite value in (0, 1000].";  // NaN fails
  for (uint32_t v : p->reserved) if (v) return "The reserved words of the temporal clamp parameters must be zero.";
  return "";
}

bool temporal_motion(const float* w_prev, const float* w_cur, float d[12]) {
  static const float kIdentity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  memcpy(d, kIdentity, sizeof(kIdentity));
  if (memcmp(w_prev, w_cur, 64) == 0) return true;  // bit-equal transforms: exactly the identity
  // a[r][c]: column-major 4 x 4, the affine part
  const auto A = [w_cur](int r, int c) { return (double)w_cur[4 * c + r]; };
  const auto P = [w_prev](int r, int c) { return (double)w_prev[4 * c + r]; };
  double inv[3][3];
  inv[0][0] = A(1, 1) * A(2, 2) - A(1, 2) * A(2, 1); inv[0][1] = A(0, 2) * A(2, 1) - A(0, 1) * A(2, 2); inv[0][2] = A(0, 1) * A(1, 2) - A(0, 2) * A(1, 1);
  inv[1][0] = A(1, 2) * A(2, 0) - A(1, 0) * A(2, 2); inv[1][1] = A(0, 0) * A(2, 2) - A(0, 2) * A(2, 0); inv[1][2] = A(0, 2) * A(1, 0) - A(0, 0) * A(1, 2);
  inv[2][0] = A(1, 0) * A(2, 1) - A(1, 1) * A(2, 0); inv[2][1] = A(0, 1) * A(2, 0) - A(0, 0) * A(2, 1); inv[2][2] = A(0, 0) * A(1, 1) - A(0, 1) * A(1, 0);
  const double det = (A(0, 0) * inv[0][0] + A(0, 1) * inv[1][0]) + A(0, 2) * inv[2][0];
  double scale = 1.0;
  for (int c = 0; c < 3; ++c) scale = scale * std::sqrt((A(0, c) * A(0, c) + A(1, c) * A(1, c)) + A(2, c) * A(2, c));
  if (!(std::fabs(det) > 1e-12 * scale)) return false;  // singular (NaN fails too)
  for (auto& row : inv) for (double& v : row) v = v / det;
  float out[12];
  for (int r = 0; r < 3; ++r) {
    double l[3];
    for (int c = 0; c < 3; ++c) l[c] = (P(r, 0) * inv[0][c] + P(r, 1) * inv[1][c]) + P(r, 2) * inv[2][c];
    const double t = P(r, 3) - ((l[0] * A(0, 3) + l[1] * A(1, 3)) + l[2] * A(2, 3));
    out[4 * r + 0] = (float)l[0]; out[4 * r + 1] = (float)l[1]; out[4 * r + 2] = (float)l[2]; out[4 * r + 3] = (float)t;
  }
  for (float v : out) if (!std::isfinite(v)) return false;
  memcpy(d, out, sizeof(out));
  return true;
}

TemporalCamera temporal_camera(const hala_gpu_camera& c, float tan_half) {
  TemporalCamera t{};
  memcpy(t.position, c.position, 12); memcpy(t.right, c.right, 12); memcpy(t.up, c.up, 12); memcpy(t.forward, c.forward, 12);
  t.tan_half = tan_half; t.xmag = c.focal_distance_or_xmag; t.ymag = c.aperture_or_ymag; t.type = c.type;
  return t;
}

void launch_temporal_resolve(const float4* accum, const float4* pos, const uint4* ids, const float4* hc, const float4* hp, const uint4* hi,
                             const uint32_t* table, uint32_t w, uint32_t h, uint32_t n, bool has_history, float4* temporal, float4* motion,
                             const Tri* tris, const Tri* snap, uint32_t tri_count, const hala_temporal_clamp_params* clamp, hipStream_t s) {
  const dim3 grid((w + kTile - 1) / kTile, (h + kTile - 1) / kTile), block(kTile, kTile);
  const bool vertex = has_history && tris && snap && tri_count;
  // without a history no pixel reaches the blend: the plain kernels, which stage nothing
  const bool clamped = has_history && clamp && clamp->radius >= 1u && clamp->radius <= kClampMaxRadius;
  const auto kernel = clamped ? (vertex ? k_temporal_resolve<true, true> : k_temporal_resolve<false, true>)
                              : (vertex ? k_temporal_resolve<true, false> : k_temporal_resolve<false, false>);
  hipLaunchKernelGGL(kernel, grid, block, 0, s, accum, pos, ids, hc, hp, hi, table, w, h, (float)n, has_history ? 1u : 0u, temporal, motion,
                     reinterpret_cast<const float4*>(tris), reinterpret_cast<const float4*>(snap), vertex ? tri_count : 0u,
                     clamped ? clamp->radius : 0u, clamped ? clamp->gamma : 0.0f);
}

}  // namespace rt

using namespace rt;

static_assert(sizeof(hala_temporal_params) == 32, "hala_temporal_params is 32 B");
static_assert(sizeof(hala_temporal_clamp_params) == 16, "hala_temporal_clamp_params is 16 B");

void hala_temporal_default_params(hala_temporal_params* out) {
  if (!out) return;
  memset(out, 0, sizeof(*out));
  out->max_history = 32.0f;  // DESIGN.md "Temporal reprojection" has the sweep behind the two
  out->tol = 0.05f;
  out->min_weight = 0.25f;
}

void hala_temporal_clamp_default_params(hala_temporal_clamp_params* out) {
  if (!out) return;
  memset(out, 0, sizeof(*out));
  out->radius = 1u;  // DESIGN.md "History clamp" has the sweep behind the two
  out->gamma = 2.0f;
}
