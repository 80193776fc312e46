// resolve.hip — the frame-space kernels behind the wavefront path tracer (trace_closest.hip has the frame's kernel sequence): resolve,
// relight, the tile scatter of sharded frames and the stand-alone texture fetch.
#include "shading.h"
#include "variants.h"

namespace rt {
// ---------------------------------------------------------------------------------------------------------
// resolve: fold this sample into the running means and write the tonemapped final image (RENDER_SPEC §8)
// ---------------------------------------------------------------------------------------------------------
// Several views (RENDER_SPEC §12): thread t of views x pixel_slots resolves pixel slot t % pixel_slots of view t / pixel_slots into that
// view's images (view_pixels float4s apart; view 0's are the renderer's usual images).
// AOV (RENDER_SPEC §13): `pos` (may be null) folds (P, hit) like the other means; `ids` (may be null) takes the ids of the sample of frame 0
// of the accumulation and keeps them after that.  The variant without the flag never looks at the two images.
// GROUPS (RENDER_SPEC §14): image g of the light groups (at gimg + g * gimg_stride, laid out like accum) folds S_g = L_g (+ Le for the
// environment's group when env_type is MAP) in frame order, a non-finite S_g replaced by 0 on its own.
template <bool AOV, bool GROUPS>
__global__ void __launch_bounds__(256) k_resolve(FrameConst fc, PathState ps, float4* __restrict__ accum, float4* __restrict__ albedo,
                                                  float4* __restrict__ normal, float4* __restrict__ final_img, float4* __restrict__ pos,
                                                  uint4* __restrict__ ids, float4* __restrict__ gimg, size_t gimg_stride) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t view = t / fc.pixel_slots, pslot = t - view * fc.pixel_slots;
  if (view >= fc.views) return;
  // padding slots (of a border block, of a padding tile, or outside the frame in a border tile) are never written: they keep the zeros
  // the images were allocated with (RENDER_SPEC §9)
  uint32_t px, py;
  if (!slot_to_pixel(fc, pslot, &px, &py)) return;
  // where the pixel of this slot lives in the images: sharded ranks keep their tile buffers in slot order (RENDER_SPEC §9), an unsharded
  // frame is row-major whatever the slot order
  const size_t at = (fc.world <= 1u ? py * fc.width + px : pslot) + (size_t)view * fc.view_pixels;
  // the running means; a batch that starts an accumulation (frame_index 0) never looks at them (fold_mean)
  float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a, n = a;
  if (fc.u.frame_index != 0u) { a = accum[at]; b = albedo[at]; n = normal[at]; }
  float4 p = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  uint4 id = make_uint4(kAbsent, kAbsent, kAbsent, kAbsent);
  if (AOV && pos && fc.u.frame_index != 0u) p = pos[at];
  for (uint32_t k = 0; k < fc.samples; ++k) {  // the batch's samples, folded in frame order
    const uint32_t slot = (k * fc.views + view) * fc.pixel_slots + pslot;
    const P3 lr = ps.radiance[slot];
    f3 L = mk3(lr.x, lr.y, lr.z);
    if (fc.u.env_type == 1u) { const P3 le = ps.radiance_env[slot]; L = L + mk3(le.x, le.y, le.z); }  // RENDER_SPEC §6: L + Le
    if (!(isfinite(L.x) && isfinite(L.y) && isfinite(L.z))) L = splat3(0.0f);
    const uint32_t fi = fc.u.frame_index + k;
    const P3 sa = ps.albedo[slot], sn = ps.normal[slot];
    a = make_float4(fold_mean(a.x, L.x, fi), fold_mean(a.y, L.y, fi), fold_mean(a.z, L.z, fi), 1.0f);
    b = make_float4(fold_mean(b.x, sa.x, fi), fold_mean(b.y, sa.y, fi), fold_mean(b.z, sa.z, fi), 1.0f);
    n = make_float4(fold_mean(n.x, sn.x, fi), fold_mean(n.y, sn.y, fi), fold_mean(n.z, sn.z, fi), 1.0f);
    if (AOV && pos) {
      const float4 sp = ps.aov_pos[slot];
      p = make_float4(fold_mean(p.x, sp.x, fi), fold_mean(p.y, sp.y, fi), fold_mean(p.z, sp.z, fi), fold_mean(p.w, sp.w, fi));
    }
    if (AOV && ids && fi == 0u) id = ps.aov_ids[slot];
  }
  accum[at] = a; albedo[at] = b; normal[at] = n;
  if (AOV && pos) pos[at] = p;
  if (GROUPS)
    for (uint32_t g = 0; g < ps.group_count; ++g) {
      float4* gi = gimg + g * gimg_stride + at;
      float4 m = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (fc.u.frame_index != 0u) m = *gi;
      for (uint32_t k = 0; k < fc.samples; ++k) {
        const uint32_t slot = (k * fc.views + view) * fc.pixel_slots + pslot;
        const P3 lr = ps.groups[(size_t)g * ps.group_stride + slot];
        f3 S = mk3(lr.x, lr.y, lr.z);
        if (fc.u.env_type == 1u && g == ps.env_group) { const P3 le = ps.radiance_env[slot]; S = S + mk3(le.x, le.y, le.z); }
        if (!(isfinite(S.x) && isfinite(S.y) && isfinite(S.z))) S = splat3(0.0f);
        const uint32_t fi = fc.u.frame_index + k;
        m = make_float4(fold_mean(m.x, S.x, fi), fold_mean(m.y, S.y, fi), fold_mean(m.z, S.z, fi), 1.0f);
      }
      *gi = m;
    }
  if (AOV && ids && fc.u.frame_index == 0u) ids[at] = id;
  const f3 c = tonemap_select(mk3(a.x, a.y, a.z) * fc.u.exposure_value, fc.u.enable_tonemap, fc.u.enable_aces, fc.u.use_simple_aces);
  final_img[at] = make_float4(c.x, c.y, c.z, 1.0f);
}

// relight (RENDER_SPEC §14): R = sum over g ascending of s_g * I_g, from 0, one IEEE multiply and add per channel and group; the linear
// image and tonemap_select(R * exposure) exactly as k_resolve writes `final`.  One thread per pixel of one view.
__global__ void __launch_bounds__(256) k_relight(const float4* __restrict__ gimg, size_t gimg_stride, uint32_t group_count, RelightScales sc,
                                                 uint32_t n, hala_global_uniform u, float4* __restrict__ linear, float4* __restrict__ toned) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  f3 acc = splat3(0.0f);
  for (uint32_t g = 0; g < group_count; ++g) {
    const float4 v = gimg[g * gimg_stride + i];
    acc = acc + mk3(sc.s[g][0], sc.s[g][1], sc.s[g][2]) * mk3(v.x, v.y, v.z);
  }
  linear[i] = make_float4(acc.x, acc.y, acc.z, 1.0f);
  const f3 c = tonemap_select(acc * u.exposure_value, u.enable_tonemap, u.enable_aces, u.use_simple_aces);
  toned[i] = make_float4(c.x, c.y, c.z, 1.0f);
}

// stand-alone texture fetch (tests): uvl = (u, v, lod) per sample
__global__ void __launch_bounds__(256) k_sample_texture(SceneView sv, uint32_t tex, const float* __restrict__ uvl, uint32_t n, float4* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = tex_sample(sv, sv.tex_lut, tex, uvl[3 * i], uvl[3 * i + 1], uvl[3 * i + 2]);
}

// tile-major gathered buffer [world][tiles_per_rank][ts][ts] -> row-major full image (RENDER_SPEC §9)
__global__ void __launch_bounds__(256) k_scatter_tiles(FrameConst fc, const float4* __restrict__ gathered, float4* __restrict__ full) {
  const uint32_t gi = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t per_rank = fc.tiles_per_rank * fc.tile_size * fc.tile_size;
  if (gi >= per_rank * fc.world) return;
  FrameConst f2 = fc;
  f2.rank = gi / per_rank;
  uint32_t px, py;
  if (!slot_to_pixel(f2, gi - f2.rank * per_rank, &px, &py)) return;
  full[(size_t)py * fc.width + px] = gathered[gi];
}
void launch_resolve(const FrameConst& fc, const PathState& ps, float4* accum, float4* albedo, float4* normal, float4* final_img, float4* pos,
                    uint4* ids, float4* group_images, size_t group_stride, hipStream_t s) {
  dispatch<kFamilyResolve>([&](auto AOV, auto GROUPS) {
    hipLaunchKernelGGL((k_resolve<AOV, GROUPS>), dim3(blocks_for(fc.pixel_slots * fc.views, 256)), dim3(256), 0, s, fc, ps, accum, albedo, normal, final_img,
                       pos, ids, group_images, group_stride);
  }, pos != nullptr || ids != nullptr, ps.groups != nullptr);
}
void launch_relight(const hala_global_uniform& u, const float4* group_images, size_t group_stride, uint32_t group_count, const RelightScales& sc, uint32_t n,
                    float4* linear, float4* toned, hipStream_t s) {
  hipLaunchKernelGGL(k_relight, dim3(blocks_for(n, 256)), dim3(256), 0, s, group_images, group_stride, group_count, sc, n, u, linear, toned);
}
void launch_sample_texture(const SceneView& sv, uint32_t tex, const float* uvl, uint32_t n, float4* out, hipStream_t s) {
  hipLaunchKernelGGL(k_sample_texture, dim3(blocks_for(n, 256)), dim3(256), 0, s, sv, tex, uvl, n, out);
}
void launch_scatter_tiles(const FrameConst& fc, const float4* gathered, float4* full, hipStream_t s) {
  const uint32_t n = fc.tiles_per_rank * fc.tile_size * fc.tile_size * fc.world;
  hipLaunchKernelGGL(k_scatter_tiles, dim3(blocks_for(n, 256)), dim3(256), 0, s, fc, gathered, full);
}

}  // namespace rt
