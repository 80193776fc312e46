// rt_outputs.hip — what a frame is made of besides the beauty image: views (RENDER_SPEC 12), first-hit AOVs (13), the adaptive
// sampling entry points (11), light groups and relighting (14, LightGroupState).
#include "renderer_state.h"

extern "C" {

int hala_rt_read_view_image(hala_rt_renderer* r, uint32_t view, int which, float* dst) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (view >= r->view_count()) RT_FAIL("The view does not exist (hala_rt_set_views set " + std::to_string(r->view_count()) + ").");
  if (view == 0u) return hala_rt_read_image(r, which, dst);
  if (!r->has_image(which) || !dst) RT_FAIL("Invalid image selector.");
  RT_HIP(hipStreamSynchronize(r->stream));
  const size_t px = r->image_pixels();  // several views: never sharded, the row-major frame
  RT_HIP(hipMemcpy(dst, r->img_local[which].ptr + view * px, px * sizeof(float4), hipMemcpyDeviceToHost));
  return HALA_OK;
}

// ---- views (RENDER_SPEC 12) ---------------------------------------------------------------------------------------------
int hala_rt_set_views(hala_rt_renderer* r, const uint32_t* camera_indices, uint32_t count) {
  if (!r) RT_FAIL("The renderer handle is null!");
  if (!camera_indices) RT_FAIL("hala_rt_set_views: the camera list is null.");
  if (count == 0 || count > kMaxViews) RT_FAIL("hala_rt_set_views: the view count must be in 1.." + std::to_string(kMaxViews) + ".");
  for (uint32_t v = 0; v < count; ++v)
    if (camera_indices[v] >= HALA_MAX_CAMERA_COUNT)
      RT_FAIL("hala_rt_set_views: camera index " + std::to_string(camera_indices[v]) + " is out of range (< " + std::to_string(HALA_MAX_CAMERA_COUNT) + ").");
  if (count > 1u && r->world > 1u) RT_FAIL("hala_rt_set_views: several views are not available on a sharded renderer (world > 1).");
  if (count > 1u && r->adaptive.enabled) RT_FAIL("hala_rt_set_views: several views are not available with adaptive sampling on.");
  if (count > 1u && r->temporal.enabled) RT_FAIL("hala_rt_set_views: several views are not available with temporal reprojection on.");
  if (ensure_device(r) != HALA_OK) return HALA_ERR;  // joins the second frame slot
  RT_HIP(hipStreamSynchronize(r->stream));
  const size_t old_n = r->image_alloc();
  std::vector<uint32_t> old_views = r->views;
  r->views.assign(camera_indices, camera_indices + count);
  const size_t n = r->image_alloc();
  // the images hold V views now: view 0 (and every view both lists have) keeps its pixels, new views start at zero.  Buffers only
  // ever grow, so that a failure half-way leaves every one large enough for either list.
  const size_t keep = std::min(old_n, n);
  for (int k = 0; k < 6; ++k) {
    if (!r->has_image(k)) continue;
    DeviceArray<float4>& img = r->img_local[k];
    hipError_t e = hipSuccess;
    if (img.count < n) {
      DeviceArray<float4> grown;
      e = grown.resize(n);
      if (e == hipSuccess) e = hipMemcpyAsync(grown.ptr, img.ptr, keep * sizeof(float4), hipMemcpyDeviceToDevice, r->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
      if (e == hipSuccess) { std::swap(img.ptr, grown.ptr); std::swap(img.count, grown.count); }
    }
    if (e == hipSuccess && n > keep) e = hipMemsetAsync(img.ptr + keep, 0, (n - keep) * sizeof(float4), r->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
    if (e != hipSuccess) { r->views = old_views; RT_HIP(e); }
  }
  if (r->groups.count) {  // light groups (RENDER_SPEC §14): every view's images, zero until its first update
    hipError_t e = r->groups.img.grow(n * r->groups.count);
    if (e == hipSuccess) e = hipMemsetAsync(r->groups.img.ptr, 0, r->groups.img.bytes(), r->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
    if (e != hipSuccess) { r->views = old_views; RT_HIP(e); }
  }
  r->invalidate(Changed::Views);
  r->reset_accumulation();
  return HALA_OK;
}

// ---- first-hit AOVs (RENDER_SPEC 13) ------------------------------------------------------------------------------------
int hala_rt_set_aovs(hala_rt_renderer* r, uint32_t mask) {
  if (!r) RT_FAIL("The renderer handle is null!");
  if (mask > 3u) RT_FAIL("hala_rt_set_aovs: unknown AOV bits (bit 0: position, bit 1: ids).");
  if (ensure_device(r) != HALA_OK) return HALA_ERR;  // joins the second frame slot
  if (r->exchange.pending && hala_rt_tile_allgather_finish(r) != HALA_OK) return HALA_ERR;  // an exchange in flight may stage images 4 and 5
  RT_HIP(hipStreamSynchronize(r->stream));
  if (r->exchange.stream) RT_HIP(hipStreamSynchronize(r->exchange.stream));
  const uint32_t old = r->aov_mask;
  r->aov_mask = mask;
  r->invalidate(Changed::Aovs);
  hipError_t e = hipSuccess;
  const size_t n = r->image_alloc();
  for (int k = 4; k < 6 && e == hipSuccess; ++k) {
    if (!r->has_image(k)) { r->img_local[k].release(); r->img_full[k].release(); r->exchange.stage[k].release(); r->exchange.recv[k].release(); continue; }
    if (r->img_local[k].count == n && ((old >> (k - 4)) & 1u)) continue;  // stays on: kept (the accumulation restarts below)
    e = r->img_local[k].resize(n);
    if (e == hipSuccess) e = hipMemsetAsync(r->img_local[k].ptr, 0, n * sizeof(float4), r->stream);
  }
  if (e == hipSuccess) e = r->fit_paths();  // the first-hit records of every path slot (§15 keeps the ids)
  if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
  if (e != hipSuccess) {  // out of memory: the AOVs are off, the other images are untouched
    r->aov_mask = 0;
    for (int k = 4; k < 6; ++k) r->img_local[k].release();
    (void)r->fit_paths();
    RT_HIP(e);
  }
  r->reset_accumulation();
  return HALA_OK;
}

// ---- adaptive sampling (RENDER_SPEC 11) -------------------------------------------------------------------------------------
int hala_rt_set_adaptive_sampling(hala_rt_renderer* r, const hala_adaptive_params* p) {
  if (p) {
    const std::string bad = adaptive_check_params(p);  // first: the CPU tier pins it without a renderer
    if (!bad.empty()) RT_FAIL(bad);
  }
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  AdaptiveState& ad = r->adaptive;
  if (p) {
    if (kPixelBlock != 8u) RT_FAIL("Adaptive sampling needs the 8 x 8 pixel blocks of RENDER_SPEC 9 (this build has RT_PIXEL_BLOCK = " + std::to_string(kPixelBlock) + ").");
    if (r->world > 1) RT_FAIL("Adaptive sampling is not available on a sharded renderer (world > 1).");
    if (r->view_count() > 1u) RT_FAIL("Adaptive sampling is not available with several views (hala_rt_set_views with one camera first).");
    if (r->temporal.enabled) RT_FAIL("Adaptive sampling is not available with temporal reprojection on (hala_rt_set_temporal(r, NULL) first).");
    if (r->shutter.rec.on || r->shutter.act.on) RT_FAIL("Adaptive sampling is not available with the shutter on (hala_rt_set_shutter(r, NULL) first).");
    if (!ad.enabled) {
      RT_HIP(hipStreamSynchronize(r->stream));
      const uint32_t blocks = r->blocks_x * ((r->height + kPixelBlock - 1) / kPixelBlock);
      RT_HIP(ad.ensure(blocks, (size_t)r->width * r->height));
    }
    ad.p = *p;
    ad.enabled = true;
  } else if (ad.enabled) {
    RT_HIP(hipStreamSynchronize(r->stream));
    ad.release();
    ad.enabled = false;
  }
  r->reset_accumulation();
  return HALA_OK;
}
int hala_rt_read_sample_counts(hala_rt_renderer* r, uint32_t* dst) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!dst) RT_FAIL("The output pointer is null!");
  const uint32_t n = r->rendered_frames();
  const size_t pixels = (size_t)r->width * r->height;
  const AdaptiveState& ad = r->adaptive;
  if (!ad.enabled || n == 0) { std::fill(dst, dst + pixels, n); return HALA_OK; }
  std::vector<uint32_t> c(ad.total_blocks);
  RT_HIP(hipStreamSynchronize(r->stream));
  RT_HIP(hipMemcpy(c.data(), ad.block_count.ptr, c.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  for (uint32_t y = 0; y < r->height; ++y)
    for (uint32_t x = 0; x < r->width; ++x) {
      const uint32_t cb = c[(y / kPixelBlock) * r->blocks_x + x / kPixelBlock];
      dst[(size_t)y * r->width + x] = cb ? cb : n;  // 0: still active
    }
  return HALA_OK;
}
int hala_rt_get_adaptive_status(hala_rt_renderer* r, hala_adaptive_status* out) {
  if (!r) RT_FAIL("The renderer handle is null!");
  if (!out) RT_FAIL("The output pointer is null!");
  memset(out, 0, sizeof(*out));
  const AdaptiveState& ad = r->adaptive;
  const uint32_t bh = kPixelBlock ? (r->height + kPixelBlock - 1) / kPixelBlock : 0u;
  out->enabled = ad.enabled ? 1u : 0u;
  out->total_blocks = ad.enabled ? ad.total_blocks : r->blocks_x * bh;
  out->active_blocks = ad.enabled ? ad.active_blocks : out->total_blocks;
  out->active_pixels = ad.enabled ? ad.active_pixels : r->width * r->height;
  out->samples = r->rendered_frames();
  out->last_snapshot = ad.enabled ? ad.last_snapshot : 0u;
  return HALA_OK;
}

// ---- light groups (RENDER_SPEC 14) ------------------------------------------------------------------------------------------
static std::string light_groups_check(const hala_light_groups* g) {
  if (g->group_count == 0 || g->group_count > kMaxLightGroups)
    return "hala_rt_set_light_groups: group_count must be in 1.." + std::to_string(kMaxLightGroups) + ".";
  if ((g->light_count && !g->light_group) || (g->material_count && !g->material_group))
    return "hala_rt_set_light_groups: a table is null but its count is not 0.";
  if (g->environment_group >= g->group_count) return "hala_rt_set_light_groups: the environment's group is out of range (>= group_count).";
  for (uint32_t k = 0; k < g->light_count; ++k)
    if (g->light_group[k] >= g->group_count) return "hala_rt_set_light_groups: the group of light " + std::to_string(k) + " is out of range (>= group_count).";
  for (uint32_t k = 0; k < g->material_count; ++k)
    if (g->material_group[k] >= g->group_count)
      return "hala_rt_set_light_groups: the group of material " + std::to_string(k) + " is out of range (>= group_count).";
  return "";
}
int hala_rt_set_light_groups(hala_rt_renderer* r, const hala_light_groups* g) {
  if (g) {
    const std::string bad = light_groups_check(g);  // first: the CPU tier pins it without a renderer
    if (!bad.empty()) RT_FAIL(bad);
  }
  if (!r) RT_FAIL("The renderer handle is null!");
  if (g && r->world > 1) RT_FAIL("hala_rt_set_light_groups: light groups are not available on a sharded renderer (world > 1).");
  if (g && r->path_shape().paths > kGroupSlotMask)
    RT_FAIL("hala_rt_set_light_groups: light groups need fewer than 2^29 path slots (pixels x samples x views).");
  if (ensure_device(r) != HALA_OK) return HALA_ERR;  // joins the second frame slot
  RT_HIP(hipStreamSynchronize(r->stream));
  r->groups.off();
  if (g) r->groups.count = g->group_count;
  hipError_t e = r->fit_paths();  // one radiance sum per path slot and group; off: freed
  if (g) {
    if (e == hipSuccess) e = r->groups.img.resize(r->image_alloc() * g->group_count);
    if (e == hipSuccess) e = hipMemsetAsync(r->groups.img.ptr, 0, r->groups.img.bytes(), r->stream);
    if (e == hipSuccess) e = r->groups.d_light_group.upload(g->light_group, g->light_count, r->stream);
    if (e == hipSuccess) e = r->groups.d_material_group.upload(g->material_group, g->material_count, r->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
    if (e != hipSuccess) { r->groups.off(); (void)r->fit_paths(); RT_HIP(e); }  // out of memory: the groups are off, the other images are untouched
    r->groups.env_group = g->environment_group;
    r->groups.light_group.assign(g->light_group, g->light_group + g->light_count);
    r->groups.material_group.assign(g->material_group, g->material_group + g->material_count);
  }
  r->reset_accumulation();
  return HALA_OK;
}
static int light_group_view_check(hala_rt_renderer* r, uint32_t view) {
  if (!r) RT_FAIL("The renderer handle is null!");
  if (!r->groups.count) RT_FAIL("Light groups are off (hala_rt_set_light_groups).");
  if (view >= r->view_count()) RT_FAIL("The view does not exist (hala_rt_set_views set " + std::to_string(r->view_count()) + ").");
  return HALA_OK;
}
int hala_rt_read_light_group(hala_rt_renderer* r, uint32_t view, uint32_t group, float* dst) {
  if (light_group_view_check(r, view) != HALA_OK) return HALA_ERR;
  if (group >= r->groups.count) RT_FAIL("The light group does not exist (hala_rt_set_light_groups set " + std::to_string(r->groups.count) + ").");
  if (!dst) RT_FAIL("The output pointer is null!");
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  RT_HIP(hipStreamSynchronize(r->stream));
  const size_t px = r->image_pixels();  // never sharded: the row-major frame
  RT_HIP(hipMemcpy(dst, r->groups.img.ptr + group * r->image_alloc() + view * px, px * sizeof(float4), hipMemcpyDeviceToHost));
  return HALA_OK;
}
int hala_rt_relight(hala_rt_renderer* r, uint32_t view, const float* rgb_scales, uint32_t group_count) {
  if (light_group_view_check(r, view) != HALA_OK) return HALA_ERR;
  if (group_count != r->groups.count) RT_FAIL("hala_rt_relight: group_count must be the light groups' count (" + std::to_string(r->groups.count) + ").");
  if (!rgb_scales) RT_FAIL("hala_rt_relight: the scales are null.");
  RelightScales sc{};
  for (uint32_t k = 0; k < 3u * group_count; ++k) {
    if (!std::isfinite(rgb_scales[k])) RT_FAIL("hala_rt_relight: the scales must be finite.");
    sc.s[k / 3u][k % 3u] = rgb_scales[k];
  }
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  const size_t px = r->image_pixels();
  RT_HIP(r->groups.relit[0].resize(px)); RT_HIP(r->groups.relit[1].resize(px));
  hala_global_uniform u{};
  r->output_settings(&u);
  launch_relight(u, r->groups.img.ptr + view * px, r->image_alloc(), r->groups.count, sc, (uint32_t)px, r->groups.relit[0].ptr, r->groups.relit[1].ptr, r->stream);
  RT_HIP(hipGetLastError());
  r->groups.relit_valid = true;
  return HALA_OK;
}
int hala_rt_read_relit(hala_rt_renderer* r, int which, float* dst) {
  if (!r) RT_FAIL("The renderer handle is null!");
  if (which < 0 || which > 1 || !dst) RT_FAIL("Invalid argument.");
  if (!r->groups.relit_valid) RT_FAIL("Nothing relit: call hala_rt_relight while light groups are on first.");
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  RT_HIP(hipStreamSynchronize(r->stream));
  RT_HIP(hipMemcpy(dst, r->groups.relit[which].ptr, r->groups.relit[which].bytes(), hipMemcpyDeviceToHost));
  return HALA_OK;
}
int hala_rt_get_relit_buffer(hala_rt_renderer* r, int which, void** d_ptr, size_t* bytes) {
  if (!r) RT_FAIL("The renderer handle is null!");
  if (which < 0 || which > 1 || !d_ptr || !bytes) RT_FAIL("Invalid argument.");
  if (!r->groups.relit_valid) RT_FAIL("Nothing relit: call hala_rt_relight while light groups are on first.");
  *d_ptr = r->groups.relit[which].ptr;
  *bytes = r->groups.relit[which].bytes();
  return HALA_OK;
}

}  // extern "C"
