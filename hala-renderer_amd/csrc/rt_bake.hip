// rt_bake.hip — bake maps (RENDER_SPEC 4.11): a BatchScope (renderer_state.h: the renderer's scratch, stream order, no host
// synchronisation in the device forms) around the kernels of bake.hip and, for a baked occlusion map, the occlusion kernels of
// occlusion.hip in between.  The samples never leave the device: the rasteriser writes them into a buffer the renderer owns, the occlusion
// kernels read them there.  (Growing one of the renderer's buffers frees the old one, which waits for whoever still reads it.)
// Bake atlases (RENDER_SPEC 4.12) follow: the same around the atlas kernels, the owned-texel list and the listed occlusion pass.
// hala_rt_bake_occlusion keeps the plain pass: on a map without empty texels the listed one measured 0.5-3 % slower.
// Transfer bakes (RENDER_SPEC 4.13) come last: the rasteriser, then the filtered closest-hit trace of trace_transfer.hip, then the dilation.
#include "renderer_state.h"

namespace {

constexpr uint32_t kBakeFlags = HALA_BAKE_SHADING_NORMAL | HALA_BAKE_FLIP_NORMAL;
// what a map and an atlas refuse alike, in the order both headers list it.  unknown_flags: a map's (a chart of an atlas has its own)
int bake_map_check(uint32_t width, uint32_t height, uint32_t margin, uint32_t unknown_flags, float bias) {
  if (width == 0 || width > HALA_MAX_BAKE_DIM || height == 0 || height > HALA_MAX_BAKE_DIM)
    RT_FAIL("The bake map's dimensions must be 1.." + std::to_string(HALA_MAX_BAKE_DIM) + " each.");
  if (margin > HALA_MAX_BAKE_MARGIN) RT_FAIL("The bake margin must be 0.." + std::to_string(HALA_MAX_BAKE_MARGIN) + ".");
  if (unknown_flags != 0u) RT_FAIL("Unknown bake flags.");
  if (!std::isfinite(bias)) RT_FAIL("The bake bias must be finite.");
  return HALA_OK;
}
int bake_rays_check(uint32_t width, uint32_t height, uint32_t rays) {
  if (check_occlusion_rays(rays) != HALA_OK) return HALA_ERR;
  return check_occlusion_size((uint64_t)width * height, rays, "The bake map is too large for its ray count.");
}
int bake_check(hala_rt_renderer* r, const hala_bake_desc* d, const void* out) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!d) RT_FAIL("The bake description is null!");
  if (!out) RT_FAIL("The bake output is null!");
  if (check_committed(r, "Bake maps") != HALA_OK) return HALA_ERR;
  if (d->instance >= r->hs.instances.size()) RT_FAIL("The bake instance is out of range.");
  return bake_map_check(d->width, d->height, d->margin, d->flags & ~kBakeFlags, d->bias);
}
int bake_occlusion_check(hala_rt_renderer* r, const hala_bake_desc* d, const void* out, uint32_t rays) {
  if (bake_check(r, d, out) != HALA_OK) return HALA_ERR;
  return bake_rays_check(d->width, d->height, rays);
}
// the renderer's scratch for a view, grown where it is too small: what a map and an atlas both need
int bake_scratch(hala_rt_renderer* r, const rt::BakeView& bv, size_t scan_bytes, rt::BakeScratch* sc) {
  const size_t owner_words = rt::bake_owner_words(bv), entries = (size_t)bv.tri_count + 1u;
  RT_HIP(r->d_bake_owner.grow(owner_words));
  RT_HIP(r->d_bake_block_bits.grow(owner_words / 64u));
  RT_HIP(r->d_bake_counts.grow(entries));
  RT_HIP(r->d_bake_offsets.grow(entries));
  RT_HIP(r->d_bake_scan.grow(scan_bytes));
  *sc = rt::BakeScratch{r->d_bake_owner.ptr, r->d_bake_counts.ptr, r->d_bake_offsets.ptr, r->d_bake_block_bits.ptr, r->d_bake_scan.ptr, scan_bytes};
  return HALA_OK;
}
// the view of a checked description and the renderer's scratch for it
int bake_prepare(hala_rt_renderer* r, const hala_bake_desc* d, rt::BakeView* bv, rt::BakeScratch* sc) {
  *bv = rt::BakeView{};
  bv->width = d->width; bv->height = d->height; bv->flags = d->flags; bv->margin = d->margin; bv->bias = d->bias; bv->reach = d->reach;
  bv->first_tri = r->hs.inst_first_tri[d->instance];
  bv->tri_count = r->hs.inst_first_tri[d->instance + 1u] - bv->first_tri;
  return bake_scratch(r, *bv, rt::bake_scan_bytes(bv->tri_count), sc);
}
// RENDER_SPEC 4.12: the refusals of an atlas, in the order the header lists them
int atlas_check(hala_rt_renderer* r, const hala_bake_atlas_desc* d, const hala_bake_chart* charts, const void* out) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!d) RT_FAIL("The bake atlas description is null!");
  if (!charts) RT_FAIL("The bake atlas chart table is null!");
  if (!out) RT_FAIL("The bake output is null!");
  if (check_committed(r, "Bake maps") != HALA_OK) return HALA_ERR;
  if (bake_map_check(d->width, d->height, d->margin, 0u, d->bias) != HALA_OK) return HALA_ERR;
  const size_t instances = r->hs.instances.size();
  if (d->chart_count == 0 || d->chart_count > instances) RT_FAIL("The bake atlas chart count must be 1.." + std::to_string(instances) + " (the scene's instances).");
  std::vector<uint8_t> seen(instances, 0);
  for (uint32_t k = 0; k < d->chart_count; ++k) {
    const hala_bake_chart& c = charts[k];
    if (c.instance >= instances) RT_FAIL("The bake instance is out of range (chart " + std::to_string(k) + ").");
    if (seen[c.instance]) RT_FAIL("A bake atlas names an instance once: instance " + std::to_string(c.instance) + " has two charts.");
    seen[c.instance] = 1;
    if ((c.flags & ~kBakeFlags) != 0u) RT_FAIL("Unknown bake flags (chart " + std::to_string(k) + ").");
    if (!all_finite(c.scale, 2) || !all_finite(c.offset, 2)) RT_FAIL("The scale and offset of a bake chart must be finite (chart " + std::to_string(k) + ").");
  }
  return HALA_OK;
}
int atlas_occlusion_check(hala_rt_renderer* r, const hala_bake_atlas_desc* d, const hala_bake_chart* charts, const void* out, uint32_t rays) {
  if (atlas_check(r, d, charts, out) != HALA_OK) return HALA_ERR;
  return bake_rays_check(d->width, d->height, rays);
}
// The view of a checked atlas, the renderer's scratch for it and the per-instance chart table, which is read here: the caller's array is
// not needed once this returns.  The view's triangles are the span of the charted instances' ranges — one count / scan / cover over it, the
// triangles of uncharted instances in between counting no pairs — so that an atlas of one instance does the work of its 4.11 map.
int atlas_prepare(hala_rt_renderer* r, const hala_bake_atlas_desc* d, const hala_bake_chart* charts, rt::BakeView* bv, rt::BakeScratch* sc,
                  std::vector<rt::BakeChartDev>* table) {
  table->assign(r->hs.instances.size(), rt::BakeChartDev{});
  uint32_t lo = 0xffffffffu, hi = 0u;
  for (uint32_t k = 0; k < d->chart_count; ++k) {
    const hala_bake_chart& c = charts[k];
    (*table)[c.instance] = rt::BakeChartDev{c.scale[0], c.scale[1], c.offset[0], c.offset[1], c.flags, 1u, 0u, 0u};
    lo = std::min(lo, r->hs.inst_first_tri[c.instance]); hi = std::max(hi, r->hs.inst_first_tri[c.instance + 1u]);
  }
  *bv = rt::BakeView{};
  bv->width = d->width; bv->height = d->height; bv->margin = d->margin; bv->bias = d->bias; bv->reach = d->reach;
  bv->first_tri = lo; bv->tri_count = hi - lo;
  const size_t scan_bytes = std::max(rt::bake_scan_bytes(bv->tri_count), rt::bake_list_scan_bytes(rt::bake_owner_words(*bv) / 64u));
  if (bake_scratch(r, *bv, scan_bytes, sc) != HALA_OK) return HALA_ERR;
  RT_HIP(r->d_bake_charts.grow(table->size()));
  return HALA_OK;
}
// RENDER_SPEC 4.13: the refusals of a transfer — those of hala_rt_bake_samples first, with their texts, then its own in the order the
// header lists them — and the target set as merged, sorted [lo, hi) ranges of global triangle ids (instances own contiguous ranges in
// instance order; a target without triangles adds none; `ranges` null: the checks alone, for the host form).  `targets` is read here: the
// caller's array is not needed once this returns.
int transfer_check(hala_rt_renderer* r, const hala_bake_desc* d, const hala_bake_transfer_desc* t, const uint32_t* targets, const void* out,
                   std::vector<uint2>* ranges) {
  if (bake_check(r, d, out) != HALA_OK) return HALA_ERR;
  if (!t) RT_FAIL("The bake transfer description is null!");
  if (t->flags != 0u) RT_FAIL("Unknown bake transfer flags.");
  if (!std::isfinite(t->front) || t->front < 0.0f) RT_FAIL("The front distance of a bake transfer must be finite and not negative.");
  if (std::isnan(t->back) || t->back < 0.0f) RT_FAIL("The back distance of a bake transfer must be +inf or a number that is not negative.");
  const size_t instances = r->hs.instances.size();
  if (t->target_count > instances) RT_FAIL("The bake transfer target count must be 0.." + std::to_string(instances) + " (the scene's instances).");
  if (t->target_count != 0u && !targets) RT_FAIL("The bake transfer target list is null!");
  std::vector<uint8_t> is_target(instances, t->target_count == 0u ? 1 : 0);
  if (t->target_count == 0u) {
    if (instances < 2u) RT_FAIL("The bake transfer has no targets: the receiver is the scene's only instance.");
    is_target[d->instance] = 0;
  }
  for (uint32_t k = 0; k < t->target_count; ++k) {
    const uint32_t i = targets[k];
    if (i >= instances) RT_FAIL("A bake transfer target is out of range (target " + std::to_string(k) + ").");
    if (is_target[i]) RT_FAIL("A bake transfer names a target once: instance " + std::to_string(i) + " is named twice.");
    if (i == d->instance) RT_FAIL("The receiver of a bake transfer cannot be one of its targets (instance " + std::to_string(i) + ").");
    is_target[i] = 1;
  }
  if (!ranges) return HALA_OK;
  ranges->clear();
  for (size_t i = 0; i < instances; ++i) {
    const uint32_t lo = r->hs.inst_first_tri[i], hi = r->hs.inst_first_tri[i + 1u];
    if (!is_target[i] || lo == hi) continue;
    if (!ranges->empty() && ranges->back().y == lo) ranges->back().y = hi;
    else ranges->push_back(make_uint2(lo, hi));
  }
  return HALA_OK;
}
// The host form of the bakes: `call(d_out, d_texels)` is the device form on the renderer's stream
template <class Rec, class Call>
int bake_host(hala_rt_renderer* r, uint32_t width, uint32_t height, Rec* out, hala_bake_texel* texels, Call call) {
  const size_t n = (size_t)width * height;
  HostOut<Rec> d_out(out, n);
  HostOut<hala_bake_texel> d_texels(texels, n);
  return host_form(r->stream, [&] { return call(d_out.ptr(), d_texels.ptr()); }, d_out, d_texels);
}

}  // namespace

extern "C" {

int hala_rt_bake_samples(hala_rt_renderer* r, const hala_bake_desc* desc, hala_occlusion_sample* d_samples, hala_bake_texel* d_texels, void* hip_stream) {
  if (bake_check(r, desc, d_samples) != HALA_OK) return HALA_ERR;
  rt::BakeView bv;
  rt::BakeScratch sc;
  if (bake_prepare(r, desc, &bv, &sc) != HALA_OK) return HALA_ERR;
  BatchScope scope = r->batch(hip_stream);
  if (scope.open() != HALA_OK) return HALA_ERR;
  RT_HIP(rt::launch_bake_samples(r->view(), r->cu_count, bv, sc, d_samples, d_texels, scope.s));
  return scope.close();
}
int hala_rt_bake_samples_host(hala_rt_renderer* r, const hala_bake_desc* desc, hala_occlusion_sample* samples, hala_bake_texel* texels) {
  if (bake_check(r, desc, samples) != HALA_OK) return HALA_ERR;
  return bake_host(r, desc->width, desc->height, samples, texels,
                   [&](hala_occlusion_sample* d_samples, hala_bake_texel* d_texels) { return hala_rt_bake_samples(r, desc, d_samples, d_texels, r->stream); });
}
int hala_rt_bake_occlusion(hala_rt_renderer* r, const hala_bake_desc* desc, uint32_t rays, uint32_t seed, hala_occlusion* d_out, hala_bake_texel* d_texels,
                           void* hip_stream) {
  if (bake_occlusion_check(r, desc, d_out, rays) != HALA_OK) return HALA_ERR;
  rt::BakeView bv;
  rt::BakeScratch sc;
  if (bake_prepare(r, desc, &bv, &sc) != HALA_OK) return HALA_ERR;
  const uint32_t count = desc->width * desc->height;
  const size_t mask_words = (size_t)count * ((rays + 31u) / 32u);
  RT_HIP(r->d_bake_samples.grow(count));
  RT_HIP(r->d_occlusion_masks.grow(mask_words));
  BatchScope scope = r->batch(hip_stream);
  if (scope.open() != HALA_OK) return HALA_ERR;
  hipStream_t s = scope.s;
  const rt::SceneView sv = r->view();
  RT_HIP(rt::launch_bake_samples(sv, r->cu_count, bv, sc, r->d_bake_samples.ptr, d_texels, s));
  if (scope.reset_work() != HALA_OK) return HALA_ERR;
  RT_HIP(hipMemsetAsync(r->d_occlusion_masks.ptr, 0, mask_words * 4, s));
  rt::launch_trace_occlusion(r->lcfg, sv, r->d_bake_samples.ptr, d_out, r->d_occlusion_masks.ptr, count, rays, seed, r->d_batch_work.ptr, s);
  rt::launch_bake_dilate(bv, sc, d_out, d_texels, s);
  return scope.close();
}
int hala_rt_bake_occlusion_host(hala_rt_renderer* r, const hala_bake_desc* desc, uint32_t rays, uint32_t seed, hala_occlusion* out, hala_bake_texel* texels) {
  if (bake_occlusion_check(r, desc, out, rays) != HALA_OK) return HALA_ERR;
  return bake_host(r, desc->width, desc->height, out, texels,
                   [&](hala_occlusion* d_out, hala_bake_texel* d_texels) { return hala_rt_bake_occlusion(r, desc, rays, seed, d_out, d_texels, r->stream); });
}

// ---- RENDER_SPEC 4.12: bake atlases ------------------------------------------------------------------------------------------------------
int hala_rt_bake_atlas_samples(hala_rt_renderer* r, const hala_bake_atlas_desc* desc, const hala_bake_chart* charts, hala_occlusion_sample* d_samples,
                               hala_bake_texel* d_texels, void* hip_stream) {
  if (atlas_check(r, desc, charts, d_samples) != HALA_OK) return HALA_ERR;
  rt::BakeView bv;
  rt::BakeScratch sc;
  std::vector<rt::BakeChartDev> table;
  if (atlas_prepare(r, desc, charts, &bv, &sc, &table) != HALA_OK) return HALA_ERR;
  BatchScope scope = r->batch(hip_stream);
  if (scope.open() != HALA_OK) return HALA_ERR;
  RT_HIP(hipMemcpyAsync(r->d_bake_charts.ptr, table.data(), table.size() * sizeof(rt::BakeChartDev), hipMemcpyHostToDevice, scope.s));  // (pageable: read before it returns)
  RT_HIP(rt::launch_bake_samples_atlas(r->view(), r->cu_count, bv, sc, r->d_bake_charts.ptr, d_samples, d_texels, scope.s));
  return scope.close();
}
int hala_rt_bake_atlas_samples_host(hala_rt_renderer* r, const hala_bake_atlas_desc* desc, const hala_bake_chart* charts, hala_occlusion_sample* samples,
                                    hala_bake_texel* texels) {
  if (atlas_check(r, desc, charts, samples) != HALA_OK) return HALA_ERR;
  return bake_host(r, desc->width, desc->height, samples, texels, [&](hala_occlusion_sample* d_samples, hala_bake_texel* d_texels) {
    return hala_rt_bake_atlas_samples(r, desc, charts, d_samples, d_texels, r->stream);
  });
}
// The occlusion pass of an atlas traces the list of owned texels that the device builds from the owner map: an ownerless texel costs one
// 16-B store, no queue entry and no trip through the persistent loop's refill.
int hala_rt_bake_atlas_occlusion(hala_rt_renderer* r, const hala_bake_atlas_desc* desc, const hala_bake_chart* charts, uint32_t rays, uint32_t seed,
                                 hala_occlusion* d_out, hala_bake_texel* d_texels, void* hip_stream) {
  if (atlas_occlusion_check(r, desc, charts, d_out, rays) != HALA_OK) return HALA_ERR;
  rt::BakeView bv;
  rt::BakeScratch sc;
  std::vector<rt::BakeChartDev> table;
  if (atlas_prepare(r, desc, charts, &bv, &sc, &table) != HALA_OK) return HALA_ERR;
  const uint32_t count = desc->width * desc->height;
  const size_t mask_words = (size_t)count * ((rays + 31u) / 32u), blocks = rt::bake_owner_words(bv) / 64u;
  RT_HIP(r->d_bake_samples.grow(count));
  RT_HIP(r->d_occlusion_masks.grow(mask_words));
  RT_HIP(r->d_bake_list.grow(count));
  RT_HIP(r->d_bake_list_counts.grow(blocks + 1u));
  RT_HIP(r->d_bake_list_offsets.grow(blocks + 1u));
  const rt::BakeListScratch ls{r->d_bake_list.ptr, r->d_bake_list_counts.ptr, r->d_bake_list_offsets.ptr};
  BatchScope scope = r->batch(hip_stream);
  if (scope.open() != HALA_OK) return HALA_ERR;
  hipStream_t s = scope.s;
  RT_HIP(hipMemcpyAsync(r->d_bake_charts.ptr, table.data(), table.size() * sizeof(rt::BakeChartDev), hipMemcpyHostToDevice, s));
  const rt::SceneView sv = r->view();
  RT_HIP(rt::launch_bake_samples_atlas(sv, r->cu_count, bv, sc, r->d_bake_charts.ptr, r->d_bake_samples.ptr, d_texels, s));
  RT_HIP(rt::launch_bake_list(bv, sc, ls, d_out, s));
  if (scope.reset_work() != HALA_OK) return HALA_ERR;
  RT_HIP(hipMemsetAsync(r->d_occlusion_masks.ptr, 0, mask_words * 4, s));
  rt::launch_trace_occlusion_listed(r->lcfg, sv, r->d_bake_samples.ptr, ls.list, ls.list_offsets + blocks, count, d_out, r->d_occlusion_masks.ptr, rays, seed,
                                    r->d_batch_work.ptr, s);
  rt::launch_bake_dilate(bv, sc, d_out, d_texels, s, true);
  return scope.close();
}
int hala_rt_bake_atlas_occlusion_host(hala_rt_renderer* r, const hala_bake_atlas_desc* desc, const hala_bake_chart* charts, uint32_t rays, uint32_t seed,
                                      hala_occlusion* out, hala_bake_texel* texels) {
  if (atlas_occlusion_check(r, desc, charts, out, rays) != HALA_OK) return HALA_ERR;
  return bake_host(r, desc->width, desc->height, out, texels, [&](hala_occlusion* d_out, hala_bake_texel* d_texels) {
    return hala_rt_bake_atlas_occlusion(r, desc, charts, rays, seed, d_out, d_texels, r->stream);
  });
}

// ---- RENDER_SPEC 4.13: transfer bakes ----------------------------------------------------------------------------------------------------
// One scope around the rasteriser (into the renderer's sample buffer), the transfer trace with its resolve, and the dilation.  Every
// texel goes to the trace's queue: an ownerless one has the all-zero sample, which the ray load rejects at the cost of one 32-B load and
// one 16-B store — a transfer traces ONE ray per texel, so the owned-texel list of 4.12 (three kernels and a scan ahead of the trace)
// has nothing like the N rays per texel of an occlusion pass to win back.
int hala_rt_bake_transfer(hala_rt_renderer* r, const hala_bake_desc* desc, const hala_bake_transfer_desc* transfer, const uint32_t* targets,
                          hala_bake_transfer_hit* d_out, hala_bake_texel* d_texels, void* hip_stream) {
  std::vector<uint2> ranges;
  if (transfer_check(r, desc, transfer, targets, d_out, &ranges) != HALA_OK) return HALA_ERR;
  rt::BakeView bv;
  rt::BakeScratch sc;
  if (bake_prepare(r, desc, &bv, &sc) != HALA_OK) return HALA_ERR;
  const uint32_t count = desc->width * desc->height;
  RT_HIP(r->d_bake_samples.grow(count));
  rt::TransferTargets tg{(uint32_t)ranges.size(), 0u, 0u, 0u, 0u, nullptr};
  if (ranges.size() > 2u) RT_HIP(r->d_bake_targets.grow(ranges.size()));
  else {
    if (ranges.size() > 0u) { tg.lo0 = ranges[0].x; tg.hi0 = ranges[0].y; }
    if (ranges.size() > 1u) { tg.lo1 = ranges[1].x; tg.hi1 = ranges[1].y; }
  }
  BatchScope scope = r->batch(hip_stream);
  if (scope.open() != HALA_OK) return HALA_ERR;
  hipStream_t s = scope.s;
  if (ranges.size() > 2u) {
    RT_HIP(hipMemcpyAsync(r->d_bake_targets.ptr, ranges.data(), ranges.size() * sizeof(uint2), hipMemcpyHostToDevice, s));  // (pageable: read before it returns)
    tg.table = r->d_bake_targets.ptr;
  }
  const rt::SceneView sv = r->view();
  RT_HIP(rt::launch_bake_samples(sv, r->cu_count, bv, sc, r->d_bake_samples.ptr, d_texels, s));
  if (scope.reset_work() != HALA_OK) return HALA_ERR;
  const float tmax = transfer->front + transfer->back;  // one float add; +inf stays +inf
  const bool fits = rt::launch_trace_transfer(r->lcfg, sv, r->cu_count, r->d_bake_samples.ptr, tg, transfer->front, tmax, d_out, count, r->d_batch_work.ptr, s);
  if (fits) rt::launch_bake_dilate_transfer(bv, sc, d_out, d_texels, s);
  return scope.close(fits ? nullptr : "The transfer traversal kernel does not fit on a compute unit.");
}
int hala_rt_bake_transfer_host(hala_rt_renderer* r, const hala_bake_desc* desc, const hala_bake_transfer_desc* transfer, const uint32_t* targets,
                               hala_bake_transfer_hit* out, hala_bake_texel* texels) {
  if (transfer_check(r, desc, transfer, targets, out, nullptr) != HALA_OK) return HALA_ERR;
  return bake_host(r, desc->width, desc->height, out, texels, [&](hala_bake_transfer_hit* d_out, hala_bake_texel* d_texels) {
    return hala_rt_bake_transfer(r, desc, transfer, targets, d_out, d_texels, r->stream);
  });
}

}  // extern "C"
