// rt_bake.hip — bake maps (RENDER_SPEC 4.11): the contract of hala_rt_trace_rays (scratch, stream order, no host synchronisation in the
// device forms) around the kernels of bake.hip and, for a baked occlusion map, the occlusion kernels of occlusion.hip in between.  The
// samples never leave the device: the rasteriser writes them into a buffer the renderer owns, the occlusion kernels read them there.
// (Growing one of the renderer's buffers frees the old one, which waits for whoever still reads it.)
// Bake atlases (RENDER_SPEC 4.12) follow: the same around the atlas kernels, the owned-texel list and the listed occlusion pass.
// hala_rt_bake_occlusion keeps the plain pass: on a map without empty texels the listed one measured 0.5-3 % slower.
#include "renderer_state.h"

namespace {

int bake_check(hala_rt_renderer* r, const hala_bake_desc* d, const void* out) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!d) RT_FAIL("The bake description is null!");
  if (!out) RT_FAIL("The bake output is null!");
  if (!r->committed) RT_FAIL("The top level acceleration structure is none!");
  if (r->two_level) RT_FAIL("Bake maps are not built for two-level trees: commit the scene flattened (instancing = 0).");
  if (d->instance >= r->hs.instances.size()) RT_FAIL("The bake instance is out of range.");
  if (d->width == 0 || d->width > HALA_MAX_BAKE_DIM || d->height == 0 || d->height > HALA_MAX_BAKE_DIM)
    RT_FAIL("The bake map's dimensions must be 1.." + std::to_string(HALA_MAX_BAKE_DIM) + " each.");
  if (d->margin > HALA_MAX_BAKE_MARGIN) RT_FAIL("The bake margin must be 0.." + std::to_string(HALA_MAX_BAKE_MARGIN) + ".");
  if ((d->flags & ~(HALA_BAKE_SHADING_NORMAL | HALA_BAKE_FLIP_NORMAL)) != 0u) RT_FAIL("Unknown bake flags.");
  if (!std::isfinite(d->bias)) RT_FAIL("The bake bias must be finite.");
  return HALA_OK;
}
int bake_occlusion_check(hala_rt_renderer* r, const hala_bake_desc* d, const void* out, uint32_t rays) {
  if (bake_check(r, d, out) != HALA_OK) return HALA_ERR;
  if (rays == 0 || rays > HALA_MAX_OCCLUSION_RAYS) RT_FAIL("The occlusion ray count must be 1.." + std::to_string(HALA_MAX_OCCLUSION_RAYS) + ".");
  if ((uint64_t)d->width * d->height * rays >= (1ull << 32)) RT_FAIL("The bake map is too large for its ray count.");
  return HALA_OK;
}
// the view of a checked description and the renderer's scratch for it, grown where it is too small
int bake_prepare(hala_rt_renderer* r, const hala_bake_desc* d, rt::BakeView* bv, rt::BakeScratch* sc) {
  *bv = rt::BakeView{};
  bv->width = d->width; bv->height = d->height; bv->flags = d->flags; bv->margin = d->margin; bv->bias = d->bias; bv->reach = d->reach;
  bv->first_tri = r->hs.inst_first_tri[d->instance];
  bv->tri_count = r->hs.inst_first_tri[d->instance + 1u] - bv->first_tri;
  const size_t owner_words = rt::bake_owner_words(*bv), entries = (size_t)bv->tri_count + 1u, scan_bytes = rt::bake_scan_bytes(bv->tri_count);
  if (r->d_bake_owner.count < owner_words) { RT_HIP(r->d_bake_owner.resize(owner_words)); RT_HIP(r->d_bake_block_bits.resize(owner_words / 64u)); }
  if (r->d_bake_counts.count < entries) { RT_HIP(r->d_bake_counts.resize(entries)); RT_HIP(r->d_bake_offsets.resize(entries)); }
  if (r->d_bake_scan.count < scan_bytes || !r->d_bake_scan.ptr) RT_HIP(r->d_bake_scan.resize(scan_bytes));
  *sc = rt::BakeScratch{r->d_bake_owner.ptr, r->d_bake_counts.ptr, r->d_bake_offsets.ptr, r->d_bake_block_bits.ptr, r->d_bake_scan.ptr, scan_bytes};
  return HALA_OK;
}
// RENDER_SPEC 4.12: the refusals of an atlas, in the order the header lists them
int atlas_check(hala_rt_renderer* r, const hala_bake_atlas_desc* d, const hala_bake_chart* charts, const void* out) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!d) RT_FAIL("The bake atlas description is null!");
  if (!charts) RT_FAIL("The bake atlas chart table is null!");
  if (!out) RT_FAIL("The bake output is null!");
  if (!r->committed) RT_FAIL("The top level acceleration structure is none!");
  if (r->two_level) RT_FAIL("Bake maps are not built for two-level trees: commit the scene flattened (instancing = 0).");
  if (d->width == 0 || d->width > HALA_MAX_BAKE_DIM || d->height == 0 || d->height > HALA_MAX_BAKE_DIM)
    RT_FAIL("The bake map's dimensions must be 1.." + std::to_string(HALA_MAX_BAKE_DIM) + " each.");
  if (d->margin > HALA_MAX_BAKE_MARGIN) RT_FAIL("The bake margin must be 0.." + std::to_string(HALA_MAX_BAKE_MARGIN) + ".");
  if (!std::isfinite(d->bias)) RT_FAIL("The bake bias must be finite.");
  const size_t instances = r->hs.instances.size();
  if (d->chart_count == 0 || d->chart_count > instances) RT_FAIL("The bake atlas chart count must be 1.." + std::to_string(instances) + " (the scene's instances).");
  std::vector<uint8_t> seen(instances, 0);
  for (uint32_t k = 0; k < d->chart_count; ++k) {
    const hala_bake_chart& c = charts[k];
    if (c.instance >= instances) RT_FAIL("The bake instance is out of range (chart " + std::to_string(k) + ").");
    if (seen[c.instance]) RT_FAIL("A bake atlas names an instance once: instance " + std::to_string(c.instance) + " has two charts.");
    seen[c.instance] = 1;
    if ((c.flags & ~(HALA_BAKE_SHADING_NORMAL | HALA_BAKE_FLIP_NORMAL)) != 0u) RT_FAIL("Unknown bake flags (chart " + std::to_string(k) + ").");
    if (!all_finite(c.scale, 2) || !all_finite(c.offset, 2)) RT_FAIL("The scale and offset of a bake chart must be finite (chart " + std::to_string(k) + ").");
  }
  return HALA_OK;
}
int atlas_occlusion_check(hala_rt_renderer* r, const hala_bake_atlas_desc* d, const hala_bake_chart* charts, const void* out, uint32_t rays) {
  if (atlas_check(r, d, charts, out) != HALA_OK) return HALA_ERR;
  if (rays == 0 || rays > HALA_MAX_OCCLUSION_RAYS) RT_FAIL("The occlusion ray count must be 1.." + std::to_string(HALA_MAX_OCCLUSION_RAYS) + ".");
  if ((uint64_t)d->width * d->height * rays >= (1ull << 32)) RT_FAIL("The bake map is too large for its ray count.");
  return HALA_OK;
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
  const size_t owner_words = rt::bake_owner_words(*bv), entries = (size_t)bv->tri_count + 1u, blocks = owner_words / 64u;
  const size_t scan_bytes = std::max(rt::bake_scan_bytes(bv->tri_count), rt::bake_list_scan_bytes(blocks));
  if (r->d_bake_owner.count < owner_words) { RT_HIP(r->d_bake_owner.resize(owner_words)); RT_HIP(r->d_bake_block_bits.resize(blocks)); }
  if (r->d_bake_counts.count < entries) { RT_HIP(r->d_bake_counts.resize(entries)); RT_HIP(r->d_bake_offsets.resize(entries)); }
  if (r->d_bake_scan.count < scan_bytes || !r->d_bake_scan.ptr) RT_HIP(r->d_bake_scan.resize(scan_bytes));
  if (r->d_bake_charts.count < table->size()) RT_HIP(r->d_bake_charts.resize(table->size()));
  *sc = rt::BakeScratch{r->d_bake_owner.ptr, r->d_bake_counts.ptr, r->d_bake_offsets.ptr, r->d_bake_block_bits.ptr, r->d_bake_scan.ptr, scan_bytes};
  return HALA_OK;
}
int bake_done(hala_rt_renderer* r, hipStream_t s) {
  if (!r->scratch.batch_done) RT_HIP(hipEventCreateWithFlags(&r->scratch.batch_done, hipEventDisableTiming));
  RT_HIP(hipEventRecord(r->scratch.batch_done, s));
  r->scratch.event = r->scratch.batch_done; r->scratch.stream = s;
  RT_HIP(hipGetLastError());
  return HALA_OK;
}

}  // namespace

extern "C" {

int hala_rt_bake_samples(hala_rt_renderer* r, const hala_bake_desc* desc, hala_occlusion_sample* d_samples, hala_bake_texel* d_texels, void* hip_stream) {
  if (bake_check(r, desc, d_samples) != HALA_OK) return HALA_ERR;
  hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : r->stream;
  rt::BakeView bv;
  rt::BakeScratch sc;
  if (bake_prepare(r, desc, &bv, &sc) != HALA_OK) return HALA_ERR;
  if (r->scratch.acquire(s) != HALA_OK) return HALA_ERR;
  RT_HIP(rt::launch_bake_samples(r->view(), r->cu_count, bv, sc, d_samples, d_texels, s));
  return bake_done(r, s);
}
int hala_rt_bake_samples_host(hala_rt_renderer* r, const hala_bake_desc* desc, hala_occlusion_sample* samples, hala_bake_texel* texels) {
  if (bake_check(r, desc, samples) != HALA_OK) return HALA_ERR;
  const size_t n = (size_t)desc->width * desc->height;
  DeviceArray<hala_occlusion_sample> d_samples;
  DeviceArray<hala_bake_texel> d_texels;
  RT_HIP(d_samples.resize(n));
  if (texels) RT_HIP(d_texels.resize(n));
  if (hala_rt_bake_samples(r, desc, d_samples.ptr, texels ? d_texels.ptr : nullptr, r->stream) != HALA_OK) return HALA_ERR;
  RT_HIP(hipMemcpyAsync(samples, d_samples.ptr, n * sizeof(hala_occlusion_sample), hipMemcpyDeviceToHost, r->stream));
  if (texels) RT_HIP(hipMemcpyAsync(texels, d_texels.ptr, n * sizeof(hala_bake_texel), hipMemcpyDeviceToHost, r->stream));
  RT_HIP(hipStreamSynchronize(r->stream));
  return HALA_OK;
}
int hala_rt_bake_occlusion(hala_rt_renderer* r, const hala_bake_desc* desc, uint32_t rays, uint32_t seed, hala_occlusion* d_out, hala_bake_texel* d_texels,
                           void* hip_stream) {
  if (bake_occlusion_check(r, desc, d_out, rays) != HALA_OK) return HALA_ERR;
  hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : r->stream;
  rt::BakeView bv;
  rt::BakeScratch sc;
  if (bake_prepare(r, desc, &bv, &sc) != HALA_OK) return HALA_ERR;
  const uint32_t count = desc->width * desc->height;
  const size_t mask_words = (size_t)count * ((rays + 31u) / 32u);
  if (r->d_bake_samples.count < count) RT_HIP(r->d_bake_samples.resize(count));
  if (r->d_occlusion_masks.count < mask_words) RT_HIP(r->d_occlusion_masks.resize(mask_words));
  if (r->scratch.acquire(s) != HALA_OK) return HALA_ERR;
  const rt::SceneView sv = r->view();
  RT_HIP(rt::launch_bake_samples(sv, r->cu_count, bv, sc, r->d_bake_samples.ptr, d_texels, s));
  RT_HIP(hipMemsetAsync(r->d_batch_work.ptr, 0, sizeof(WorkCounters), s));
  RT_HIP(hipMemsetAsync(r->d_occlusion_masks.ptr, 0, mask_words * 4, s));
  rt::launch_trace_occlusion(r->lcfg, sv, r->d_bake_samples.ptr, d_out, r->d_occlusion_masks.ptr, count, rays, seed, r->d_batch_work.ptr, s);
  rt::launch_bake_dilate(bv, sc, d_out, d_texels, s);
  return bake_done(r, s);
}
int hala_rt_bake_occlusion_host(hala_rt_renderer* r, const hala_bake_desc* desc, uint32_t rays, uint32_t seed, hala_occlusion* out, hala_bake_texel* texels) {
  if (bake_occlusion_check(r, desc, out, rays) != HALA_OK) return HALA_ERR;
  const size_t n = (size_t)desc->width * desc->height;
  DeviceArray<hala_occlusion> d_out;
  DeviceArray<hala_bake_texel> d_texels;
  RT_HIP(d_out.resize(n));
  if (texels) RT_HIP(d_texels.resize(n));
  if (hala_rt_bake_occlusion(r, desc, rays, seed, d_out.ptr, texels ? d_texels.ptr : nullptr, r->stream) != HALA_OK) return HALA_ERR;
  RT_HIP(hipMemcpyAsync(out, d_out.ptr, n * sizeof(hala_occlusion), hipMemcpyDeviceToHost, r->stream));
  if (texels) RT_HIP(hipMemcpyAsync(texels, d_texels.ptr, n * sizeof(hala_bake_texel), hipMemcpyDeviceToHost, r->stream));
  RT_HIP(hipStreamSynchronize(r->stream));
  return HALA_OK;
}

// ---- RENDER_SPEC 4.12: bake atlases ------------------------------------------------------------------------------------------------------
int hala_rt_bake_atlas_samples(hala_rt_renderer* r, const hala_bake_atlas_desc* desc, const hala_bake_chart* charts, hala_occlusion_sample* d_samples,
                               hala_bake_texel* d_texels, void* hip_stream) {
  if (atlas_check(r, desc, charts, d_samples) != HALA_OK) return HALA_ERR;
  hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : r->stream;
  rt::BakeView bv;
  rt::BakeScratch sc;
  std::vector<rt::BakeChartDev> table;
  if (atlas_prepare(r, desc, charts, &bv, &sc, &table) != HALA_OK) return HALA_ERR;
  if (r->scratch.acquire(s) != HALA_OK) return HALA_ERR;
  RT_HIP(hipMemcpyAsync(r->d_bake_charts.ptr, table.data(), table.size() * sizeof(rt::BakeChartDev), hipMemcpyHostToDevice, s));  // (pageable: read before it returns)
  RT_HIP(rt::launch_bake_samples_atlas(r->view(), r->cu_count, bv, sc, r->d_bake_charts.ptr, d_samples, d_texels, s));
  return bake_done(r, s);
}
int hala_rt_bake_atlas_samples_host(hala_rt_renderer* r, const hala_bake_atlas_desc* desc, const hala_bake_chart* charts, hala_occlusion_sample* samples,
                                    hala_bake_texel* texels) {
  if (atlas_check(r, desc, charts, samples) != HALA_OK) return HALA_ERR;
  const size_t n = (size_t)desc->width * desc->height;
  DeviceArray<hala_occlusion_sample> d_samples;
  DeviceArray<hala_bake_texel> d_texels;
  RT_HIP(d_samples.resize(n));
  if (texels) RT_HIP(d_texels.resize(n));
  if (hala_rt_bake_atlas_samples(r, desc, charts, d_samples.ptr, texels ? d_texels.ptr : nullptr, r->stream) != HALA_OK) return HALA_ERR;
  RT_HIP(hipMemcpyAsync(samples, d_samples.ptr, n * sizeof(hala_occlusion_sample), hipMemcpyDeviceToHost, r->stream));
  if (texels) RT_HIP(hipMemcpyAsync(texels, d_texels.ptr, n * sizeof(hala_bake_texel), hipMemcpyDeviceToHost, r->stream));
  RT_HIP(hipStreamSynchronize(r->stream));
  return HALA_OK;
}
// The occlusion pass of an atlas traces the list of owned texels that the device builds from the owner map: an ownerless texel costs one
// 16-B store, no queue entry and no trip through the persistent loop's refill.
int hala_rt_bake_atlas_occlusion(hala_rt_renderer* r, const hala_bake_atlas_desc* desc, const hala_bake_chart* charts, uint32_t rays, uint32_t seed,
                                 hala_occlusion* d_out, hala_bake_texel* d_texels, void* hip_stream) {
  if (atlas_occlusion_check(r, desc, charts, d_out, rays) != HALA_OK) return HALA_ERR;
  hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : r->stream;
  rt::BakeView bv;
  rt::BakeScratch sc;
  std::vector<rt::BakeChartDev> table;
  if (atlas_prepare(r, desc, charts, &bv, &sc, &table) != HALA_OK) return HALA_ERR;
  const uint32_t count = desc->width * desc->height;
  const size_t mask_words = (size_t)count * ((rays + 31u) / 32u), blocks = rt::bake_owner_words(bv) / 64u;
  if (r->d_bake_samples.count < count) RT_HIP(r->d_bake_samples.resize(count));
  if (r->d_occlusion_masks.count < mask_words) RT_HIP(r->d_occlusion_masks.resize(mask_words));
  if (r->d_bake_list.count < count) RT_HIP(r->d_bake_list.resize(count));
  if (r->d_bake_list_counts.count < blocks + 1u) { RT_HIP(r->d_bake_list_counts.resize(blocks + 1u)); RT_HIP(r->d_bake_list_offsets.resize(blocks + 1u)); }
  const rt::BakeListScratch ls{r->d_bake_list.ptr, r->d_bake_list_counts.ptr, r->d_bake_list_offsets.ptr};
  if (r->scratch.acquire(s) != HALA_OK) return HALA_ERR;
  RT_HIP(hipMemcpyAsync(r->d_bake_charts.ptr, table.data(), table.size() * sizeof(rt::BakeChartDev), hipMemcpyHostToDevice, s));
  const rt::SceneView sv = r->view();
  RT_HIP(rt::launch_bake_samples_atlas(sv, r->cu_count, bv, sc, r->d_bake_charts.ptr, r->d_bake_samples.ptr, d_texels, s));
  RT_HIP(rt::launch_bake_list(bv, sc, ls, d_out, s));
  RT_HIP(hipMemsetAsync(r->d_batch_work.ptr, 0, sizeof(WorkCounters), s));
  RT_HIP(hipMemsetAsync(r->d_occlusion_masks.ptr, 0, mask_words * 4, s));
  rt::launch_trace_occlusion_listed(r->lcfg, sv, r->d_bake_samples.ptr, ls.list, ls.list_offsets + blocks, count, d_out, r->d_occlusion_masks.ptr, rays, seed,
                                    r->d_batch_work.ptr, s);
  rt::launch_bake_dilate(bv, sc, d_out, d_texels, s, true);
  return bake_done(r, s);
}
int hala_rt_bake_atlas_occlusion_host(hala_rt_renderer* r, const hala_bake_atlas_desc* desc, const hala_bake_chart* charts, uint32_t rays, uint32_t seed,
                                      hala_occlusion* out, hala_bake_texel* texels) {
  if (atlas_occlusion_check(r, desc, charts, out, rays) != HALA_OK) return HALA_ERR;
  const size_t n = (size_t)desc->width * desc->height;
  DeviceArray<hala_occlusion> d_out;
  DeviceArray<hala_bake_texel> d_texels;
  RT_HIP(d_out.resize(n));
  if (texels) RT_HIP(d_texels.resize(n));
  if (hala_rt_bake_atlas_occlusion(r, desc, charts, rays, seed, d_out.ptr, texels ? d_texels.ptr : nullptr, r->stream) != HALA_OK) return HALA_ERR;
  RT_HIP(hipMemcpyAsync(out, d_out.ptr, n * sizeof(hala_occlusion), hipMemcpyDeviceToHost, r->stream));
  if (texels) RT_HIP(hipMemcpyAsync(texels, d_texels.ptr, n * sizeof(hala_bake_texel), hipMemcpyDeviceToHost, r->stream));
  RT_HIP(hipStreamSynchronize(r->stream));
  return HALA_OK;
}

}  // extern "C"
