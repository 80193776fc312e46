// rt_bake.hip — bake maps (RENDER_SPEC 4.11): the contract of hala_rt_trace_rays (scratch, stream order, no host synchronisation in the
// device forms) around the kernels of bake.hip and, for a baked occlusion map, the occlusion kernels of occlusion.hip in between.  The
// samples never leave the device: the rasteriser writes them into a buffer the renderer owns, the occlusion kernels read them there.
// (Growing one of the renderer's buffers frees the old one, which waits for whoever still reads it.)
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

}  // extern "C"
