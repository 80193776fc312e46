// rt_rays.hip — what works without a frame: the ray-batch operator on the committed scene's tree, the hala_rtprog object over it,
// and the stand-alone helpers of the C ABI (environment distribution, tonemap, hash, image files).
#include "renderer_state.h"

extern "C" {

// ---- ray-batch operator ------------------------------------------------------------------------------------------------
int hala_rt_trace_rays(hala_rt_renderer* r, const hala_ray* d_rays, hala_hit* d_hits, uint32_t count, int mode, uint64_t* d_counters, void* hip_stream) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!r->committed) RT_FAIL("The top level acceleration structure is none!");  // src/rt_renderer.rs:284
  if (mode != 0 && mode != 1) RT_FAIL("Invalid trace mode.");
  if (count == 0) return HALA_OK;
  if (!d_rays || !d_hits) RT_FAIL("The ray batch is null!");
  hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : r->stream;
  if (r->scratch.acquire(s) != HALA_OK) return HALA_ERR;  // stream-ordered behind the previous user of the renderer's scratch (include/halart.h)
  RT_HIP(hipMemsetAsync(r->d_batch_work.ptr, 0, sizeof(WorkCounters), s));
  // counters: the kernel accumulates into the control block's 64-bit fields; copy them out if requested
  if (d_counters) RT_HIP(hipMemsetAsync(&r->d_ctl.ptr->totals.steps[mode][0], 0, 16, s));
  // RENDER_SPEC 4.2: far origins are re-based where the batch enters, and the distance comes back on the closest hits where it leaves —
  // the traversal launch in between sees ordinary rays.  (Growing the copy frees the old one, which waits for whoever still reads it.)
  if (r->d_batch_rays.count < count) { RT_HIP(r->d_batch_rays.resize(count)); RT_HIP(r->d_batch_moved.resize(count)); }
  const SceneView sv = r->view();
  launch_rebase_batch(sv, d_rays, r->d_batch_rays.ptr, r->d_batch_moved.ptr, count, s);
  launch_trace_batch(r->lcfg, sv, r->d_batch_rays.ptr, d_hits, nullptr, count, r->d_batch_work.ptr, r->d_ctl.ptr, mode == 1, d_counters != nullptr, false, s);
  if (mode == 0) launch_unbase_hits(d_hits, r->d_batch_moved.ptr, count, s);
  if (d_counters) RT_HIP(hipMemcpyAsync(d_counters, &r->d_ctl.ptr->totals.steps[mode][0], 16, hipMemcpyDeviceToDevice, s));
  if (!r->scratch.batch_done) RT_HIP(hipEventCreateWithFlags(&r->scratch.batch_done, hipEventDisableTiming));
  RT_HIP(hipEventRecord(r->scratch.batch_done, s));
  r->scratch.event = r->scratch.batch_done; r->scratch.stream = s;
  RT_HIP(hipGetLastError());
  return HALA_OK;
}
// RENDER_SPEC 4.7: the contract of hala_rt_trace_rays (scratch, stream order, the renderer's own re-based copy of the batch) around the
// multi-hit kernel; the distance a far ray was moved comes back on every record of its list
int hala_rt_trace_rays_multi(hala_rt_renderer* r, const hala_ray* d_rays, hala_hit* d_hits, uint32_t* d_counts, uint32_t count, uint32_t k, void* hip_stream) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!r->committed) RT_FAIL("The top level acceleration structure is none!");
  if (k == 0 || k > HALA_MAX_MULTI_HITS) RT_FAIL("The multi-hit capacity must be 1.." + std::to_string(HALA_MAX_MULTI_HITS) + ".");
  if (count == 0) return HALA_OK;
  if (!d_rays || !d_hits) RT_FAIL("The ray batch is null!");
  if ((uint64_t)count * k > (1ull << 32)) RT_FAIL("The multi-hit batch is too large.");
  hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : r->stream;
  if (r->scratch.acquire(s) != HALA_OK) return HALA_ERR;
  RT_HIP(hipMemsetAsync(r->d_batch_work.ptr, 0, sizeof(WorkCounters), s));
  if (r->d_batch_rays.count < count) { RT_HIP(r->d_batch_rays.resize(count)); RT_HIP(r->d_batch_moved.resize(count)); }
  const SceneView sv = r->view();
  launch_rebase_batch(sv, d_rays, r->d_batch_rays.ptr, r->d_batch_moved.ptr, count, s);
  const bool fits = launch_trace_multi(r->lcfg, sv, r->cu_count, r->d_batch_rays.ptr, d_hits, d_counts, count, k, r->d_batch_work.ptr, s);
  if (fits) launch_unbase_multi(d_hits, r->d_batch_moved.ptr, count, k, s);
  if (!r->scratch.batch_done) RT_HIP(hipEventCreateWithFlags(&r->scratch.batch_done, hipEventDisableTiming));
  RT_HIP(hipEventRecord(r->scratch.batch_done, s));
  r->scratch.event = r->scratch.batch_done; r->scratch.stream = s;
  if (!fits) RT_FAIL("The multi-hit traversal kernel does not fit on a compute unit.");
  RT_HIP(hipGetLastError());
  return HALA_OK;
}
int hala_rt_trace_rays_multi_host(hala_rt_renderer* r, const hala_ray* rays, hala_hit* hits, uint32_t* counts, uint32_t count, uint32_t k) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!r->committed) RT_FAIL("The top level acceleration structure is none!");
  if (k == 0 || k > HALA_MAX_MULTI_HITS) RT_FAIL("The multi-hit capacity must be 1.." + std::to_string(HALA_MAX_MULTI_HITS) + ".");
  if (count == 0) return HALA_OK;
  if (!rays || !hits) RT_FAIL("The ray batch is null!");
  if ((uint64_t)count * k > (1ull << 32)) RT_FAIL("The multi-hit batch is too large.");
  DeviceArray<hala_ray> d_rays;
  DeviceArray<hala_hit> d_hits;
  DeviceArray<uint32_t> d_counts;
  RT_HIP(d_rays.upload(rays, count, r->stream));
  RT_HIP(d_hits.resize((size_t)count * k));
  if (counts) RT_HIP(d_counts.resize(count));
  if (hala_rt_trace_rays_multi(r, d_rays.ptr, d_hits.ptr, counts ? d_counts.ptr : nullptr, count, k, r->stream) != HALA_OK) return HALA_ERR;
  RT_HIP(hipMemcpyAsync(hits, d_hits.ptr, (size_t)count * k * sizeof(hala_hit), hipMemcpyDeviceToHost, r->stream));
  if (counts) RT_HIP(hipMemcpyAsync(counts, d_counts.ptr, (size_t)count * 4, hipMemcpyDeviceToHost, r->stream));
  RT_HIP(hipStreamSynchronize(r->stream));
  return HALA_OK;
}
// RENDER_SPEC 4.8: the contract of hala_rt_trace_rays (scratch, stream order) around the closest-point kernel.  Nothing is re-based: the
// kernel reads the caller's queries.  d_counters (2 x uint64, or null): node visits and triangle tests of the batch.
int hala_rt_closest_points_counted(hala_rt_renderer* r, const hala_point_query* d_queries, hala_closest_point* d_out, uint32_t count,
                                   uint64_t* d_counters, void* hip_stream) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!r->committed) RT_FAIL("The top level acceleration structure is none!");
  if (r->two_level) RT_FAIL("Closest-point queries are not built for two-level trees: commit the scene flattened (instancing = 0).");
  if (count == 0) return HALA_OK;
  if (!d_queries || !d_out) RT_FAIL("The query batch is null!");
  hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : r->stream;
  if (r->scratch.acquire(s) != HALA_OK) return HALA_ERR;
  RT_HIP(hipMemsetAsync(r->d_batch_work.ptr, 0, sizeof(WorkCounters), s));
  if (d_counters) RT_HIP(hipMemsetAsync(d_counters, 0, 16, s));
  const bool fits = launch_closest_point(r->lcfg, r->view(), r->cu_count, d_queries, d_out, count, r->d_batch_work.ptr,
                                         reinterpret_cast<unsigned long long*>(d_counters), s);
  if (!r->scratch.batch_done) RT_HIP(hipEventCreateWithFlags(&r->scratch.batch_done, hipEventDisableTiming));
  RT_HIP(hipEventRecord(r->scratch.batch_done, s));
  r->scratch.event = r->scratch.batch_done; r->scratch.stream = s;
  if (!fits) RT_FAIL("The closest-point kernel does not fit on a compute unit.");
  RT_HIP(hipGetLastError());
  return HALA_OK;
}
int hala_rt_closest_points(hala_rt_renderer* r, const hala_point_query* d_queries, hala_closest_point* d_out, uint32_t count, void* hip_stream) {
  return hala_rt_closest_points_counted(r, d_queries, d_out, count, nullptr, hip_stream);
}
int hala_rt_closest_points_host(hala_rt_renderer* r, const hala_point_query* queries, hala_closest_point* out, uint32_t count) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!r->committed) RT_FAIL("The top level acceleration structure is none!");
  if (r->two_level) RT_FAIL("Closest-point queries are not built for two-level trees: commit the scene flattened (instancing = 0).");
  if (count == 0) return HALA_OK;
  if (!queries || !out) RT_FAIL("The query batch is null!");
  DeviceArray<hala_point_query> d_queries;
  DeviceArray<hala_closest_point> d_out;
  RT_HIP(d_queries.upload(queries, count, r->stream));
  RT_HIP(d_out.resize(count));
  if (hala_rt_closest_points(r, d_queries.ptr, d_out.ptr, count, r->stream) != HALA_OK) return HALA_ERR;
  RT_HIP(hipMemcpyAsync(out, d_out.ptr, (size_t)count * sizeof(hala_closest_point), hipMemcpyDeviceToHost, r->stream));
  RT_HIP(hipStreamSynchronize(r->stream));
  return HALA_OK;
}
// RENDER_SPEC 4.9.  Which distance kernel an automatic grid runs (DESIGN.md 28 has the measurements the rule rests on).  The per-wave
// walk runs, in every lane, the union of what its 64 voxels need, and saves the wave its node and triangle fetches.  It wins where those
// fetches come from memory (not a staged tree), where the band does not end a query early (it spans the scene box) and where the voxels
// are fine against the scene: spacing * sqrt(triangles) <= 4.4 x the box's largest extent.  Everywhere else a voxel per lane.
static uint32_t grid_auto_method(const SceneView& sv, const hala_distance_grid_desc* g) {
  if (sv.staged) return 1u;
  const float extent = std::max(sv.box_max[0] - sv.box_min[0], std::max(sv.box_max[1] - sv.box_min[1], sv.box_max[2] - sv.box_min[2]));
  if (!(g->band >= extent)) return 1u;
  return g->spacing * std::sqrt((float)sv.tri_count) <= 4.4f * extent ? 2u : 1u;
}
static int grid_check(hala_rt_renderer* r, const hala_distance_grid_desc* g, const void* distance) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!g) RT_FAIL("The distance grid description is null!");
  if (!distance) RT_FAIL("The distance grid output is null!");
  if (!r->committed) RT_FAIL("The top level acceleration structure is none!");
  if (r->two_level) RT_FAIL("Distance grids are not built for two-level trees: commit the scene flattened (instancing = 0).");
  for (int a = 0; a < 3; ++a)
    if (g->dims[a] == 0 || g->dims[a] > 1024u) RT_FAIL("The distance grid's dims must be 1..1024 each.");
  if (!(std::isfinite(g->spacing) && g->spacing > 0.0f)) RT_FAIL("The distance grid's spacing must be finite and positive.");
  if (!(g->band >= 0.0f)) RT_FAIL("The distance grid's band must be >= 0 or +inf.");
  if ((g->flags & ~7u) != 0u || ((g->flags >> HALA_GRID_METHOD_SHIFT) & 3u) == 3u) RT_FAIL("Unknown distance grid flags.");
  return HALA_OK;
}
// The contract of hala_rt_trace_rays (scratch, stream order) around the row pass of a signed grid and the distance pass; the rows' bits
// live in a buffer the renderer owns (growing it frees the old one, which waits for whoever still reads it).
int hala_rt_distance_grid_counted(hala_rt_renderer* r, const hala_distance_grid_desc* desc, float* d_distance, uint32_t* d_prim, uint64_t* d_counters,
                                  void* hip_stream) {
  if (grid_check(r, desc, d_distance) != HALA_OK) return HALA_ERR;
  GridView g{};
  memcpy(g.origin, desc->origin, sizeof(g.origin));
  g.spacing = desc->spacing; g.band = desc->band; g.nx = desc->dims[0]; g.ny = desc->dims[1]; g.nz = desc->dims[2];
  g.words = (g.nx + 1u + 31u) / 32u;
  const bool is_signed = (desc->flags & HALA_GRID_SIGNED) != 0u;
  uint32_t method = (desc->flags >> HALA_GRID_METHOD_SHIFT) & 3u;
  const SceneView sv = r->view();
  if (method == 0u) method = grid_auto_method(sv, desc);
  hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : r->stream;
  const size_t bit_words = (size_t)g.ny * g.nz * g.words;
  if (is_signed && r->d_grid_bits.count < bit_words) RT_HIP(r->d_grid_bits.resize(bit_words));
  if (r->scratch.acquire(s) != HALA_OK) return HALA_ERR;
  unsigned long long* counters = reinterpret_cast<unsigned long long*>(d_counters);
  if (d_counters) RT_HIP(hipMemsetAsync(d_counters, 0, 48, s));
  bool fits = true;
  if (is_signed) {
    RT_HIP(hipMemsetAsync(r->d_batch_work.ptr, 0, sizeof(WorkCounters), s));
    RT_HIP(hipMemsetAsync(r->d_grid_bits.ptr, 0, bit_words * 4, s));
    fits = launch_grid_rows(r->lcfg, sv, r->cu_count, g, r->d_grid_bits.ptr, r->d_batch_work.ptr, counters, s);
  }
  if (fits) {
    RT_HIP(hipMemsetAsync(r->d_batch_work.ptr, 0, sizeof(WorkCounters), s));
    fits = launch_distance_grid(r->lcfg, sv, r->cu_count, g, method, d_distance, d_prim, is_signed ? r->d_grid_bits.ptr : nullptr, r->d_batch_work.ptr, counters, s);
  }
  if (!r->scratch.batch_done) RT_HIP(hipEventCreateWithFlags(&r->scratch.batch_done, hipEventDisableTiming));
  RT_HIP(hipEventRecord(r->scratch.batch_done, s));
  r->scratch.event = r->scratch.batch_done; r->scratch.stream = s;
  if (!fits) RT_FAIL("The distance grid kernels do not fit on a compute unit.");
  RT_HIP(hipGetLastError());
  return HALA_OK;
}
int hala_rt_distance_grid(hala_rt_renderer* r, const hala_distance_grid_desc* desc, float* d_distance, uint32_t* d_prim, void* hip_stream) {
  return hala_rt_distance_grid_counted(r, desc, d_distance, d_prim, nullptr, hip_stream);
}
int hala_rt_distance_grid_host(hala_rt_renderer* r, const hala_distance_grid_desc* desc, float* distance, uint32_t* prim) {
  if (grid_check(r, desc, distance) != HALA_OK) return HALA_ERR;
  const size_t n = (size_t)desc->dims[0] * desc->dims[1] * desc->dims[2];
  DeviceArray<float> d_distance;
  DeviceArray<uint32_t> d_prim;
  RT_HIP(d_distance.resize(n));
  if (prim) RT_HIP(d_prim.resize(n));
  if (hala_rt_distance_grid(r, desc, d_distance.ptr, prim ? d_prim.ptr : nullptr, r->stream) != HALA_OK) return HALA_ERR;
  RT_HIP(hipMemcpyAsync(distance, d_distance.ptr, n * 4, hipMemcpyDeviceToHost, r->stream));
  if (prim) RT_HIP(hipMemcpyAsync(prim, d_prim.ptr, n * 4, hipMemcpyDeviceToHost, r->stream));
  RT_HIP(hipStreamSynchronize(r->stream));
  return HALA_OK;
}
// RENDER_SPEC 4.10: the contract of hala_rt_trace_rays (scratch, stream order) around the occlusion kernels.  Nothing is copied or
// re-based ahead of the launch: the rays are made, far origins included, in the lanes that trace them.  Without the caller's mask array
// the words live in a buffer the renderer owns (growing it frees the old one, which waits for whoever still reads it).
static int occlusion_check(hala_rt_renderer* r, const void* samples, const void* out, uint32_t count, uint32_t rays) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!r->committed) RT_FAIL("The top level acceleration structure is none!");
  if (rays == 0 || rays > HALA_MAX_OCCLUSION_RAYS) RT_FAIL("The occlusion ray count must be 1.." + std::to_string(HALA_MAX_OCCLUSION_RAYS) + ".");
  if (count == 0) return HALA_OK;
  if (!samples || !out) RT_FAIL("The occlusion batch is null!");
  if ((uint64_t)count * rays >= (1ull << 32)) RT_FAIL("The occlusion batch is too large.");
  return HALA_OK;
}
int hala_rt_occlusion(hala_rt_renderer* r, const hala_occlusion_sample* d_samples, hala_occlusion* d_out, uint32_t* d_masks, uint32_t count, uint32_t rays,
                      uint32_t seed, void* hip_stream) {
  if (occlusion_check(r, d_samples, d_out, count, rays) != HALA_OK) return HALA_ERR;
  if (count == 0) return HALA_OK;
  hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : r->stream;
  const size_t mask_words = (size_t)count * ((rays + 31u) / 32u);
  if (!d_masks) {
    if (r->d_occlusion_masks.count < mask_words) RT_HIP(r->d_occlusion_masks.resize(mask_words));
    d_masks = r->d_occlusion_masks.ptr;
  }
  if (r->scratch.acquire(s) != HALA_OK) return HALA_ERR;
  RT_HIP(hipMemsetAsync(r->d_batch_work.ptr, 0, sizeof(WorkCounters), s));
  RT_HIP(hipMemsetAsync(d_masks, 0, mask_words * 4, s));
  launch_trace_occlusion(r->lcfg, r->view(), d_samples, d_out, d_masks, count, rays, seed, r->d_batch_work.ptr, s);
  if (!r->scratch.batch_done) RT_HIP(hipEventCreateWithFlags(&r->scratch.batch_done, hipEventDisableTiming));
  RT_HIP(hipEventRecord(r->scratch.batch_done, s));
  r->scratch.event = r->scratch.batch_done; r->scratch.stream = s;
  RT_HIP(hipGetLastError());
  return HALA_OK;
}
int hala_rt_occlusion_host(hala_rt_renderer* r, const hala_occlusion_sample* samples, hala_occlusion* out, uint32_t* masks, uint32_t count, uint32_t rays,
                           uint32_t seed) {
  if (occlusion_check(r, samples, out, count, rays) != HALA_OK) return HALA_ERR;
  if (count == 0) return HALA_OK;
  const size_t mask_words = (size_t)count * ((rays + 31u) / 32u);
  DeviceArray<hala_occlusion_sample> d_samples;
  DeviceArray<hala_occlusion> d_out;
  DeviceArray<uint32_t> d_masks;
  RT_HIP(d_samples.upload(samples, count, r->stream));
  RT_HIP(d_out.resize(count));
  if (masks) RT_HIP(d_masks.resize(mask_words));
  if (hala_rt_occlusion(r, d_samples.ptr, d_out.ptr, masks ? d_masks.ptr : nullptr, count, rays, seed, r->stream) != HALA_OK) return HALA_ERR;
  RT_HIP(hipMemcpyAsync(out, d_out.ptr, (size_t)count * sizeof(hala_occlusion), hipMemcpyDeviceToHost, r->stream));
  if (masks) RT_HIP(hipMemcpyAsync(masks, d_masks.ptr, mask_words * 4, hipMemcpyDeviceToHost, r->stream));
  RT_HIP(hipStreamSynchronize(r->stream));
  return HALA_OK;
}
int hala_rt_trace_rays_indirect(hala_rt_renderer* r, const hala_ray* d_rays, hala_hit* d_hits, const uint32_t* d_indirect, int mode, void* hip_stream) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!d_indirect) RT_FAIL("The indirect command address is null!");
  hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : r->stream;
  uint32_t whd[3] = {0, 0, 0};
  RT_HIP(hipMemcpyAsync(whd, d_indirect, 12, hipMemcpyDeviceToHost, s));
  RT_HIP(hipStreamSynchronize(s));
  const uint64_t n = (uint64_t)whd[0] * whd[1] * whd[2];
  if (n > 0xffffffffull) RT_FAIL("The indirect launch is too large.");
  return hala_rt_trace_rays(r, d_rays, d_hits, (uint32_t)n, mode, nullptr, hip_stream);
}
int hala_rt_trace_rays_host(hala_rt_renderer* r, const hala_ray* rays, hala_hit* hits, uint32_t count, int mode, uint64_t counters[2]) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (count == 0) return HALA_OK;
  DeviceArray<hala_ray> d_rays;
  DeviceArray<hala_hit> d_hits;
  DeviceArray<uint64_t> d_ctr;
  RT_HIP(d_rays.upload(rays, count, r->stream));
  RT_HIP(d_hits.resize(count));
  if (counters) RT_HIP(d_ctr.resize(2));
  if (hala_rt_trace_rays(r, d_rays.ptr, d_hits.ptr, count, mode, counters ? d_ctr.ptr : nullptr, r->stream) != HALA_OK) return HALA_ERR;
  RT_HIP(hipMemcpyAsync(hits, d_hits.ptr, (size_t)count * sizeof(hala_hit), hipMemcpyDeviceToHost, r->stream));
  if (counters) RT_HIP(hipMemcpyAsync(counters, d_ctr.ptr, 16, hipMemcpyDeviceToHost, r->stream));
  RT_HIP(hipStreamSynchronize(r->stream));
  return HALA_OK;
}

// ---- stand-alone pieces ---------------------------------------------------------------------------------------------------
int hala_envmap_build_distribution(int device_ordinal, const float* rgba32f, uint32_t width, uint32_t height, float* total_sum, float* marginal, float* conditional) {
  if (!rgba32f || !total_sum || !marginal || !conditional || !width || !height) RT_FAIL("Invalid argument.");
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) RT_FAIL("No HIP device is available: libhalart has no CPU path.");
  RT_HIP(hipSetDevice(device_ordinal));
  DeviceArray<float4> d_px;
  DeviceArray<float> d_total, d_m, d_c;
  const size_t n = (size_t)width * height;
  RT_HIP(d_px.upload(reinterpret_cast<const float4*>(rgba32f), n, nullptr));
  RT_HIP(d_total.resize(1)); RT_HIP(d_m.resize(height)); RT_HIP(d_c.resize(n));
  const std::string e = envmap_build_distribution(d_px.ptr, width, height, d_total.ptr, d_m.ptr, d_c.ptr, nullptr);
  if (!e.empty()) RT_FAIL(e);
  RT_HIP(hipMemcpy(total_sum, d_total.ptr, 4, hipMemcpyDeviceToHost));
  RT_HIP(hipMemcpy(marginal, d_m.ptr, (size_t)height * 4, hipMemcpyDeviceToHost));
  RT_HIP(hipMemcpy(conditional, d_c.ptr, n * 4, hipMemcpyDeviceToHost));
  return HALA_OK;
}

void hala_tonemap_pixels(float* rgba32f, size_t pixel_count, int enable_tonemap, int enable_aces, int use_simple_aces) {
  if (rgba32f) tonemap_pixels(rgba32f, pixel_count, enable_tonemap, enable_aces, use_simple_aces);
}
int hala_cryptomatte_hash(const char* name, uint32_t* raw, uint32_t* id) {
  if (!name) RT_FAIL("The name is null!");
  const uint32_t h = murmur3_32(name, strlen(name), 0u);  // RENDER_SPEC 15: seed 0
  if (raw) *raw = h;
  if (id) *id = crypto_id(h);
  return HALA_OK;
}
int hala_write_exr(const char* path, uint32_t width, uint32_t height, uint32_t channel_count, const char* const* channel_names,
                   const float* const* planes, uint32_t attribute_count, const char* const* attr_names, const char* const* attr_values) {
  const std::string e = write_exr(path, width, height, channel_count, channel_names, planes, attribute_count, attr_names, attr_values);
  if (!e.empty()) RT_FAIL(e);
  return HALA_OK;
}
int hala_write_pfm(const char* path, const float* rgba32f, uint32_t width, uint32_t height) {
  if (!path || !rgba32f) RT_FAIL("Invalid argument.");
  const std::string e = write_pfm(path, rgba32f, width, height);
  if (!e.empty()) RT_FAIL(e);
  return HALA_OK;
}

int hala_load_float_image(const char* path, uint32_t* width, uint32_t* height, uint32_t* channels, float* dst, size_t capacity_floats) {
  if (!path || !width || !height || !channels) RT_FAIL("Invalid argument.");
  HostImage img;
  const std::string e = load_float_image(path, &img);
  if (!e.empty()) RT_FAIL(e);
  *width = img.width; *height = img.height; *channels = img.channels;
  if (dst) {
    if (capacity_floats < img.pixels.size()) RT_FAIL("The destination buffer is too small.");
    memcpy(dst, img.pixels.data(), img.pixels.size() * sizeof(float));
  }
  return HALA_OK;
}

int hala_rtprog_parse_desc(const char* desc_json, hala_rtprog_desc_info* out) {
  // serde field names and defaults of HalaRayTracingProgramDesc (src/raytracing_program.rs:33-55)
  if (!desc_json || !out) RT_FAIL("Invalid argument.");
  JsonValue root;
  const std::string e = json_parse(desc_json, &root);
  if (!e.empty()) RT_FAIL("Failed to parse the ray tracing program description: " + e);
  if (root.kind != JsonValue::Object) RT_FAIL("The ray tracing program description is not an object.");
  auto string_array = [&](const char* key, bool required, uint32_t* n) -> int {
    const JsonValue* v = root.find(key);
    if (!v) { if (required) RT_FAIL(std::string("missing field `") + key + "`"); *n = 0; return HALA_OK; }
    if (v->kind != JsonValue::Array) RT_FAIL(std::string("field `") + key + "` is not an array");
    for (const auto& it : v->items) if (it.kind != JsonValue::String) RT_FAIL(std::string("field `") + key + "` must hold strings");
    *n = (uint32_t)v->items.size();
    return HALA_OK;
  };
  memset(out, 0, sizeof(*out));
  if (string_array("raygen_shader_file_paths", true, &out->raygen_count) != HALA_OK) return HALA_ERR;
  if (string_array("miss_shader_file_paths", false, &out->miss_count) != HALA_OK) return HALA_ERR;
  if (string_array("callable_shader_file_paths", false, &out->callable_count) != HALA_OK) return HALA_ERR;
  if (string_array("bindings", false, &out->binding_count) != HALA_OK) return HALA_ERR;
  const JsonValue* hits = root.find("hit_shader_file_paths");
  if (!hits) RT_FAIL("missing field `hit_shader_file_paths`");
  if (hits->kind != JsonValue::Array) RT_FAIL("field `hit_shader_file_paths` is not an array");
  for (const auto& h : hits->items) {
    if (h.kind != JsonValue::Object) RT_FAIL("a hit shader description is not an object");
    for (const auto& m : h.members) {
      if (m.first != "closest_hit_shader_file_path" && m.first != "any_hit_shader_file_path" && m.first != "intersection_shader_file_path") continue;
      if (m.second.kind != JsonValue::String && m.second.kind != JsonValue::Null) RT_FAIL("field `" + m.first + "` must be a string or null");
    }
  }
  out->hit_count = (uint32_t)hits->items.size();
  auto u32_field = [&](const char* key, uint32_t def, uint32_t* dst) -> int {
    const JsonValue* v = root.find(key);
    if (!v) { *dst = def; return HALA_OK; }
    if (v->kind != JsonValue::Number || v->num < 0 || v->num > 4294967295.0 || v->num != std::floor(v->num)) RT_FAIL(std::string("field `") + key + "` is not a u32");
    *dst = (uint32_t)v->num;
    return HALA_OK;
  };
  if (u32_field("push_constant_size", 0, &out->push_constant_size) != HALA_OK) return HALA_ERR;
  if (u32_field("ray_recursion_depth", 1, &out->ray_recursion_depth) != HALA_OK) return HALA_ERR;  // default_ray_recursion_depth :53-55
  return HALA_OK;
}


// ---- HalaRayTracingProgram (src/raytracing_program.rs:70-341) as an object of the C ABI -------------------------------------------------
// Reference: {shader groups, pipeline, SBT}; bind() attaches descriptor sets, push_constants() writes the constant block, trace_rays(w, h, d)
// launches w*h*d ray-gen invocations against the acceleration structure the descriptor sets name.  Here the shader groups are the library's
// traversal kernels (the SPIR-V paths of the description are recorded, as hala_rt_push_*_shader does), the "descriptor sets" are the device
// buffers of one ray batch, and the acceleration structure is the committed renderer's.  Bytes 0..3 of the constant block select the
// hit-group behaviour: 0 = closest hit, 1 = any hit.
struct hala_rtprog {
  hala_rt_renderer* renderer = nullptr;
  hala_rtprog_desc_info info{};
  std::string debug_name;
  std::vector<uint8_t> constants;
  const hala_ray* d_rays = nullptr;
  hala_hit* d_hits = nullptr;
};

int hala_rtprog_create(hala_rt_renderer* r, const char* desc_json, const char* debug_name, hala_rtprog** out) {
  if (!out) RT_FAIL("The output handle is null!");
  *out = nullptr;
  if (!r) RT_FAIL("The renderer handle is null!");
  hala_rtprog_desc_info info;
  if (hala_rtprog_parse_desc(desc_json, &info) != HALA_OK) return HALA_ERR;
  if (info.raygen_count == 0) RT_FAIL("The raygen shader list is empty!");  // a pipeline without a ray generation group cannot be built (:85-106)
  if (info.push_constant_size % 4u != 0u) RT_FAIL("push_constant_size must be a multiple of 4.");  // VkPushConstantRange.size
  std::unique_ptr<hala_rtprog> p(new hala_rtprog());
  p->renderer = r; p->info = info; p->debug_name = debug_name ? debug_name : "";
  p->constants.assign(std::max<uint32_t>(info.push_constant_size, 4u), 0);
  *out = p.release();
  return HALA_OK;
}
void hala_rtprog_destroy(hala_rtprog* p) { delete p; }
int hala_rtprog_get_desc_info(const hala_rtprog* p, hala_rtprog_desc_info* out) {
  if (!p || !out) RT_FAIL("Invalid argument.");
  *out = p->info;
  return HALA_OK;
}
int hala_rtprog_bind(hala_rtprog* p, const hala_ray* d_rays, hala_hit* d_hits) {  // :264-278
  if (!p) RT_FAIL("The program handle is null!");
  if (!d_rays || !d_hits) RT_FAIL("The ray batch is null!");
  p->d_rays = d_rays; p->d_hits = d_hits;
  return HALA_OK;
}
int hala_rtprog_push_constants(hala_rtprog* p, uint32_t offset, const void* data, size_t len) {  // :285-300
  if (!p) RT_FAIL("The program handle is null!");
  if (!data && len) RT_FAIL("Invalid argument.");
  if ((size_t)offset + len > p->constants.size()) RT_FAIL("The push constant range exceeds push_constant_size.");
  if (len) memcpy(p->constants.data() + offset, data, len);
  return HALA_OK;
}
int hala_rtprog_push_constants_f32(hala_rtprog* p, uint32_t offset, const float* data, size_t count) {  // :307-322
  return hala_rtprog_push_constants(p, offset, data, count * sizeof(float));
}
static int rtprog_mode(const hala_rtprog* p) {
  uint32_t m = 0;
  memcpy(&m, p->constants.data(), 4);
  return (int)(m & 1u);
}
int hala_rtprog_trace_rays(hala_rtprog* p, uint32_t width, uint32_t height, uint32_t depth, void* hip_stream) {  // :330-332
  if (!p) RT_FAIL("The program handle is null!");
  if (!p->d_rays || !p->d_hits) RT_FAIL("The program is not bound to a ray batch.");
  const uint64_t n = (uint64_t)width * height * depth;
  if (n > 0xffffffffull) RT_FAIL("The launch is too large.");
  return hala_rt_trace_rays(p->renderer, p->d_rays, p->d_hits, (uint32_t)n, rtprog_mode(p), nullptr, hip_stream);
}
// RENDER_SPEC 4.7 on the bound batch (its hit buffer holds width * height * depth * k records); the constant block is not consulted
int hala_rtprog_trace_rays_multi(hala_rtprog* p, uint32_t width, uint32_t height, uint32_t depth, uint32_t k, uint32_t* d_counts, void* hip_stream) {
  if (!p) RT_FAIL("The program handle is null!");
  if (!p->d_rays || !p->d_hits) RT_FAIL("The program is not bound to a ray batch.");
  const uint64_t n = (uint64_t)width * height * depth;
  if (n > 0xffffffffull) RT_FAIL("The launch is too large.");
  return hala_rt_trace_rays_multi(p->renderer, p->d_rays, p->d_hits, d_counts, (uint32_t)n, k, hip_stream);
}
int hala_rtprog_trace_rays_indirect(hala_rtprog* p, const uint32_t* d_indirect, void* hip_stream) {  // :338-340
  if (!p) RT_FAIL("The program handle is null!");
  if (!p->d_rays || !p->d_hits) RT_FAIL("The program is not bound to a ray batch.");
  return hala_rt_trace_rays_indirect(p->renderer, p->d_rays, p->d_hits, d_indirect, rtprog_mode(p), hip_stream);
}

}  // extern "C"
