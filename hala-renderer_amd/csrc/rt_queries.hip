// rt_queries.hip — the query batches that are not rays, on the committed scene's tree: closest points (RENDER_SPEC 4.8), distance grids
// (4.9) and occlusion (4.10).  Each device form runs inside a BatchScope (renderer_state.h: the renderer's scratch, stream order, no host
// synchronisation); each host form is host_form around its device form.  Where a batch needs a buffer the renderer owns, growing it
// frees the old one, which waits for whoever still reads it.
#include "renderer_state.h"

namespace {

int point_check(hala_rt_renderer* r, const void* queries, const void* out, uint32_t count) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (check_committed(r, "Closest-point queries") != HALA_OK) return HALA_ERR;
  if (count == 0) return HALA_OK;
  if (!queries || !out) RT_FAIL("The query batch is null!");
  return HALA_OK;
}
// RENDER_SPEC 4.9.  Which distance kernel an automatic grid runs (DESIGN.md 28 has the measurements the rule rests on).  The per-wave
// walk runs, in every lane, the union of what its 64 voxels need, and saves the wave its node and triangle fetches.  It wins where those
// fetches come from memory (not a staged tree), where the band does not end a query early (it spans the scene box) and where the voxels
// are fine against the scene: spacing * sqrt(triangles) <= 4.4 x the box's largest extent.  Everywhere else a voxel per lane.
uint32_t grid_auto_method(const SceneView& sv, const hala_distance_grid_desc* g) {
  if (sv.staged) return 1u;
  const float extent = std::max(sv.box_max[0] - sv.box_min[0], std::max(sv.box_max[1] - sv.box_min[1], sv.box_max[2] - sv.box_min[2]));
  if (!(g->band >= extent)) return 1u;
  return g->spacing * std::sqrt((float)sv.tri_count) <= 4.4f * extent ? 2u : 1u;
}
int grid_check(hala_rt_renderer* r, const hala_distance_grid_desc* g, const void* distance) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!g) RT_FAIL("The distance grid description is null!");
  if (!distance) RT_FAIL("The distance grid output is null!");
  if (check_committed(r, "Distance grids") != HALA_OK) return HALA_ERR;
  for (int a = 0; a < 3; ++a)
    if (g->dims[a] == 0 || g->dims[a] > 1024u) RT_FAIL("The distance grid's dims must be 1..1024 each.");
  if (!(std::isfinite(g->spacing) && g->spacing > 0.0f)) RT_FAIL("The distance grid's spacing must be finite and positive.");
  if (!(g->band >= 0.0f)) RT_FAIL("The distance grid's band must be >= 0 or +inf.");
  if ((g->flags & ~7u) != 0u || ((g->flags >> HALA_GRID_METHOD_SHIFT) & 3u) == 3u) RT_FAIL("Unknown distance grid flags.");
  return HALA_OK;
}
int occlusion_check(hala_rt_renderer* r, const void* samples, const void* out, uint32_t count, uint32_t rays) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (check_committed(r) != HALA_OK || check_occlusion_rays(rays) != HALA_OK) return HALA_ERR;
  if (count == 0) return HALA_OK;
  if (!samples || !out) RT_FAIL("The occlusion batch is null!");
  return check_occlusion_size(count, rays, "The occlusion batch is too large.");
}

}  // namespace

extern "C" {

// Nothing is re-based: the kernel reads the caller's queries.  d_counters (2 x uint64, or null): node visits and triangle tests of the batch.
int hala_rt_closest_points_counted(hala_rt_renderer* r, const hala_point_query* d_queries, hala_closest_point* d_out, uint32_t count,
                                   uint64_t* d_counters, void* hip_stream) {
  if (point_check(r, d_queries, d_out, count) != HALA_OK) return HALA_ERR;
  if (count == 0) return HALA_OK;
  BatchScope scope = r->batch(hip_stream);
  if (scope.open() != HALA_OK || scope.reset_work() != HALA_OK) return HALA_ERR;
  if (d_counters) RT_HIP(hipMemsetAsync(d_counters, 0, 16, scope.s));
  const bool fits = launch_closest_point(r->lcfg, r->view(), r->cu_count, d_queries, d_out, count, r->d_batch_work.ptr,
                                         reinterpret_cast<unsigned long long*>(d_counters), scope.s);
  return scope.close(fits ? nullptr : "The closest-point kernel does not fit on a compute unit.");
}
int hala_rt_closest_points(hala_rt_renderer* r, const hala_point_query* d_queries, hala_closest_point* d_out, uint32_t count, void* hip_stream) {
  return hala_rt_closest_points_counted(r, d_queries, d_out, count, nullptr, hip_stream);
}
int hala_rt_closest_points_host(hala_rt_renderer* r, const hala_point_query* queries, hala_closest_point* out, uint32_t count) {
  if (point_check(r, queries, out, count) != HALA_OK) return HALA_ERR;
  if (count == 0) return HALA_OK;
  DeviceArray<hala_point_query> d_queries;
  HostOut<hala_closest_point> d_out(out, count);
  RT_HIP(d_queries.upload(queries, count, r->stream));
  return host_form(r->stream, [&] { return hala_rt_closest_points(r, d_queries.ptr, d_out.ptr(), count, r->stream); }, d_out);
}

// The row pass of a signed grid, then the distance pass; the rows' bits live in a buffer the renderer owns.
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
  const size_t bit_words = (size_t)g.ny * g.nz * g.words;
  if (is_signed) RT_HIP(r->d_grid_bits.grow(bit_words));
  BatchScope scope = r->batch(hip_stream);
  if (scope.open() != HALA_OK) return HALA_ERR;
  hipStream_t s = scope.s;
  unsigned long long* counters = reinterpret_cast<unsigned long long*>(d_counters);
  if (d_counters) RT_HIP(hipMemsetAsync(d_counters, 0, 48, s));
  bool fits = true;
  if (is_signed) {
    if (scope.reset_work() != HALA_OK) return HALA_ERR;
    RT_HIP(hipMemsetAsync(r->d_grid_bits.ptr, 0, bit_words * 4, s));
    fits = launch_grid_rows(r->lcfg, sv, r->cu_count, g, r->d_grid_bits.ptr, r->d_batch_work.ptr, counters, s);
  }
  if (fits) {
    if (scope.reset_work() != HALA_OK) return HALA_ERR;
    fits = launch_distance_grid(r->lcfg, sv, r->cu_count, g, method, d_distance, d_prim, is_signed ? r->d_grid_bits.ptr : nullptr, r->d_batch_work.ptr, counters, s);
  }
  return scope.close(fits ? nullptr : "The distance grid kernels do not fit on a compute unit.");
}
int hala_rt_distance_grid(hala_rt_renderer* r, const hala_distance_grid_desc* desc, float* d_distance, uint32_t* d_prim, void* hip_stream) {
  return hala_rt_distance_grid_counted(r, desc, d_distance, d_prim, nullptr, hip_stream);
}
int hala_rt_distance_grid_host(hala_rt_renderer* r, const hala_distance_grid_desc* desc, float* distance, uint32_t* prim) {
  if (grid_check(r, desc, distance) != HALA_OK) return HALA_ERR;
  const size_t n = (size_t)desc->dims[0] * desc->dims[1] * desc->dims[2];
  HostOut<float> d_distance(distance, n);
  HostOut<uint32_t> d_prim(prim, n);
  return host_form(r->stream, [&] { return hala_rt_distance_grid(r, desc, d_distance.ptr(), d_prim.ptr(), r->stream); }, d_distance, d_prim);
}

// Nothing is copied or re-based ahead of the launch: the rays are made, far origins included, in the lanes that trace them.  Without the
// caller's mask array the words live in a buffer the renderer owns.
int hala_rt_occlusion(hala_rt_renderer* r, const hala_occlusion_sample* d_samples, hala_occlusion* d_out, uint32_t* d_masks, uint32_t count, uint32_t rays,
                      uint32_t seed, void* hip_stream) {
  if (occlusion_check(r, d_samples, d_out, count, rays) != HALA_OK) return HALA_ERR;
  if (count == 0) return HALA_OK;
  const size_t mask_words = (size_t)count * ((rays + 31u) / 32u);
  if (!d_masks) {
    RT_HIP(r->d_occlusion_masks.grow(mask_words));
    d_masks = r->d_occlusion_masks.ptr;
  }
  BatchScope scope = r->batch(hip_stream);
  if (scope.open() != HALA_OK || scope.reset_work() != HALA_OK) return HALA_ERR;
  RT_HIP(hipMemsetAsync(d_masks, 0, mask_words * 4, scope.s));
  launch_trace_occlusion(r->lcfg, r->view(), d_samples, d_out, d_masks, count, rays, seed, r->d_batch_work.ptr, scope.s);
  return scope.close();
}
int hala_rt_occlusion_host(hala_rt_renderer* r, const hala_occlusion_sample* samples, hala_occlusion* out, uint32_t* masks, uint32_t count, uint32_t rays,
                           uint32_t seed) {
  if (occlusion_check(r, samples, out, count, rays) != HALA_OK) return HALA_ERR;
  if (count == 0) return HALA_OK;
  DeviceArray<hala_occlusion_sample> d_samples;
  HostOut<hala_occlusion> d_out(out, count);
  HostOut<uint32_t> d_masks(masks, (size_t)count * ((rays + 31u) / 32u));
  RT_HIP(d_samples.upload(samples, count, r->stream));
  return host_form(r->stream, [&] { return hala_rt_occlusion(r, d_samples.ptr, d_out.ptr(), d_masks.ptr(), count, rays, seed, r->stream); }, d_out, d_masks);
}

}  // extern "C"
