// rt_rays.hip — what works without a frame: the ray-batch operators on the committed scene's tree (single-hit and multi-hit), the
// hala_rtprog object over them, and the stand-alone helpers of the C ABI (environment distribution, tonemap, hash, image files).  The
// other query batches are in rt_queries.hip and rt_bake.hip; all of them run inside a BatchScope (renderer_state.h).
#include "renderer_state.h"

extern "C" {

// ---- ray-batch operator ------------------------------------------------------------------------------------------------
int hala_rt_trace_rays(hala_rt_renderer* r, const hala_ray* d_rays, hala_hit* d_hits, uint32_t count, int mode, uint64_t* d_counters, void* hip_stream) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (check_committed(r) != HALA_OK) return HALA_ERR;
  if (mode != 0 && mode != 1) RT_FAIL("Invalid trace mode.");
  if (count == 0) return HALA_OK;
  if (!d_rays || !d_hits) RT_FAIL("The ray batch is null!");
  BatchScope scope = r->batch(hip_stream);
  if (scope.open() != HALA_OK || scope.reset_work() != HALA_OK) return HALA_ERR;
  hipStream_t s = scope.s;
  // counters: the kernel accumulates into the control block's 64-bit fields; copy them out if requested
  if (d_counters) RT_HIP(hipMemsetAsync(&r->d_ctl.ptr->totals.steps[mode][0], 0, 16, s));
  // RENDER_SPEC 4.2: far origins are re-based where the batch enters, and the distance comes back on the closest hits where it leaves —
  // the traversal launch in between sees ordinary rays.  (Growing the copy frees the old one, which waits for whoever still reads it.)
  RT_HIP(r->d_batch_rays.grow(count));
  RT_HIP(r->d_batch_moved.grow(count));
  const SceneView sv = r->view();
  launch_rebase_batch(sv, d_rays, r->d_batch_rays.ptr, r->d_batch_moved.ptr, count, s);
  launch_trace_batch(r->lcfg, sv, r->d_batch_rays.ptr, d_hits, nullptr, count, r->d_batch_work.ptr, r->d_ctl.ptr, mode == 1, d_counters != nullptr, false, s);
  if (mode == 0) launch_unbase_hits(d_hits, r->d_batch_moved.ptr, count, s);
  if (d_counters) RT_HIP(hipMemcpyAsync(d_counters, &r->d_ctl.ptr->totals.steps[mode][0], 16, hipMemcpyDeviceToDevice, s));
  return scope.close();
}
// RENDER_SPEC 4.7: the same (scope, the renderer's own re-based copy of the batch) around the multi-hit kernel; the distance a far ray was
// moved comes back on every record of its list
static int multi_check(hala_rt_renderer* r, const void* rays, const void* hits, uint32_t count, uint32_t k) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (check_committed(r) != HALA_OK) return HALA_ERR;
  if (k == 0 || k > HALA_MAX_MULTI_HITS) RT_FAIL("The multi-hit capacity must be 1.." + std::to_string(HALA_MAX_MULTI_HITS) + ".");
  if (count == 0) return HALA_OK;
  if (!rays || !hits) RT_FAIL("The ray batch is null!");
  if ((uint64_t)count * k > (1ull << 32)) RT_FAIL("The multi-hit batch is too large.");
  return HALA_OK;
}
int hala_rt_trace_rays_multi(hala_rt_renderer* r, const hala_ray* d_rays, hala_hit* d_hits, uint32_t* d_counts, uint32_t count, uint32_t k, void* hip_stream) {
  if (multi_check(r, d_rays, d_hits, count, k) != HALA_OK) return HALA_ERR;
  if (count == 0) return HALA_OK;
  BatchScope scope = r->batch(hip_stream);
  if (scope.open() != HALA_OK || scope.reset_work() != HALA_OK) return HALA_ERR;
  RT_HIP(r->d_batch_rays.grow(count));
  RT_HIP(r->d_batch_moved.grow(count));
  const SceneView sv = r->view();
  launch_rebase_batch(sv, d_rays, r->d_batch_rays.ptr, r->d_batch_moved.ptr, count, scope.s);
  const bool fits = launch_trace_multi(r->lcfg, sv, r->cu_count, r->d_batch_rays.ptr, d_hits, d_counts, count, k, r->d_batch_work.ptr, scope.s);
  if (fits) launch_unbase_multi(d_hits, r->d_batch_moved.ptr, count, k, scope.s);
  return scope.close(fits ? nullptr : "The multi-hit traversal kernel does not fit on a compute unit.");
}
int hala_rt_trace_rays_multi_host(hala_rt_renderer* r, const hala_ray* rays, hala_hit* hits, uint32_t* counts, uint32_t count, uint32_t k) {
  if (multi_check(r, rays, hits, count, k) != HALA_OK) return HALA_ERR;
  if (count == 0) return HALA_OK;
  DeviceArray<hala_ray> d_rays;
  HostOut<hala_hit> d_hits(hits, (size_t)count * k);
  HostOut<uint32_t> d_counts(counts, count);
  RT_HIP(d_rays.upload(rays, count, r->stream));
  return host_form(r->stream, [&] { return hala_rt_trace_rays_multi(r, d_rays.ptr, d_hits.ptr(), d_counts.ptr(), count, k, r->stream); }, d_hits, d_counts);
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
  HostOut<hala_hit> d_hits(hits, count);
  HostOut<uint64_t> d_ctr(counters, 2);
  RT_HIP(d_rays.upload(rays, count, r->stream));
  return host_form(r->stream, [&] { return hala_rt_trace_rays(r, d_rays.ptr, d_hits.ptr(), count, mode, d_ctr.ptr(), r->stream); }, d_hits, d_ctr);
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
