// renderer.hip — HalaRenderer (src/rt_renderer.rs:568-1353) re-designed for one MI355X: the C++ object behind the
// C ABI of include/halart.h.  Descriptor sets become a struct of device pointers (rt::SceneView), trace_rays becomes the
// wavefront kernel sequence of trace_closest.hip, timestamp queries become HIP events, staging buffers become
// hipMemcpyAsync from the caller's memory.  Everything that computes runs on the GPU; the host units only orchestrate.
// This unit: create / destroy, settings, scene, envmap and commit, the update itself, render and the read-backs of the frame,
// statistics.  The object and the other host units: renderer_state.h.
#include "renderer_state.h"

namespace rt {

int ensure_device(hala_rt_renderer* r, bool join) {
  if (!r) RT_FAIL("The renderer handle is null!");
  RT_HIP(hipSetDevice(r->device));
  if (join && r->slots.join(r->stream) != HALA_OK) return HALA_ERR;
  return HALA_OK;
}

// slot 1's set, all or nothing: without it the renderer works with one slot until the sets are sized again
static bool fit_second(FrameSlots& fs, const PathShape& want) {
  fs.second_failed = fs.slot[1].set.fit(want) != hipSuccess;
  if (fs.second_failed) { (void)hipGetLastError(); fs.slot[1].set.release(); }
  return !fs.second_failed;
}

// wavefront state for `capacity` paths per pixel slot in flight (samples x views, hala_rt_update_batch)
static int alloc_wavefront(hala_rt_renderer* r, uint32_t capacity) {
  FrameSlots& fs = r->slots;
  const PathShape want = r->path_shape(capacity);
  if (want.paths > 0xfffffff0ull) RT_FAIL("The sample batch is too large for 32-bit path slots.");
  if (want.groups && want.paths > kGroupSlotMask) RT_FAIL("Light groups need fewer than 2^29 path slots (pixels x samples x views).");
  RT_HIP(fs.slot[0].set.fit(want));
  r->batch_capacity = capacity;
  fs.second_failed = false;
  if (fs.slot[1].set.shape.paths) (void)fit_second(fs, want);  // the second frame slot follows (callers have joined it and waited)
  return HALA_OK;
}

// The slot of an overlapped update: the other one than the latest update's — slot 1 only once its set exists, which is allocated the
// first time slot 0 is found busy (and again after a feature changed what a path slot holds).  Never fails: without it slot 0, serial.
static int pick_slot(hala_rt_renderer* r) {
  FrameSlots& fs = r->slots;
  if (fs.last == 1) return 0;
  if (r->staged) return 1;  // slot 1's stream and control block, slot 0's set (begin_update)
  const PathShape want = r->path_shape(), &second = fs.slot[1].set.shape;
  if (second == want) return 1;
  if (fs.second_failed) return 0;
  if (second.paths == 0) {  // not yet: only when it would help
    const bool busy = fs.slot[0].end && hipEventQuery(fs.slot[0].end) == hipErrorNotReady;
    (void)hipGetLastError();
    if (!busy) return 0;
  } else if (fs.join(r->stream) != HALA_OK || hipStreamSynchronize(r->stream) != hipSuccess) return 0;  // stale: fitted to other features (their setters joined and waited)
  return fit_second(fs, want) ? 1 : 0;
}

int alloc_frame_buffers(hala_rt_renderer* r) {
  const size_t n = r->image_alloc();
  for (int k = 0; k < 6; ++k) {
    DeviceArray<float4>& i = r->img_local[k];
    if (!r->has_image(k)) { i.release(); continue; }
    RT_HIP(i.resize(n)); RT_HIP(hipMemsetAsync(i.ptr, 0, n * sizeof(float4), r->stream));
  }
  if (r->groups.count) { RT_HIP(r->groups.img.resize(n * r->groups.count)); RT_HIP(hipMemsetAsync(r->groups.img.ptr, 0, r->groups.img.bytes(), r->stream)); }
  r->groups.relit_valid = false;
  if (alloc_wavefront(r, 1) != HALA_OK) return HALA_ERR;
  RT_HIP(r->d_ctl.resize(2));  // one per frame slot
  RT_HIP(hipMemsetAsync(r->d_ctl.ptr, 0, 2 * sizeof(Control), r->stream));
  RT_HIP(r->d_batch_work.resize(1));
  return HALA_OK;
}

// resolve one ring slot's events into the totals (the slot's work must have completed)
static void resolve_slot(hala_rt_renderer* r, TraceEvents& t) {
  if (!t.pending) return;
  (void)hipEventSynchronize(t.frame_end);
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, t.frame_begin, t.frame_end) == hipSuccess) { r->stats.last_gpu_ms = ms; r->stats.gpu_ms_total += ms; }
  // four events per depth: a | closest-hit launch | b | shade launch | c | shadow launch(es) or the fused launch | d
  double tr[3] = {0.0, 0.0, 0.0}, sh = 0.0;  // closest-hit launches, shadow launches, fused launches
  unsigned long long rays[3] = {0, 0, 0}, launches[3] = {0, 0, 0};
  const QueueSizes* qs = t.host_sizes;
  for (size_t k = 0, depth = 0; k + 3 < t.used; k += 4, ++depth) {
    float m = 0.0f;
    const bool own_closest = depth == 0 || !((t.traced_mask >> depth) & 1ull);  // else: it ran inside the previous depth's fused launch
    if (own_closest && hipEventElapsedTime(&m, t.ev[k], t.ev[k + 1]) == hipSuccess) {
      const unsigned long long n = depth == 0 ? (unsigned long long)t.primary_pixels * t.samples : qs->n_active[depth];
      tr[0] += m; rays[0] += n; launches[0] += 1;
      if (depth == 0) { r->stats.traverse_primary_ms_total += m; r->stats.traverse_primary_launches += 1; r->stats.rays_primary_timed += n; }  // k_trace_primary
    }
    if (hipEventElapsedTime(&m, t.ev[k + 1], t.ev[k + 2]) == hipSuccess) sh += m;
    if (hipEventElapsedTime(&m, t.ev[k + 2], t.ev[k + 3]) == hipSuccess) {
      const unsigned long long ns = (unsigned long long)qs->n_shadow[0][depth] + qs->n_shadow[1][depth];
      if ((t.fused_mask >> depth) & 1ull) {
        tr[2] += m; launches[2] += 1;
        r->stats.rays_fused_shadow_timed += ns;
        if ((t.traced_mask >> (depth + 1)) & 1ull) r->stats.rays_fused_closest_timed += qs->n_active[depth + 1];
      } else { tr[1] += m; rays[1] += ns; }
    }
  }
  r->stats.traverse_ms_last_update = tr[0] + tr[1] + tr[2];
  r->stats.traverse_closest_ms_total += tr[0];
  r->stats.traverse_shadow_ms_total += tr[1];
  r->stats.traverse_fused_ms_total += tr[2];
  r->stats.shade_ms_total += sh;
  r->stats.traverse_closest_launches += launches[0];
  r->stats.traverse_fused_launches += launches[2];
  r->stats.shade_launches += t.used / 4;
  r->stats.traverse_shadow_launches += t.used ? t.shadow_launches : 0;  // as issued: one per connection kind the scene has, per depth
  r->stats.rays_closest_timed += rays[0]; r->stats.rays_shadow_timed += rays[1];
  r->stats.updates_rendered += t.samples;
  const Totals& tot = *t.host_totals;
  const unsigned long long rc = tot.rays_closest, rs = tot.rays_shadow;
  r->stats.rays_last_update = rc + rs;
  r->stats.rays_total += rc + rs;
  r->stats.rays_closest_total += rc;
  r->stats.rays_primary_total += (unsigned long long)t.primary_pixels * t.samples;
  r->stats.rays_shadow_total += rs;
  if (t.counted) {
    r->stats.nodes_closest_total += tot.steps[0][0]; r->stats.tris_closest_total += tot.steps[0][1];
    r->stats.nodes_shadow_total += tot.steps[1][0]; r->stats.tris_shadow_total += tot.steps[1][1];
    r->stats.rays_closest_counted += rc; r->stats.rays_shadow_counted += rs;
    r->stats.wave_steps_closest_total += tot.probe[0][0]; r->stats.leaf_passes_closest_total += tot.probe[0][1]; r->stats.leaf_lanes_closest_total += tot.probe[0][2];
    r->stats.nodes_primary_total += tot.primary_steps[0]; r->stats.tris_primary_total += tot.primary_steps[1];
    r->stats.rays_primary_counted += (unsigned long long)t.primary_pixels * t.samples;
    r->stats.wave_steps_shadow_total += tot.probe[1][0]; r->stats.leaf_passes_shadow_total += tot.probe[1][1]; r->stats.leaf_lanes_shadow_total += tot.probe[1][2];
  }
  t.pending = false;
}
static hipEvent_t next_event(TraceEvents& t) {
  if (t.used == t.ev.size()) { hipEvent_t e = nullptr; (void)hipEventCreate(&e); t.ev.push_back(e); }
  return t.ev[t.used++];
}

std::string file_stem(const char* path) {
  std::string p(path);
  const size_t slash = p.find_last_of("/\\");
  std::string base = slash == std::string::npos ? p : p.substr(slash + 1);
  const size_t dot = base.find_last_of('.');
  if (dot != std::string::npos && dot != 0) base = base.substr(0, dot);
  return base;
}

static int install_envmap(hala_rt_renderer* r, const float* pixels, uint32_t channels, uint32_t w, uint32_t h, float rotation,
                   const float* cached_total, const float* cached_marginal, const float* cached_conditional) {
  if (!pixels || w == 0 || h == 0 || (channels != 3 && channels != 4)) RT_FAIL("Unsupported color type for environment map.");  // src/envmap.rs:57-60
  std::vector<float> data((size_t)w * h * 4);
  for (size_t i = 0; i < (size_t)w * h; ++i) {  // src/envmap.rs:63-89
    for (uint32_t c = 0; c < 3; ++c) {
      const float v = pixels[i * channels + c];
      if (std::isnan(v)) RT_FAIL("The pixel value is NaN!");
      if (std::isinf(v)) RT_FAIL("The pixel value is infinite!");
      data[4 * i + c] = v;
    }
    data[4 * i + 3] = 1.0f;  // :87
  }
  RT_HIP(r->d_env.upload(reinterpret_cast<const float4*>(data.data()), (size_t)w * h, r->stream));
  RT_HIP(r->d_env_total.resize(1)); RT_HIP(r->d_marginal.resize(h)); RT_HIP(r->d_conditional.resize((size_t)w * h));
  if (cached_total) {  // ./out/<stem>.dist_cache hit (src/envmap.rs:91-117)
    RT_HIP(hipMemcpyAsync(r->d_env_total.ptr, cached_total, 4, hipMemcpyHostToDevice, r->stream));
    RT_HIP(hipMemcpyAsync(r->d_marginal.ptr, cached_marginal, (size_t)h * 4, hipMemcpyHostToDevice, r->stream));
    RT_HIP(hipMemcpyAsync(r->d_conditional.ptr, cached_conditional, (size_t)w * h * 4, hipMemcpyHostToDevice, r->stream));
    RT_HIP(hipStreamSynchronize(r->stream));
    r->env_total_sum = *cached_total;
  } else {
    const std::string e = envmap_build_distribution(r->d_env.ptr, w, h, r->d_env_total.ptr, r->d_marginal.ptr, r->d_conditional.ptr, r->stream);
    if (!e.empty()) RT_FAIL(e);
    RT_HIP(hipMemcpy(&r->env_total_sum, r->d_env_total.ptr, 4, hipMemcpyDeviceToHost));
  }
  r->env_w = w; r->env_h = h; r->has_env = true; r->env_rotation = rotation;  // src/rt_renderer.rs:1192
  return HALA_OK;
}

}  // namespace rt

// =================================================================================================================
// C ABI
// =================================================================================================================
extern "C" {

const char* hala_last_error_message(void) { return get_last_error(); }
const char* hala_version(void) { return "halart 0.1 (gfx950)"; }

int hala_rt_create(const char* name, uint32_t width, uint32_t height, int device_ordinal, uint32_t max_depth, uint32_t rr_depth,
                   int enable_tonemap, int enable_aces, int use_simple_aces, uint64_t max_frames, hala_rt_renderer** out) {
  if (!out) RT_FAIL("The output handle is null!");
  *out = nullptr;
  if (width == 0 || height == 0) RT_FAIL("The renderer resolution is zero!");
  if (max_depth == 0 || max_depth > kMaxDepth) RT_FAIL("max_depth must be in 1.." + std::to_string(kMaxDepth) + ".");
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) RT_FAIL("No HIP device is available: libhalart has no CPU path.");
  if (device_ordinal < 0 || device_ordinal >= count) RT_FAIL("The requested device ordinal does not exist.");
  RT_HIP(hipSetDevice(device_ordinal));
  std::unique_ptr<hala_rt_renderer> r(new hala_rt_renderer());
  r->name = name ? name : "";
  r->width = width; r->height = height; r->device = device_ordinal;
  r->max_depth = max_depth; r->rr_depth = rr_depth;
  r->enable_tonemap = enable_tonemap != 0; r->enable_aces = enable_aces != 0; r->use_simple_aces = use_simple_aces != 0;
  r->max_frames = max_frames == 0 ? UINT64_MAX : max_frames;  // src/rt_renderer.rs:774
  hipDeviceProp_t prop;
  RT_HIP(hipGetDeviceProperties(&prop, device_ordinal));
  r->cu_count = (uint32_t)prop.multiProcessorCount;
  RT_HIP(hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking));
  FrameSlots& fs = r->slots;
  fs.slot[0].stream = r->stream;
  RT_HIP(hipStreamCreateWithFlags(&fs.slot[1].stream, hipStreamNonBlocking));
  for (hipEvent_t* e : {&fs.slot[0].folded, &fs.slot[1].folded, &fs.slot[0].lead, &fs.slot[1].lead, &fs.forked}) RT_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
  compute_tiling(r.get());
  // create_storage_images (src/rt_renderer.rs:818-917): final, accum, albedo, normal
  if (alloc_frame_buffers(r.get()) != HALA_OK) return HALA_ERR;
  RT_HIP(hipStreamSynchronize(r->stream));
  *out = r.release();
  return HALA_OK;
}

void hala_rt_destroy(hala_rt_renderer* r) { delete r; }

int hala_rt_push_general_shader(hala_rt_renderer* r, const void* code, size_t code_size, int stage, const char*) {
  if (!r) RT_FAIL("The renderer handle is null!");
  if (!code || code_size == 0) RT_FAIL("The shader code is empty!");
  if (stage == 0) r->n_raygen++; else if (stage == 1) r->n_miss++; else if (stage == 2) r->n_callable++; else RT_FAIL("Invalid general shader stage.");
  return HALA_OK;
}
int hala_rt_push_general_shader_with_file(hala_rt_renderer* r, const char* file_path, int stage, const char* debug_name) {
  if (!r) RT_FAIL("The renderer handle is null!");
  struct stat st;
  if (!file_path || stat(file_path, &st) != 0) RT_FAIL(std::string("Failed to load shader file \"") + (file_path ? file_path : "") + "\".");
  static const char dummy = 0;
  return hala_rt_push_general_shader(r, &dummy, 1, stage, debug_name);
}
int hala_rt_push_hit_shaders(hala_rt_renderer* r, const void* ch, size_t chs, const void* ah, size_t ahs, const void* is, size_t iss, const char*) {
  if (!r) RT_FAIL("The renderer handle is null!");
  if ((!ch || !chs) && (!ah || !ahs) && (!is || !iss)) RT_FAIL("The hit shader group is empty!");
  r->n_hit++;
  return HALA_OK;
}
int hala_rt_push_hit_shaders_with_file(hala_rt_renderer* r, const char* ch, const char* ah, const char* is, const char*) {
  if (!r) RT_FAIL("The renderer handle is null!");
  struct stat st;
  for (const char* p : {ch, ah, is}) if (p && stat(p, &st) != 0) RT_FAIL(std::string("Failed to load shader file \"") + p + "\".");
  if (!ch && !ah && !is) RT_FAIL("The hit shader group is empty!");
  r->n_hit++;
  return HALA_OK;
}

int hala_rt_load_blue_noise_pixels(hala_rt_renderer* r, const uint8_t* rgba8, uint32_t width, uint32_t height);
int hala_rt_load_blue_noise_texture(hala_rt_renderer* r, const char* path) {
  if (!r) RT_FAIL("The renderer handle is null!");
  if (!path || !*path || file_stem(path).empty()) RT_FAIL("The file name is none!");  // src/rt_renderer.rs:1120
  uint32_t w = 0, h = 0;
  std::vector<uint8_t> px;
  std::string e;
  try { e = rt::decode_image_file_rgba8(path, &w, &h, &px); }
  catch (const std::exception& ex) { e = std::string("Failed to open image \"") + path + "\": " + ex.what(); }  // nothing is thrown across the C ABI
  if (!e.empty()) RT_FAIL(e);
  return hala_rt_load_blue_noise_pixels(r, px.data(), w, h);
}
int hala_rt_load_blue_noise_pixels(hala_rt_renderer* r, const uint8_t* rgba8, uint32_t width, uint32_t height) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!rgba8 || !width || !height) RT_FAIL("The blue noise texture is empty!");
  RT_HIP(r->blue_noise.upload(rgba8, (size_t)width * height * 4, r->stream));
  RT_HIP(hipStreamSynchronize(r->stream));
  r->blue_w = width; r->blue_h = height;
  return HALA_OK;
}

int hala_rt_set_scene(hala_rt_renderer* r, const hala_scene_desc* scene) {
  RtRange range("halart::set_scene");
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  RT_HIP(hipStreamSynchronize(r->stream));
  r->has_scene = false; r->committed = false;  // "Release the old scene in the GPU." (src/rt_renderer.rs:1164)
  r->temporal.drop_history();  // RENDER_SPEC §16: the history belongs to the old scene
  r->deform.off();             // RENDER_SPEC §17: so do the deformers
  r->shutter.off();            // RENDER_SPEC §18: and every key, and the shutter
  r->rig.off();                // RENDER_SPEC §19: and the rig that registered deformers
  r->nodes.release();          // RENDER_SPEC §20: and the bound node set (the host mirror is replaced whole below)
  r->nodes_dirty = false; r->materials_dirty = false;
  const std::string e = r->hs.assign(scene);
  if (!e.empty()) RT_FAIL(e);
  if (upload_packed(r) != HALA_OK) return HALA_ERR;
  if (upload_textures(r) != HALA_OK) return HALA_ERR;
  r->has_scene = true;
  return HALA_OK;
}

int hala_rt_set_envmap_pixels(hala_rt_renderer* r, const float* pixels, uint32_t channels, uint32_t width, uint32_t height, float rotation_degrees) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  RT_HIP(hipStreamSynchronize(r->stream));
  return install_envmap(r, pixels, channels, width, height, rotation_degrees, nullptr, nullptr, nullptr);
}

int hala_rt_set_envmap_file(hala_rt_renderer* r, const char* path, float rotation_degrees) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!path || !*path) RT_FAIL("The file name is none!");  // src/envmap.rs:45
  HostImage img;
  const std::string e = load_float_image(path, &img);
  if (!e.empty()) RT_FAIL(e);
  RT_HIP(hipStreamSynchronize(r->stream));
  // ./out/<stem>.dist_cache: [f32 total_sum][f32 x H][f32 x W*H], native endian, no header (src/envmap.rs:90-142)
  const std::string cache = "./out/" + file_stem(path) + ".dist_cache";
  const size_t W = img.width, H = img.height;
  std::vector<float> blob(1 + H + W * H);
  FILE* f = fopen(cache.c_str(), "rb");
  if (f) {
    const size_t got = fread(blob.data(), 4, blob.size(), f);
    fclose(f);
    if (got != blob.size()) RT_FAIL("Failed to read from file.");  // :101, :107, :114
    return install_envmap(r, img.pixels.data(), img.channels, img.width, img.height, rotation_degrees, &blob[0], &blob[1], &blob[1 + H]);
  }
  if (install_envmap(r, img.pixels.data(), img.channels, img.width, img.height, rotation_degrees, nullptr, nullptr, nullptr) != HALA_OK) return HALA_ERR;
  blob[0] = r->env_total_sum;
  RT_HIP(hipMemcpy(&blob[1], r->d_marginal.ptr, H * 4, hipMemcpyDeviceToHost));
  RT_HIP(hipMemcpy(&blob[1 + H], r->d_conditional.ptr, W * H * 4, hipMemcpyDeviceToHost));
  f = fopen(cache.c_str(), "wb");
  if (!f) RT_FAIL("Failed to create file \"" + cache + "\".");  // :125 (the reference does not create ./out either)
  const size_t put = fwrite(blob.data(), 4, blob.size(), f);
  if (fclose(f) != 0 || put != blob.size()) RT_FAIL("Failed to write to file.");
  return HALA_OK;
}

void hala_rt_set_ground_color(hala_rt_renderer* r, const float rgba[4]) { if (r && rgba) memcpy(r->ground, rgba, 16); }
void hala_rt_set_sky_color(hala_rt_renderer* r, const float rgba[4]) { if (r && rgba) memcpy(r->sky, rgba, 16); }
void hala_rt_set_env_intensity(hala_rt_renderer* r, float v) { if (r) r->env_intensity = v; }
void hala_rt_set_exposure_value(hala_rt_renderer* r, float v) { if (r) r->exposure = v; }

int hala_rt_commit(hala_rt_renderer* r) {
  RtRange range("halart::commit");
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!r->has_scene) RT_FAIL("The scene in GPU is none!");  // src/rt_renderer.rs:138
  if (r->hs.cameras.empty()) RT_FAIL("The scene has no camera.");
  if (r->hs.instances.empty()) RT_FAIL("The scene has no mesh primitive.");  // `primitives[0]` panics in the reference (gpu_uploader.rs:888)
  RT_HIP(hipStreamSynchronize(r->stream));  // (a recommit: earlier frames may still read the bundles)
  if (update_texture_bundles(r, true) != HALA_OK) return HALA_ERR;
  r->sync_host_mirror();
  r->nodes.release();  // RENDER_SPEC §20: a commit drops the binding
  if (build_bvh(r) != HALA_OK) return HALA_ERR;
  r->committed = true;
  r->invalidate(Changed::Commit);
  r->reset_accumulation();
  return HALA_OK;
}

// ---- update: `frames` consecutive update()s in one wavefront pass, in four steps (update_impl) ---------------------------------------------
// what prepare_update decided; samples == 0: the frames count, nothing is launched
struct UpdatePlan {
  uint64_t first = 0;           // frame_index of the first frame of the batch
  uint32_t samples = 0;         // frames that render
  uint32_t primary_pixels = 0;  // camera rays per frame, all views
  bool timed = false;           // the update carries per-launch timing events
  FrameConst fc{}; SceneView sv{};  // (fc.u: the uniform)
  bool far_camera = false;      // RENDER_SPEC 4.2: a camera ray of some view may start beyond the scene's far limit
};
// RENDER_SPEC 4.2: can a ray of this camera (§5: the position, moved over the lens or the orthographic window) start beyond `far_limit`?
// A bound, not the test: the camera-ray kernel built for far cameras tests every ray itself; the ordinary one tests none.
static bool camera_may_be_far(const hala_gpu_camera& c, float far_limit) {
  const float m = std::max({std::fabs(c.position[0]), std::fabs(c.position[1]), std::fabs(c.position[2])});
  const float len = std::max(std::sqrt(c.right[0] * c.right[0] + c.right[1] * c.right[1] + c.right[2] * c.right[2]),
                             std::sqrt(c.up[0] * c.up[0] + c.up[1] * c.up[1] + c.up[2] * c.up[2]));
  const float window = std::fabs(c.aperture_or_ymag) + (c.type == 0u ? 0.0f : std::fabs(c.focal_distance_or_xmag));
  return !((m + 2.0f * window * len) * 1.001f <= far_limit);  // (a NaN anywhere: far)
}
// where begin_update put the update: its entry of the statistics ring, its frame slot and what a launch on that slot takes
struct SlotRun {
  TraceEvents* te; int slot; hipStream_t stream; Control* ctl; Queues q; PathState ps; LaunchCfg lc;
  hipEvent_t lead;        // the slot's, to record
  hipEvent_t before_end;  // LDS-staged trees: the end of the update before this one, which the depth-0 shade waits for (else null)
};

// Step 1, host side: validation, the shutter's step, the frame counter, capacity, tables, the uniform.  Bookkeeping per frame as in the
// reference: total_frames is incremented first (pre_update, src/renderer.rs:278) and a frame whose number exceeds max_frames is skipped
// (src/rt_renderer.rs:394-396); the frames that do render share one kernel sequence with `samples` paths per pixel.
static int prepare_update(hala_rt_renderer* r, uint32_t frames, UpdatePlan* p) {
  if (!r->committed) RT_FAIL("The pipeline is none!");  // src/rt_renderer.rs:443
  const uint32_t V = r->view_count();
  for (uint32_t v = 0; v < V; ++v)  // RENDER_SPEC §12: a scene set or committed after hala_rt_set_views may have fewer cameras
    if (r->views[v] >= r->hs.cameras.size())
      RT_FAIL("hala_rt_update: view " + std::to_string(v) + " renders camera " + std::to_string(r->views[v]) + ", but the committed scene has " +
              std::to_string(r->hs.cameras.size()) + " camera(s) (hala_rt_set_views).");
  if (r->groups.count && (r->hs.lights.size() > r->groups.light_group.size() || r->hs.gpu_materials.size() > r->groups.material_group.size()))  // RENDER_SPEC §14
    RT_FAIL("hala_rt_update: the light groups cover " + std::to_string(r->groups.light_group.size()) + " light(s) and " + std::to_string(r->groups.material_group.size()) +
            " material(s), but the committed scene has " + std::to_string(r->hs.lights.size()) + " and " + std::to_string(r->hs.gpu_materials.size()) +
            " (hala_rt_set_light_groups).");
  const uint64_t first = r->total_frames;  // frame_index of the first frame of this batch = total_frames - 1 after its increment
  // RENDER_SPEC §18: a frame of another step than the one the scene stands at moves the scene first (hala_rt_update_batch ends its chunks
  // on stride boundaries: every frame of this batch belongs to one step).  The frame counter advances only behind a successful step.
  if (r->shutter.act.active() && first < r->max_frames) {
    const uint32_t step = (uint32_t)first / r->shutter.act.stride;
    if (step != r->shutter.step && shutter_step(r, step) != HALA_OK) return HALA_ERR;
  }
  r->total_frames += frames;
  if (first >= r->max_frames) return HALA_OK;
  const uint32_t samples = (uint32_t)std::min<uint64_t>(frames, r->max_frames - first);
  if (samples * V > r->batch_capacity) {
    if (r->slots.join(r->stream) != HALA_OK) return HALA_ERR;
    RT_HIP(hipStreamSynchronize(r->stream));
    if (alloc_wavefront(r, samples * V) != HALA_OK) return HALA_ERR;
  }
  if (r->crypto.mask && crypto_prepare(r) != HALA_OK) return HALA_ERR;  // RENDER_SPEC §15: id tables and records for this scene and views
  if (V > 1u) {  // the view table: tan_half / pixel_spread follow the cameras' yfov, which a new scene may change
    std::vector<ViewConst> table(V);
    for (uint32_t v = 0; v < V; ++v) table[v] = r->view_const(r->views[v], (float)r->height);
    if (table.size() != r->views_uploaded.size() || memcmp(table.data(), r->views_uploaded.data(), V * sizeof(ViewConst)) != 0) {
      if (r->slots.join(r->stream) != HALA_OK) return HALA_ERR;
      RT_HIP(hipStreamSynchronize(r->stream));  // no update in flight reads the old table
      RT_HIP(r->d_views.upload(table.data(), V, r->stream));
      RT_HIP(hipStreamSynchronize(r->stream));
      r->views_uploaded = table;
    }
  }
  hala_global_uniform u{};                                 // :408-427
  memcpy(u.ground_color, r->ground, 16); memcpy(u.sky_color, r->sky, 16);
  u.resolution[0] = (float)r->width; u.resolution[1] = (float)r->height;
  u.max_depth = r->max_depth; u.rr_depth = r->rr_depth;
  u.frame_index = (uint32_t)first;  // == total_frames - 1 for a single-frame update (:414)
  u.camera_index = r->views[0];  // RENDER_SPEC §12: view 0's camera (0 unless hala_rt_set_views chose another)
  u.env_type = r->has_env ? 1u : 0u;
  u.env_map_width = r->has_env ? r->env_w : 0; u.env_map_height = r->has_env ? r->env_h : 0;
  u.env_total_sum = r->has_env ? r->env_total_sum : 0.0f;
  u.env_rotation = r->env_rotation / 360.0f;
  u.env_intensity = r->env_intensity;
  r->output_settings(&u);
  u.num_of_lights = (uint32_t)r->hs.lights.size();
  r->last_uniform = u;
  r->last_uniform.frame_index = (uint32_t)(first + samples - 1);  // what the last frame of the batch would have uploaded
  AdaptiveState& ad = r->adaptive;
  if (ad.enabled && first == 0 && (r->slots.join(r->stream) != HALA_OK || adaptive_begin(ad, r->stream) != hipSuccess)) RT_FAIL("hala_rt_update: the adaptive sampling state could not be reset.");
  if (ad.enabled && ad.active_blocks == 0) {  // RENDER_SPEC 11: every block has converged; the frames count, nothing is launched
    for (int k = 0; k < kStatRing; ++k) resolve_slot(r, r->ring[(r->ring_pos + k) % kStatRing]);  // done: the last check waited for them
    r->stats.rays_last_update = 0;
    return HALA_OK;
  }
  p->first = first; p->samples = samples;
  p->primary_pixels = (ad.enabled ? ad.active_pixels : r->real_pixels) * V;
  p->fc = r->frame_const(u, samples);
  p->sv = r->view();
  for (uint32_t v = 0; v < V; ++v) p->far_camera = p->far_camera || camera_may_be_far(r->hs.cameras[r->views[v]], p->sv.far_limit);
  // per-launch HIP events (statistics: traverse_*_ms_total) on every launch_event_period-th update; each record is a barrier
  // packet on the stream, i.e. a few microseconds between two launches
  p->timed = r->launch_event_period == 1u || (r->launch_event_period > 1u && (r->update_counter % r->launch_event_period) == 0u);
  r->update_counter++;
  return HALA_OK;
}

// Step 2: the update's frame slot, and its stream put behind everything the update has to follow.  Untimed updates alternate between the
// two frame slots (FrameSlots), each wholly on its slot's stream.  Updates that carry per-launch timing events or counting kernels join
// both slots and run alone, so that every measured launch has the chip to itself.
static int begin_update(hala_rt_renderer* r, const UpdatePlan& p, SlotRun* run) {
  TraceEvents& te = r->ring[r->ring_pos];  // the update's entry of the statistics ring: what it held before is folded into the totals first
  r->ring_pos = (r->ring_pos + 1) % kStatRing;
  resolve_slot(r, te);
  if (!te.frame_begin) { RT_HIP(hipEventCreate(&te.frame_begin)); RT_HIP(hipEventCreate(&te.frame_end)); RT_HIP(hipHostMalloc(reinterpret_cast<void**>(&te.host_totals), sizeof(Totals), hipHostMallocDefault)); }
  te.used = 0; te.counted = r->counting; te.shadow_launches = 0; te.fused_mask = 0; te.traced_mask = 0;
  te.samples = p.samples; te.primary_pixels = p.primary_pixels;
  FrameSlots& fs = r->slots;
  const bool overlapped = fs.in_flight == 2u && !p.timed && !r->counting;
  if (!overlapped && fs.join(r->stream) != HALA_OK) return HALA_ERR;
  const int slot = overlapped ? pick_slot(r) : 0;
  // LDS-staged trees (small scenes): two workgroups of their traversal kernels fill a CU's LDS, so the traversal launches of two updates
  // cannot share the chip, and a second set of buffers only halves what the caches keep from frame to frame (profiles/frames_in_flight.txt).
  // Their updates alternate between the streams and control blocks but share slot 0's set: the camera-ray launch, which touches
  // none of what the end of the update before it reads or writes, starts behind that update's last shade, the depth-0 shade behind its end
  const bool shared = overlapped && r->staged;
  const hipStream_t s = fs.slot[slot].stream;
  const int set = shared ? 0 : slot;
  *run = SlotRun{&te, slot, s, r->d_ctl.ptr + slot, r->queues(set), r->path_state(set), r->launch_cfg(slot), fs.slot[slot].lead,
                 shared && fs.last != slot ? fs.slot[fs.last].end : nullptr};
  if (slot == 1 && fs.fork) {  // whatever the renderer's stream did since the last join (edits, restarts, serial updates) comes first
    RT_HIP(hipEventRecord(fs.forked, r->stream));
    RT_HIP(hipStreamWaitEvent(s, fs.forked, 0));
    fs.fork = false;
  }
  // the camera-ray launch starts beside the last bounces of the update before it (kLeadBounces), which runs on the other slot
  if (overlapped && fs.last != slot) RT_HIP(hipStreamWaitEvent(s, fs.slot[fs.last].lead, 0));
  // slot 0 shares its control block and spill area with external trace_rays calls (which join both slots)
  if (slot == 0 && r->scratch.acquire(s) != HALA_OK) return HALA_ERR;
  RT_HIP(hipEventRecord(te.frame_begin, s));
  RT_HIP(hipMemsetAsync(run->ctl, 0, sizeof(Control), s));
  return HALA_OK;
}

// Step 3: the kernel sequence of the bounces on the stream of `run`, with the timing events of a timed update.
static int issue_bounces(hala_rt_renderer* r, const UpdatePlan& p, const SlotRun& run) {
  TraceEvents& te = *run.te;
  const hala_global_uniform& u = p.fc.u;
  Control* ctl = run.ctl;
  const hipStream_t s = run.stream;
  const bool timed = p.timed;
  // The shadow passes of bounce d and the closest-hit traversal of bounce d + 1 are independent: untimed updates issue them as ONE
  // persistent launch (k_trace_shadow_then_batch: one tail of long rays instead of three).  Updates that carry per-launch timing events or
  // counting kernels keep one launch per pass, so that every measured launch is one kernel symbol with the chip to itself.
  const bool fuse = (r->fuse_mode == 2u || (r->fuse_mode == 1u && !timed)) && !r->counting && (u.num_of_lights > 0 || u.env_type == 1u);
  if (timed && !te.host_sizes) RT_HIP(hipHostMalloc(reinterpret_cast<void**>(&te.host_sizes), sizeof(QueueSizes), hipHostMallocDefault));
  bool traced = false;  // the closest-hit pass of this depth already ran inside the previous depth's fused launch
  // where the next update may start (run.lead).  LDS-staged trees: behind the last shade (beside the last shadow launches and the resolve only)
  const uint32_t lead_bounces = r->staged ? 0u : std::min(kLeadBounces, r->max_depth - 1u);
  for (uint32_t depth = 0; depth < r->max_depth; ++depth) {
    if (timed) { hipEvent_t a = next_event(te); RT_HIP(hipEventRecord(a, s)); }
    // depth 0: the camera rays are generated inside the traversal kernel, there is no ray-generation pass
    if (depth == 0) {
      launch_trace_primary(run.lc, p.sv, p.fc, run.q.hits, &ctl->work_closest, ctl, p.primary_pixels * p.samples, r->counting, p.far_camera, s);
      if (r->counting) RT_HIP(hipMemcpyAsync(ctl->totals.primary_steps, ctl->totals.steps[0], 16, hipMemcpyDeviceToDevice, s));
      if (run.before_end) RT_HIP(hipStreamWaitEvent(s, run.before_end, 0));
    }
    else if (!traced) launch_trace_batch(run.lc, p.sv, run.q.rays[depth & 1u], run.q.hits, &ctl->sizes.n_active[depth], 0, &ctl->work_closest, ctl, false, r->counting, true, s);
    traced = false;
    if (timed) { hipEvent_t b = next_event(te); RT_HIP(hipEventRecord(b, s)); }
    launch_shade(p.fc, p.sv, run.q, run.ps, ctl, depth, s);
    if (depth + 1u + lead_bounces == r->max_depth) RT_HIP(hipEventRecord(run.lead, s));
    if (timed) { hipEvent_t c = next_event(te); RT_HIP(hipEventRecord(c, s)); }
    // light connections add to the path's L, environment connections to its Le (RENDER_SPEC §6): the two passes are independent of each
    // other and of the next bounce's closest-hit pass
    const uint32_t kinds = (u.num_of_lights > 0 ? 1u : 0u) | (u.env_type == 1u ? 2u : 0u);
    const bool last = depth + 1u >= r->max_depth;  // no closest-hit pass follows: only worth one launch when there are two shadow passes
    if (fuse && kinds && (!last || kinds == 3u) && launch_trace_shadow_then_batch(run.lc, p.sv, run.q, run.ps, ctl, depth, kinds, !last, s)) {
      traced = !last;
      if (timed) { te.fused_mask |= 1ull << depth; if (traced) te.traced_mask |= 1ull << (depth + 1u); }
    }
    else
      for (uint32_t kind = 0; kind < 2u; ++kind) {
        if (!((kinds >> kind) & 1u)) continue;
        launch_trace_shadow(run.lc, p.sv, run.q, run.ps, ctl, depth, kind, r->counting, s);
        te.shadow_launches += timed ? 1u : 0u;
      }
    if (timed) { hipEvent_t d = next_event(te); RT_HIP(hipEventRecord(d, s)); }
  }
  return HALA_OK;
}

// Step 4: the samples folded into the accumulated images in frame order, the read-backs, the end of the update and what the slots
// remember of it; then the snapshot and check frames of adaptive sampling.
static int finish_update(hala_rt_renderer* r, const UpdatePlan& p, const SlotRun& run) {
  FrameSlots& fs = r->slots;
  TraceEvents& te = *run.te;
  const int slot = run.slot;
  const hipStream_t s = run.stream;
  // everything that folds into the accumulated images stays in frame order: behind the fold of the update before this one
  if (fs.last_folded >= 0 && fs.last_folded != slot) RT_HIP(hipStreamWaitEvent(s, fs.slot[fs.last_folded].folded, 0));
  launch_resolve(p.fc, run.ps, r->img_local[0].ptr, r->img_local[1].ptr, r->img_local[2].ptr, r->img_local[3].ptr, r->has_image(4) ? r->img_local[4].ptr : nullptr,
                 r->has_image(5) ? reinterpret_cast<uint4*>(r->img_local[5].ptr) : nullptr, r->groups.img.ptr, r->image_alloc(), s);
  if (r->crypto.mask) {  // RENDER_SPEC §15: fold the batch's first hits right behind the resolve
    launch_crypto_fold(p.fc, run.ps.aov_ids, r->crypto.view(r->slot_count), r->crypto.rec.ptr, s);
    r->crypto.ready = true;
  }
  RT_HIP(hipEventRecord(fs.slot[slot].folded, s));
  fs.last_folded = slot; fs.last = slot;
  RT_HIP(hipMemcpyAsync(te.host_totals, &run.ctl->totals, sizeof(Totals), hipMemcpyDeviceToHost, s));
  if (p.timed) RT_HIP(hipMemcpyAsync(te.host_sizes, &run.ctl->sizes, sizeof(QueueSizes), hipMemcpyDeviceToHost, s));
  // frame_begin -> frame_end spans the whole update
  RT_HIP(hipEventRecord(te.frame_end, s));
  fs.slot[slot].end = te.frame_end;
  if (slot == 0) { r->scratch.event = te.frame_end; r->scratch.stream = s; }
  else { fs.open = true; fs.second_updates++; }
  RT_HIP(hipGetLastError());
  te.pending = true;
  for (bool& v : r->full_valid) v = false;
  // RENDER_SPEC 11: hala_rt_update_batch ends its chunks on these frames, so n is the snapshot or check frame itself
  AdaptiveState& ad = r->adaptive;
  const uint32_t n = (uint32_t)(p.first + p.samples);
  if (ad.enabled && (n == ad.p.min_samples / 2u || adaptive_is_check(ad.p, n)) && fs.join(r->stream) != HALA_OK) return HALA_ERR;  // they read the accumulation
  if (ad.enabled && n == ad.p.min_samples / 2u) {
    RT_HIP(hipMemcpyAsync(ad.snapshot.ptr, r->img_local[0].ptr, ad.snapshot.bytes(), hipMemcpyDeviceToDevice, r->stream));
    ad.last_snapshot = n;
  }
  if (ad.enabled && adaptive_is_check(ad.p, n)) {  // the one synchronising update: the next ones are sized by the two counts
    RT_HIP(adaptive_enqueue_check(ad, r->img_local[0].ptr, r->width, r->height, r->blocks_x, r->exposure, n, r->stream));
    RT_HIP(hipStreamSynchronize(r->stream));
    adaptive_finish_check(ad, n);
  }
  return HALA_OK;
}

static int update_impl(hala_rt_renderer* r, uint32_t frames) {
  RtRange range("halart::update");
  if (ensure_device(r, false) != HALA_OK) return HALA_ERR;
  UpdatePlan plan; SlotRun run;
  if (prepare_update(r, frames, &plan) != HALA_OK) return HALA_ERR;
  if (plan.samples == 0) return HALA_OK;  // frames past max_frames, or every block has converged
  if (begin_update(r, plan, &run) != HALA_OK || issue_bounces(r, plan, run) != HALA_OK) return HALA_ERR;
  return finish_update(r, plan, run);
}

int hala_rt_update(hala_rt_renderer* r, double, uint32_t, uint32_t) { return update_impl(r, 1); }

int hala_rt_update_batch(hala_rt_renderer* r, uint32_t frames) {
  if (!r) RT_FAIL("The renderer handle is null!");
  // several views multiply the paths per pixel slot: a chunk keeps them at kMaxSampleBatch at most (RENDER_SPEC §12)
  const uint32_t max_chunk = std::max(1u, kMaxSampleBatch / r->view_count());
  while (frames > 0) {
    uint32_t chunk = std::min(frames, max_chunk);
    if (r->adaptive.enabled && r->total_frames < r->max_frames)  // a chunk ends on the next snapshot or check frame (RENDER_SPEC 11)
      chunk = (uint32_t)std::min<uint64_t>(chunk, adaptive_frames_to_event(r->adaptive.p, r->total_frames));
    if (r->shutter.act.active() && r->total_frames < r->max_frames)  // ... and on the last frame of the shutter's step (RENDER_SPEC §18)
      chunk = std::min(chunk, r->shutter.act.stride - (uint32_t)r->total_frames % r->shutter.act.stride);
    if (update_impl(r, chunk) != HALA_OK) return HALA_ERR;
    frames -= chunk;
  }
  return HALA_OK;
}

int hala_rt_render(hala_rt_renderer* r) {  // src/rt_renderer.rs:475-502: nothing to present; make the frame's work visible
  if (ensure_device(r, false) != HALA_OK) return HALA_ERR;
  if (r->total_frames > r->max_frames) return HALA_OK;  // :484-486
  // submit_and_present_frame hands the frame to the queue and only blocks on the fence of the swapchain image it reuses: with no
  // swapchain here, render() bounds the updates in flight to two (it waits for the update before the latest), so the host can
  // enqueue the next frame while this one runs.  Everything that reads results (read_image, save_images, statistics, wait_idle,
  // tile_buffer users via wait_idle) synchronises on its own.
  const TraceEvents& before_last = r->ring[(r->ring_pos + kStatRing - 2) % kStatRing];
  if (before_last.pending && before_last.frame_end) RT_HIP(hipEventSynchronize(before_last.frame_end));
  return HALA_OK;
}
int hala_rt_wait_idle(hala_rt_renderer* r) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  RT_HIP(hipStreamSynchronize(r->stream));
  return HALA_OK;
}

int hala_rt_read_image(hala_rt_renderer* r, int which, float* dst) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!r->has_image(which) || !dst) RT_FAIL("Invalid image selector.");
  RT_HIP(hipStreamSynchronize(r->stream));  // wait_idle (src/rt_renderer.rs:1242)
  const size_t bytes = (size_t)r->width * r->height * sizeof(float4);
  if (r->world <= 1) { RT_HIP(hipMemcpy(dst, r->img_local[which].ptr, bytes, hipMemcpyDeviceToHost)); return HALA_OK; }
  if (!r->full_valid[which]) RT_FAIL("The frame is sharded across ranks: gather the tiles (hala_rt_scatter_gathered_tiles) before reading the image.");
  RT_HIP(hipMemcpy(dst, r->img_full[which].ptr, bytes, hipMemcpyDeviceToHost));
  return HALA_OK;
}

int hala_rt_save_images(hala_rt_renderer* r, const char* path) {
  RtRange range("halart::save_images");
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!path || !*path) RT_FAIL("The file name is none!");  // src/rt_renderer.rs:1234
  std::string p(path);
  const size_t slash = p.find_last_of("/\\");
  const std::string dir = slash == std::string::npos ? "" : p.substr(0, slash + 1);
  const std::string stem = file_stem(path);
  std::vector<float> px((size_t)r->width * r->height * 4);
  static const char* suffix[3] = {"_color.pfm", "_albedo.pfm", "_normal.pfm"};  // :1235-1237
  for (int which = 0; which < 3; ++which) {
    if (hala_rt_read_image(r, which, px.data()) != HALA_OK) return HALA_ERR;
    if (which == 0) tonemap_pixels(px.data(), (size_t)r->width * r->height, r->enable_tonemap, r->enable_aces, r->use_simple_aces);  // :1256-1316
    const std::string e = write_pfm((dir + stem + suffix[which]).c_str(), px.data(), r->width, r->height);
    if (!e.empty()) RT_FAIL(e);
  }
  return HALA_OK;
}

int hala_rt_get_info(hala_rt_renderer* r, hala_rt_info* out) {
  if (!r || !out) RT_FAIL("The renderer handle is null!");
  out->width = r->width; out->height = r->height;
  return HALA_OK;
}
int hala_rt_get_statistics(hala_rt_renderer* r, hala_rt_statistics* out) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!out) RT_FAIL("The output pointer is null!");
  RT_HIP(hipStreamSynchronize(r->stream));
  for (int k = 0; k < kStatRing; ++k) resolve_slot(r, r->ring[(r->ring_pos + k) % kStatRing]);  // oldest first
  r->stats.total_frames = r->total_frames;
  *out = r->stats;
  return HALA_OK;
}
int hala_rt_reset_accumulation(hala_rt_renderer* r) {
  if (!r) RT_FAIL("The renderer handle is null!");
  r->reset_accumulation();
  return HALA_OK;
}

int hala_rt_set_launch_timing_period(hala_rt_renderer* r, uint32_t period) {
  if (!r) RT_FAIL("The renderer handle is null!");
  r->launch_event_period = period;
  r->update_counter = 0;
  return HALA_OK;
}
int hala_rt_set_frames_in_flight(hala_rt_renderer* r, uint32_t n) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;  // joins both slots
  if (n != 1u && n != 2u) RT_FAIL("hala_rt_set_frames_in_flight: n must be 1 or 2.");
  r->slots.in_flight = n;
  r->slots.second_failed = false;
  if (n == 1u) {  // strictly serial: one slot, one stream, one set of buffers
    RT_HIP(hipStreamSynchronize(r->stream));
    r->slots.slot[1].set.release();
  }
  return HALA_OK;
}
int hala_rt_frames_in_flight_info(hala_rt_renderer* r, unsigned long long* second_slot_updates, uint32_t* second_buffers) {
  if (!r) RT_FAIL("The renderer handle is null!");
  if (second_slot_updates) *second_slot_updates = r->slots.second_updates;
  if (second_buffers) *second_buffers = r->slots.slot[1].set.shape.paths ? 1u : 0u;
  return HALA_OK;
}
int hala_rt_set_pass_fusion(hala_rt_renderer* r, uint32_t mode) {
  if (!r) RT_FAIL("The renderer handle is null!");
  if (mode > 2u) RT_FAIL("Invalid pass fusion mode.");
  r->fuse_mode = mode;
  return HALA_OK;
}
int hala_rt_variant_ledger(uint32_t family, uint64_t* launched, uint64_t* built, int reset) {
  if (!variant_ledger(family, launched, built, reset != 0))
    RT_FAIL("hala_rt_variant_ledger: there is no kernel family " + std::to_string(family) + " (0 ... " + std::to_string(kVariantFamilies - 1u) + ").");
  return HALA_OK;
}
int hala_rt_set_counting(hala_rt_renderer* r, int enable) {
  if (!r) RT_FAIL("The renderer handle is null!");
  r->counting = enable != 0;
  return HALA_OK;
}
int hala_rt_get_global_uniform(hala_rt_renderer* r, hala_global_uniform* out) {
  if (!r || !out) RT_FAIL("The renderer handle is null!");
  *out = r->last_uniform;
  return HALA_OK;
}

#define RT_READBACK(dev, T, dst, cap, cnt)                                                               \
  do {                                                                                                     \
    *(cnt) = (uint32_t)(dev).count;                                                                        \
    const size_t _n = std::min<size_t>((cap), (dev).count);                                                \
    if ((dst) && _n) RT_HIP(hipMemcpy((dst), (dev).ptr, _n * sizeof(T), hipMemcpyDeviceToHost));           \
  } while (0)

int hala_rt_get_packed_cameras(hala_rt_renderer* r, hala_gpu_camera* dst, uint32_t capacity, uint32_t* count) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!r->has_scene || !count) RT_FAIL("The scene in GPU is none!");
  RT_READBACK(r->d_cameras, hala_gpu_camera, dst, capacity, count);
  return HALA_OK;
}
int hala_rt_get_packed_lights(hala_rt_renderer* r, hala_gpu_light* dst, hala_aabb* bb, uint32_t capacity, uint32_t* count) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!r->has_scene || !count) RT_FAIL("The scene in GPU is none!");
  RT_READBACK(r->d_lights, hala_gpu_light, dst, capacity, count);
  if (bb) memcpy(bb, r->hs.light_aabbs.data(), std::min<size_t>(capacity, r->hs.light_aabbs.size()) * sizeof(hala_aabb));
  return HALA_OK;
}
int hala_rt_get_packed_materials(hala_rt_renderer* r, hala_gpu_material* dst, uint32_t capacity, uint32_t* count) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!r->has_scene || !count) RT_FAIL("The scene in GPU is none!");
  RT_READBACK(r->d_materials, hala_gpu_material, dst, capacity, count);
  return HALA_OK;
}
int hala_rt_get_packed_primitives(hala_rt_renderer* r, hala_gpu_mesh_data* dst, float* t3x4, uint32_t capacity, uint32_t* count) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!r->has_scene || !count) RT_FAIL("The scene in GPU is none!");
  RT_READBACK(r->d_instances, hala_gpu_mesh_data, dst, capacity, count);
  r->sync_host_mirror();
  if (t3x4) memcpy(t3x4, r->hs.instance_3x4.data(), std::min<size_t>(capacity, r->hs.instances.size()) * 12 * sizeof(float));
  return HALA_OK;
}
int hala_rt_get_env_distribution(hala_rt_renderer* r, float* total_sum, float* marginal, float* conditional) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!r->has_env) RT_FAIL("The environment map is none!");
  if (total_sum) *total_sum = r->env_total_sum;
  if (marginal) RT_HIP(hipMemcpy(marginal, r->d_marginal.ptr, (size_t)r->env_h * 4, hipMemcpyDeviceToHost));
  if (conditional) RT_HIP(hipMemcpy(conditional, r->d_conditional.ptr, (size_t)r->env_w * r->env_h * 4, hipMemcpyDeviceToHost));
  return HALA_OK;
}

}  // extern "C"
