// rt_post.hip — what runs on the accumulated frame after the updates: denoising (RENDER_SPEC 10, DenoiseBuffers) and temporal
// reprojection (RENDER_SPEC 16, TemporalState).  The kernels are in denoise.hip and temporal.hip.
#include "renderer_state.h"

namespace {

// The GPU time of what a caller enqueues between begin() and end(), for the entry points that report one.  Untimed (gpu_ms == NULL) it
// creates no event and both calls do nothing.
struct GpuTimer {
  hipEvent_t ev[2] = {nullptr, nullptr};
  float* ms = nullptr;
  ~GpuTimer() { for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x); }
  int create(float* gpu_ms) {
    ms = gpu_ms;
    if (!ms) return HALA_OK;
    RT_HIP(hipEventCreate(&ev[0]));
    if (hipEventCreate(&ev[1]) != hipSuccess) RT_FAIL("hipEventCreate failed.");
    return HALA_OK;
  }
  hipError_t begin(hipStream_t s) { return ms ? hipEventRecord(ev[0], s) : hipSuccess; }
  // `e`: what the enqueue returned; a failure passes through, otherwise the stream is waited for and *ms written
  hipError_t end(hipError_t e, hipStream_t s) {
    if (e == hipSuccess && ms) e = hipEventRecord(ev[1], s);
    if (e == hipSuccess && ms) e = hipEventSynchronize(ev[1]);
    if (e == hipSuccess && ms) e = hipEventElapsedTime(ms, ev[0], ev[1]);
    return e;
  }
};

}  // namespace

extern "C" {

// ---- denoising (RENDER_SPEC 10) -----------------------------------------------------------------------------------------------
int hala_rt_denoise(hala_rt_renderer* r, const hala_denoise_params* p, float* gpu_ms) {
  RtRange range("halart::denoise");
  const std::string bad = denoise_check_params(p);  // first: the CPU tier pins it without a renderer
  if (!bad.empty()) RT_FAIL(bad);
  if (!r) RT_FAIL("The renderer handle is null!");
  if (r->total_frames == 0) RT_FAIL("Nothing to denoise: no sample has been accumulated since the renderer was created or its accumulation reset.");
  if (r->world > 1 && !(r->full_valid[0] && r->full_valid[1] && r->full_valid[2]))
    RT_FAIL("The frame is sharded across ranks: gather AOVs 0, 1 and 2 (accum, albedo, normal) before denoising.");
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  DeviceArray<float4>* img = r->world > 1 ? r->img_full : r->img_local;
  RT_HIP(r->denoise.ensure(r->width, r->height));
  GpuTimer timer;
  if (timer.create(gpu_ms) != HALA_OK) return HALA_ERR;
  hipError_t e = timer.begin(r->stream);
  if (e == hipSuccess) e = denoise_enqueue(r->denoise, img[0].ptr, img[1].ptr, img[2].ptr, *p, r->stream);
  e = timer.end(e, r->stream);
  if (e != hipSuccess) RT_FAIL(std::string("hala_rt_denoise: ") + hipGetErrorString(e));
  r->denoised = true;
  return HALA_OK;
}
int hala_rt_read_denoised(hala_rt_renderer* r, float* dst) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!dst) RT_FAIL("Invalid argument.");
  if (!r->denoised) RT_FAIL("Nothing has been denoised yet (hala_rt_denoise).");
  RT_HIP(hipStreamSynchronize(r->stream));
  RT_HIP(hipMemcpy(dst, r->denoise.out.ptr, (size_t)r->denoise.width * r->denoise.height * sizeof(float4), hipMemcpyDeviceToHost));
  return HALA_OK;
}
int hala_rt_get_denoised_buffer(hala_rt_renderer* r, void** d_ptr, size_t* bytes) {
  if (!r || !d_ptr || !bytes) RT_FAIL("Invalid argument.");
  if (!r->denoised) RT_FAIL("Nothing has been denoised yet (hala_rt_denoise).");
  *d_ptr = r->denoise.out.ptr;
  *bytes = (size_t)r->denoise.width * r->denoise.height * sizeof(float4);
  return HALA_OK;
}
int hala_rt_save_denoised(hala_rt_renderer* r, const char* path) {
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  if (!path || !*path) RT_FAIL("The file name is none!");
  if (!r->denoised) RT_FAIL("Nothing has been denoised yet (hala_rt_denoise).");
  std::string p(path);
  const size_t slash = p.find_last_of("/\\");
  const std::string dir = slash == std::string::npos ? "" : p.substr(0, slash + 1);
  const size_t n = (size_t)r->denoise.width * r->denoise.height;
  std::vector<float> px(n * 4);
  if (hala_rt_read_denoised(r, px.data()) != HALA_OK) return HALA_ERR;
  tonemap_pixels(px.data(), n, r->enable_tonemap, r->enable_aces, r->use_simple_aces);  // as save_images treats _color.pfm
  const std::string e = write_pfm((dir + file_stem(path) + "_denoised.pfm").c_str(), px.data(), r->denoise.width, r->denoise.height);
  if (!e.empty()) RT_FAIL(e);
  return HALA_OK;
}

// ---- temporal reprojection (RENDER_SPEC 16) ------------------------------------------------------------------------------------
static int temporal_ready(hala_rt_renderer* r, const char* fn) {
  if (!r) RT_FAIL("The renderer handle is null!");
  if (!r->temporal.enabled) RT_FAIL(std::string(fn) + ": temporal reprojection is off (hala_rt_set_temporal).");
  if ((r->aov_mask & 3u) != 3u) RT_FAIL(std::string(fn) + ": the position and ids AOVs must both be on (hala_rt_set_aovs(r, 3)).");
  if (!r->committed) RT_FAIL(std::string(fn) + ": no scene is committed.");
  if (r->views[0] >= r->hs.cameras.size()) RT_FAIL(std::string(fn) + ": view 0 renders a camera the committed scene lacks (hala_rt_set_views).");
  return HALA_OK;
}
// The table of this resolve (temporal.h) and the launch, on the renderer's stream, which has joined the second frame slot.  The table is rebuilt and
// uploaded only while TemporalState::table_dirty (after a capture, a mark, a refit, ...), behind a wait for the resolves that still read the
// old one; every other resolve is the launch alone.
static int temporal_enqueue_resolve(hala_rt_renderer* r, hipEvent_t before = nullptr) {
  TemporalState& t = r->temporal;
  r->sync_host_mirror();  // RENDER_SPEC §20: the motion of an instance is read off the host's instance transforms
  const HostScene& hs = r->hs;
  const uint32_t cam = r->views[0];
  const bool hist = t.has_history && t.world.size() == 16 * hs.instances.size() && t.inst_marked.size() == hs.instances.size() &&
                    t.mat_marked.size() == hs.gpu_materials.size();
  const uint32_t ni = hist ? (uint32_t)hs.instances.size() : 0u, nm = hist ? (uint32_t)hs.gpu_materials.size() : 0u;
  // RENDER_SPEC 16 "Vertex motion": the snapshot can follow a vertex edit only on the one-level tree it was taken from
  const bool follow = hist && t.vertex_motion && t.has_snapshot && !r->two_level && t.snapshot.count == r->bvh.tri_count && r->bvh.tri_count != 0u;
  if (t.table_dirty || !t.table.ptr) {
    constexpr size_t kHeadWords = sizeof(TemporalHead) / 4, kInstWords = sizeof(TemporalInst) / 4;
    std::vector<uint32_t> tab(kHeadWords + (size_t)ni * kInstWords + nm, 0u);
    TemporalHead hd{};
    hd.cur = temporal_camera(hs.cameras[cam], r->view_const(cam, (float)r->height).tan_half);
    hd.prev = hist ? temporal_camera(t.cam, t.tan_half) : hd.cur;
    hd.width = (float)r->width; hd.height = (float)r->height; hd.aspect = hd.width / hd.height;
    hd.max_history = t.p.max_history; hd.tol = t.p.tol; hd.min_weight = t.p.min_weight;
    hd.inst_count = ni; hd.mat_count = nm;
    memcpy(tab.data(), &hd, sizeof(hd));
    t.table_vertex = false;
    for (uint32_t i = 0; i < ni; ++i) {
      TemporalInst ti{};
      const bool ok = temporal_motion(&t.world[16 * (size_t)i], hs.instances[i].transform, ti.d);
      ti.marked = !ok ? 1u : (t.inst_marked[i] ? (follow ? 2u : 1u) : 0u);
      t.table_vertex = t.table_vertex || ti.marked == 2u;
      memcpy(tab.data() + kHeadWords + (size_t)i * kInstWords, &ti, sizeof(ti));
    }
    for (uint32_t m = 0; m < nm; ++m) tab[kHeadWords + (size_t)ni * kInstWords + m] = t.mat_marked[m] ? 1u : 0u;
    RT_HIP(hipStreamSynchronize(r->stream));
    RT_HIP(t.table.upload(tab.data(), tab.size(), r->stream));
    RT_HIP(hipStreamSynchronize(r->stream));
    t.table_dirty = false;
  }
  if (before) RT_HIP(hipEventRecord(before, r->stream));  // a timed resolve brackets the launch alone
  launch_temporal_resolve(r->img_local[0].ptr, r->img_local[4].ptr, reinterpret_cast<const uint4*>(r->img_local[5].ptr), t.hc.ptr, t.hp.ptr,
                          reinterpret_cast<const uint4*>(t.hi.ptr), t.table.ptr, r->width, r->height, r->rendered_frames(), hist, t.out[0].ptr,
                          t.out[1].ptr, t.table_vertex ? r->d_tris_by_id.ptr : nullptr, t.table_vertex ? t.snapshot.ptr : nullptr,
                          t.table_vertex ? r->bvh.tri_count : 0u, t.clamp ? &t.cp : nullptr, r->stream);
  RT_HIP(hipGetLastError());
  t.resolved = true;
  return HALA_OK;
}
int hala_rt_set_temporal(hala_rt_renderer* r, const hala_temporal_params* p) {
  if (p) {
    const std::string bad = temporal_check_params(p);  // first: the CPU tier pins it without a renderer
    if (!bad.empty()) RT_FAIL(bad);
  }
  if (!r) RT_FAIL("The renderer handle is null!");
  if (p && r->world > 1) RT_FAIL("hala_rt_set_temporal: temporal reprojection is not available on a sharded renderer (world > 1).");
  if (p && r->view_count() > 1u) RT_FAIL("hala_rt_set_temporal: temporal reprojection is not available with several views (hala_rt_set_views with one camera first).");
  if (p && r->adaptive.enabled) RT_FAIL("hala_rt_set_temporal: temporal reprojection is not available with adaptive sampling on (hala_rt_set_adaptive_sampling(r, NULL) first).");
  if (p && (r->shutter.rec.on || r->shutter.act.on)) RT_FAIL("hala_rt_set_temporal: temporal reprojection is not available with the shutter on (hala_rt_set_shutter(r, NULL) first).");
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  TemporalState& t = r->temporal;
  if (!p) {
    if (t.enabled) { RT_HIP(hipStreamSynchronize(r->stream)); t.release(); }
    return HALA_OK;
  }
  if (!t.enabled) {
    const size_t n = (size_t)r->width * r->height;
    hipError_t e = hipSuccess;
    for (DeviceArray<float4>* a : {&t.hc, &t.hp, &t.hi, &t.out[0], &t.out[1]})
      if (e == hipSuccess) e = a->resize(n);
    if (e != hipSuccess) { t.release(); RT_HIP(e); }  // out of memory: the feature stays off
    t.enabled = true;
  }
  t.p = *p;
  t.table_dirty = true;
  return HALA_OK;
}
int hala_rt_set_temporal_vertex_motion(hala_rt_renderer* r, int enable) {
  if (!r) RT_FAIL("The renderer handle is null!");
  if (!r->temporal.enabled) RT_FAIL("hala_rt_set_temporal_vertex_motion: temporal reprojection is off (hala_rt_set_temporal).");
  TemporalState& t = r->temporal;
  if (!enable && t.has_snapshot) {
    if (ensure_device(r) != HALA_OK) return HALA_ERR;
    RT_HIP(hipStreamSynchronize(r->stream));  // a resolve may still read the snapshot
    t.drop_snapshot();
  }
  t.vertex_motion = enable != 0;
  t.table_dirty = true;
  return HALA_OK;
}
int hala_rt_set_temporal_clamp(hala_rt_renderer* r, const hala_temporal_clamp_params* p) {
  if (p) {
    const std::string bad = temporal_check_clamp_params(p);  // first: the CPU tier pins it without a renderer
    if (!bad.empty()) RT_FAIL(bad);
  }
  if (!r) RT_FAIL("The renderer handle is null!");
  if (!r->temporal.enabled) RT_FAIL("hala_rt_set_temporal_clamp: temporal reprojection is off (hala_rt_set_temporal).");
  // two launch arguments of the next resolve: nothing on the device changes, and the resolves enqueued so far keep theirs
  r->temporal.clamp = p != nullptr;
  if (p) r->temporal.cp = *p;
  return HALA_OK;
}
int hala_rt_temporal_capture(hala_rt_renderer* r) {
  RtRange range("halart::temporal_capture");
  if (temporal_ready(r, "hala_rt_temporal_capture") != HALA_OK) return HALA_ERR;
  if (r->rendered_frames() == 0) return HALA_OK;  // two edits with no frame between: the history stands
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  TemporalState& t = r->temporal;
  // RENDER_SPEC 16 "Vertex motion": the snapshot of the new history.  A snapshot of another size follows nothing, so it goes before the
  // resolve; one of this size is what the resolve reads, and the copy below overwrites it behind the resolve on the same stream.
  const uint32_t snap_count = t.vertex_motion && !r->two_level ? r->bvh.tri_count : 0u;
  if (t.has_snapshot && t.snapshot.count != snap_count) { RT_HIP(hipStreamSynchronize(r->stream)); t.drop_snapshot(); }
  if (snap_count) RT_HIP(t.snapshot.resize(snap_count));
  if (temporal_enqueue_resolve(r) != HALA_OK) return HALA_ERR;
  if (snap_count) RT_HIP(hipMemcpyAsync(t.snapshot.ptr, r->d_tris_by_id.ptr, (size_t)snap_count * sizeof(Tri), hipMemcpyDeviceToDevice, r->stream));
  t.has_snapshot = snap_count != 0u;
  const size_t bytes = (size_t)r->width * r->height * sizeof(float4);
  RT_HIP(hipMemcpyAsync(t.hc.ptr, t.out[0].ptr, bytes, hipMemcpyDeviceToDevice, r->stream));
  RT_HIP(hipMemcpyAsync(t.hp.ptr, r->img_local[4].ptr, bytes, hipMemcpyDeviceToDevice, r->stream));
  RT_HIP(hipMemcpyAsync(t.hi.ptr, r->img_local[5].ptr, bytes, hipMemcpyDeviceToDevice, r->stream));
  const HostScene& hs = r->hs;
  t.cam = hs.cameras[r->views[0]];
  t.tan_half = r->view_const(r->views[0], (float)r->height).tan_half;
  t.world.resize(16 * hs.instances.size());
  for (size_t i = 0; i < hs.instances.size(); ++i) memcpy(&t.world[16 * i], hs.instances[i].transform, 64);
  t.inst_marked.assign(hs.instances.size(), 0);
  t.mat_marked.assign(hs.gpu_materials.size(), 0);
  t.has_history = true;
  t.table_dirty = true;
  return HALA_OK;
}
int hala_rt_temporal_resolve(hala_rt_renderer* r, float* gpu_ms) {
  RtRange range("halart::temporal_resolve");
  if (temporal_ready(r, "hala_rt_temporal_resolve") != HALA_OK) return HALA_ERR;
  if (r->rendered_frames() == 0) RT_FAIL("hala_rt_temporal_resolve: no sample has been folded since the accumulation restarted.");
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  GpuTimer timer;
  if (timer.create(gpu_ms) != HALA_OK) return HALA_ERR;
  if (temporal_enqueue_resolve(r, timer.ev[0]) != HALA_OK) return HALA_ERR;  // (records the first event itself, behind the table upload)
  const hipError_t e = timer.end(hipSuccess, r->stream);
  if (e != hipSuccess) RT_FAIL(std::string("hala_rt_temporal_resolve: ") + hipGetErrorString(e));
  return HALA_OK;
}
static int temporal_output_check(hala_rt_renderer* r, int which) {
  if (!r) RT_FAIL("The renderer handle is null!");
  if (which < 0 || which > 1) RT_FAIL("Invalid temporal image selector (0: temporal, 1: motion).");
  if (!r->temporal.enabled) RT_FAIL("Temporal reprojection is off (hala_rt_set_temporal).");
  if (!r->temporal.resolved) RT_FAIL("Nothing has been resolved yet (hala_rt_temporal_resolve).");
  return HALA_OK;
}
int hala_rt_read_temporal(hala_rt_renderer* r, int which, float* dst) {
  if (temporal_output_check(r, which) != HALA_OK) return HALA_ERR;
  if (!dst) RT_FAIL("The output pointer is null!");
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  RT_HIP(hipStreamSynchronize(r->stream));
  RT_HIP(hipMemcpy(dst, r->temporal.out[which].ptr, r->temporal.out[which].bytes(), hipMemcpyDeviceToHost));
  return HALA_OK;
}
int hala_rt_get_temporal_buffer(hala_rt_renderer* r, int which, void** d_ptr, size_t* bytes) {
  if (temporal_output_check(r, which) != HALA_OK) return HALA_ERR;
  if (!d_ptr || !bytes) RT_FAIL("Invalid argument.");
  *d_ptr = r->temporal.out[which].ptr;
  *bytes = r->temporal.out[which].bytes();
  return HALA_OK;
}
int hala_rt_denoise_temporal(hala_rt_renderer* r, const hala_denoise_params* p, float* gpu_ms) {
  RtRange range("halart::denoise_temporal");
  const std::string bad = denoise_check_params(p);  // first, as in hala_rt_denoise
  if (!bad.empty()) RT_FAIL(bad);
  if (temporal_output_check(r, 0) != HALA_OK) return HALA_ERR;
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  RT_HIP(r->denoise.ensure(r->width, r->height));
  GpuTimer timer;
  if (timer.create(gpu_ms) != HALA_OK) return HALA_ERR;
  hipError_t e = timer.begin(r->stream);
  if (e == hipSuccess) e = denoise_enqueue(r->denoise, r->temporal.out[0].ptr, r->img_local[1].ptr, r->img_local[2].ptr, *p, r->stream);
  e = timer.end(e, r->stream);
  if (e != hipSuccess) RT_FAIL(std::string("hala_rt_denoise_temporal: ") + hipGetErrorString(e));
  r->denoised = true;
  return HALA_OK;
}

}  // extern "C"
