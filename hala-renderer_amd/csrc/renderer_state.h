// renderer_state.h — the renderer object behind the C ABI (struct hala_rt_renderer), shared by the host units that implement it:
// renderer.hip (life cycle, scene, update), rt_scene.hip (uploads, edits), rt_trees.hip (trees, refit sequence), rt_outputs.hip (views, AOVs, adaptive sampling, light
// groups), rt_cryptomatte.hip, rt_post.hip (denoise, temporal reprojection), rt_deform.hip (deformers), rt_rig.hip (rigs and clips), rt_shutter.hip (shutter motion blur), rt_nodes.hip (node batches), rt_tiles.hip (tile shard and exchange), rt_rays.hip (ray batches), rt_queries.hip and rt_bake.hip (the other query batches).
// Each feature keeps its state in one struct that knows how to turn itself off.  What is indexed by path slot (per-path state, queues)
// lives in the WavefrontSet of a frame slot (FrameSlots::slot[2]: two updates in flight), sized by WavefrontSet::fit to the one PathShape
// that hala_rt_renderer::path_shape() computes: a feature with per-path state adds a field to the shape and an array to the set.
// Nothing outside csrc/ includes this header.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <sys/stat.h>
#include <vector>

#include "adaptive.h"
#include "cryptomatte.h"
#include "deform.h"
#include "denoise.h"
#include "dyn_api.h"
#include "hala_types.h"
#include "host_image.h"
#include "host_scene.h"
#include "host_util.h"
#include "kernels.h"
#include "node_batch.h"
#include "rig.h"
#include "shutter.h"
#include "temporal.h"

namespace rt { std::string decode_image_file_rgba8(const char* path, uint32_t* w, uint32_t* h, std::vector<uint8_t>* rgba); }  // gltf_loader.cpp

#pragma GCC visibility push(hidden)  // internal to libhalart.so: nothing below joins the exported symbols

namespace rt {

constexpr uint32_t kLeafMax = 4;  // triangles per leaf, large scenes: the wave tests a leaf's triangles side by side (traverse.h), so fewer, fuller leaves win (profiles/r02_experiments.txt; 2 while each lane tested its own leaves)
constexpr uint32_t kLeafMaxStaged = 4;  // ... unless the whole tree sits in LDS: leaves of two packed pairs, fewer node steps (+2 % on Cornell)
constexpr size_t kLdsStageBudget = 40 * 1024;  // a BVH up to this size is staged whole in LDS (next to the 24-KB stack)
constexpr uint32_t kRefillThreshold = 24;      // idle lanes that trigger a refill of the wave (persistent_trace; profiles/r02_experiments.txt)
constexpr int kStatRing = 16;
// maps a material must reference to get a texel bundle.  Measured on configs[3] (profiles/texture_bundles.txt): the two-map DIFFUSE
// materials (base colour + normal) gain from the 16-B bundle too, although half of every texel they load is idle
#ifndef RT_BUNDLE_MIN_MAPS
#define RT_BUNDLE_MIN_MAPS 2
#endif
constexpr uint32_t kBundleMinMaps = RT_BUNDLE_MIN_MAPS;
// Two updates in flight (FrameSlots): the next update starts behind the shade of the bounce this many before the last one of the update
// before it, so that its camera-ray launch and depth-0 shade (dense work) run beside that update's last launches (short queues: mostly
// the tails of a few long rays), not beside its dense early bounces.  Measured on configs[3] (profiles/frames_in_flight.txt): 1 is
// best; 0 (behind the last shade) equals the former tail stream; starting earlier, or with no start dependency at all, is slower.
constexpr uint32_t kLeadBounces = 1;
constexpr uint32_t kMaxSampleBatch = 16;  // frames per wavefront pass in hala_rt_update_batch (~250 B of state per path)

// ---- RENDER_SPEC §2.2 on the host (for tan(yfov/2); same polynomials as rt_math.h) ---------------------------
inline float h_sin_poly(float a) {
  float a2 = a * a;
  float p = -2.50521083854417187751e-8f;
  p = std::fmaf(p, a2, 2.75573192239858906526e-6f);
  p = std::fmaf(p, a2, -1.98412698412698412698e-4f);
  p = std::fmaf(p, a2, 8.33333333333333333333e-3f);
  p = std::fmaf(p, a2, -1.66666666666666666667e-1f);
  p = std::fmaf(p, a2, 1.0f);
  return a * p;
}
inline float h_cos_poly(float a) {
  float a2 = a * a;
  float p = 2.08767569878680989792e-9f;
  p = std::fmaf(p, a2, -2.75573192239858906526e-7f);
  p = std::fmaf(p, a2, 2.48015873015873015873e-5f);
  p = std::fmaf(p, a2, -1.38888888888888888889e-3f);
  p = std::fmaf(p, a2, 4.16666666666666666667e-2f);
  p = std::fmaf(p, a2, -0.5f);
  p = std::fmaf(p, a2, 1.0f);
  return p;
}
inline void h_sincos_rad(float a, float* s, float* c) {
  float t = a * 0.15915494309189533577f;
  t = t - std::floor(t);
  if (t >= 1.0f) t = 0.0f;
  float x = t * 4.0f;
  int q = (int)x;
  float f = x - (float)q;
  float ang = f * 1.57079632679489661923f;
  float sa = h_sin_poly(ang), ca = h_cos_poly(ang);
  switch (q & 3) {
    case 0: *s = sa; *c = ca; break;
    case 1: *s = ca; *c = -sa; break;
    case 2: *s = -sa; *c = -ca; break;
    default: *s = -ca; *c = sa; break;
  }
}

struct TraceEvents {
  std::vector<hipEvent_t> ev;  // pairs
  size_t used = 0;
  hipEvent_t frame_begin = nullptr, frame_end = nullptr;
  bool pending = false, counted = false;
  uint32_t samples = 1;  // frames rendered by this wavefront pass
  uint32_t primary_pixels = 0;  // pixels that traced a camera ray per frame (all real ones; the active blocks' under adaptive sampling)
  uint32_t shadow_launches = 0;  // k_trace_shadow launches inside the timed brackets of this pass (0, 1 or 2 per depth)
  // timed passes: bit d of fused_mask = the third bracket of depth d holds a fused launch (k_trace_shadow_then_batch); bit d of
  // traced_mask = the closest-hit pass of depth d ran inside depth d - 1's fused launch (its own bracket is empty)
  unsigned long long fused_mask = 0, traced_mask = 0;
  QueueSizes* host_sizes = nullptr;  // pinned copy of Control::sizes as the pass left it (timed passes only)
  Totals* host_totals = nullptr;     // pinned copy of Control::totals
};

// ---- one struct per feature -------------------------------------------------------------------------------------------------------

// texel bundles (hala_types.h: BundleDesc): the co-sized 8-bit maps of a material interleaved, built by commit beside the per-texture
// arenas; a refit follows material edits (update_texture_bundles)
struct BundleState {
  struct Source { uint32_t image[kBundleLanes], texture[kBundleLanes]; };  // per lane: the image (what bundles are shared by) and one texture that shows it, kAbsent = no map
  uint32_t mode = 0;  // hala_rt_build_options::texture_bundles: 0 automatic (on), 1 off
  bool on = false;    // as the last commit decided (automatic mode gives up when the arena cannot be had)
  std::vector<Source> sources;
  std::vector<BundleDesc> host;
  DeviceArray<uint4> d_arena;
  DeviceArray<BundleDesc> d_descs;
  DeviceArray<uint32_t> d_material;
  uint32_t bundled_materials = 0, unbundled_textured_materials = 0;
  void off() { on = false; sources.clear(); host.clear(); d_arena.release(); }  // every material on the per-texture path
};

// light groups (RENDER_SPEC §14; hala_rt_set_light_groups): count 0 = off.  The tables as set (they may cover more lights /
// materials than the committed scene has); img holds group g of every view at g * image_alloc(), laid out like accum
struct LightGroupState {
  uint32_t count = 0, env_group = 0;
  std::vector<uint32_t> light_group, material_group;
  DeviceArray<uint32_t> d_light_group, d_material_group;
  DeviceArray<float4> img;
  DeviceArray<float4> relit[2];  // hala_rt_relight: linear, tonemapped (W x H)
  bool relit_valid = false;
  void off() {  // (the per-path sums belong to the frame slots: hala_rt_renderer::fit_paths)
    count = 0; env_group = 0;
    light_group.clear(); material_group.clear();
    d_light_group.release(); d_material_group.release(); img.release();
    relit[0].release(); relit[1].release(); relit_valid = false;
  }
};

// Cryptomatte (RENDER_SPEC §15; hala_rt_set_cryptomatte): layer mask 0 = off.  rec holds one 64-B record (4 quads) per pixel slot,
// view and enabled layer (cryptomatte.h: CryptoTables); the id tables are filled by the first update after commit, refit or the call.
// While on, the depth-0 shade writes the 16-B first-hit record of every path slot (WavefrontSet::aov_ids) whether or not image 5 is on.
struct CryptoState {
  uint32_t mask = 0;
  std::vector<std::string> material_names;  // the caller's names ("" = material<m>)
  DeviceArray<uint4> rec;
  std::vector<uint32_t> object, asset, material;  // ids per node / node / material, as uploaded
  DeviceArray<uint32_t> d_object, d_asset, d_material;
  bool tables = false;  // the tables belong to the committed scene
  bool ready = false;   // an update has folded samples since the accumulation restarted
  size_t quads(uint32_t views, uint32_t slot_count) const { return 4 * (size_t)__builtin_popcount(mask) * views * slot_count; }
  CryptoTables view(uint32_t slot_count) const {
    return CryptoTables{d_object.ptr, d_asset.ptr, d_material.ptr, (uint32_t)object.size(), (uint32_t)material.size(), mask, slot_count};
  }
  void off() {  // (the first-hit records belong to the frame slots: hala_rt_renderer::fit_paths)
    mask = 0; material_names.clear(); tables = false;
    rec.release(); d_object.release(); d_asset.release(); d_material.release();
  }
};

// update() and trace_rays() share per-renderer scratch (work counters, step counters, the stack spill area): launches that use it
// are ordered across streams by an event — the last user records one, a user on another stream waits for it first
struct ScratchOrder {
  hipEvent_t event = nullptr;       // not owned: a ring slot's frame_end or batch_done
  hipStream_t stream = nullptr;
  hipEvent_t batch_done = nullptr;
  int acquire(hipStream_t s) {
    if (event && stream != s) RT_HIP(hipStreamWaitEvent(s, event, 0));
    return HALA_OK;
  }
  void release() { if (batch_done) (void)hipEventDestroy(batch_done); }
};
// The scratch contract of a query batch's device form (ray batches, multi-hit, closest points, distance grids, occlusion, bakes), once:
// the work runs on the caller's stream, ordered behind the scratch's previous user, without a host synchronisation, and batch_done is
// recorded behind it for the next user.  hala_rt_renderer::batch(hip_stream) makes one; open() before the first launch or memset that
// touches the scratch, close() as the entry point's result.  A scope left open — an RT_HIP or RT_FAIL return in between — still records
// batch_done behind whatever the call queued, quietly: the call is failing already, and the message stays that of the first failure.
struct BatchScope {
  ScratchOrder& scratch;
  WorkCounters* work;
  hipStream_t s;
  bool opened = false;
  BatchScope(ScratchOrder& order, WorkCounters* counters, hipStream_t stream) : scratch(order), work(counters), s(stream) {}
  BatchScope(const BatchScope&) = delete;
  BatchScope& operator=(const BatchScope&) = delete;
  ~BatchScope() {
    if (!opened) return;
    if (!scratch.batch_done && hipEventCreateWithFlags(&scratch.batch_done, hipEventDisableTiming) != hipSuccess) { scratch.batch_done = nullptr; return; }
    if (hipEventRecord(scratch.batch_done, s) == hipSuccess) { scratch.event = scratch.batch_done; scratch.stream = s; }
  }
  int open() {
    if (scratch.acquire(s) != HALA_OK) return HALA_ERR;
    opened = true;
    return HALA_OK;
  }
  int reset_work() {
    RT_HIP(hipMemsetAsync(work, 0, sizeof(WorkCounters), s));
    return HALA_OK;
  }
  // refusal: a launcher found that its kernel fits no compute unit — said once the event is recorded, as the result
  int close(const char* refusal = nullptr) {
    opened = false;
    if (!scratch.batch_done) RT_HIP(hipEventCreateWithFlags(&scratch.batch_done, hipEventDisableTiming));
    RT_HIP(hipEventRecord(scratch.batch_done, s));
    scratch.event = scratch.batch_done; scratch.stream = s;
    if (refusal) RT_FAIL(refusal);
    RT_HIP(hipGetLastError());
    return HALA_OK;
  }
};

// multi-GPU exchange (C1 of SURVEY 2.1): one RCCL all-gather of the rank's tile buffer per AOV and frame, inside the library
struct ExchangeState {
  ncclComm_t comm = nullptr;
  bool comm_owned = false;
  int comm_rank = 0, comm_world = 1;
  hipStream_t stream = nullptr;
  DeviceArray<float4> stage[6], recv[6];
  hipEvent_t ev_rendered = nullptr, ev_staged = nullptr, ev_gathered = nullptr;
  uint32_t pending = 0;  // AOV mask of the collective in flight (hala_rt_tile_allgather_begin)
  void release() {
    if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
    for (hipEvent_t e : {ev_rendered, ev_staged, ev_gathered}) if (e) (void)hipEventDestroy(e);
    if (comm && comm_owned) { if (const RcclApi* api = rccl_api(nullptr)) (void)api->CommDestroy(comm); }
  }
};

// What a path slot holds: `paths` path slots (slot_count x batch_capacity), each with the mandatory per-path state and queue entries, the
// first-hit position and id records while wanted (RENDER_SPEC §13, §15) and one radiance sum per light group (§14).  Computed by
// hala_rt_renderer::path_shape() alone; a feature that adds a per-path array adds a field here and an array to WavefrontSet::fit
struct PathShape {
  size_t paths = 0;  // 0: nothing
  bool aov_pos = false, aov_ids = false;  // the 16-B first-hit position / id record of every path slot
  uint32_t groups = 0;                    // light groups: one radiance sum per path slot each
  bool operator==(const PathShape& o) const { return paths == o.paths && aov_pos == o.aov_pos && aov_ids == o.aov_ids && groups == o.groups; }
};
// The per-path state and the queues of one update in flight: everything indexed by path slot.  Each frame slot has one.
struct WavefrontSet {
  DeviceArray<P3> lr, le, alb, nrm;
  DeviceArray<P3> groups;       // shape.groups x path slots, group-major; light connections carry the group in the top bits of the slot word
  DeviceArray<float4> aov_pos;  // 16 B per path slot each, only while wanted
  DeviceArray<uint4> aov_ids;
  DeviceArray<hala_ray> rays[2];
  DeviceArray<float4> state[2];
  DeviceArray<hala_hit> hits;
  DeviceArray<uint32_t> perm;
  DeviceArray<ShadowEntry> shadow[2];
  PathShape shape;  // what the last successful fit gave it
  // Sizes every array for `want` and frees the optional ones it does not name.  Arrays that already have their size are kept as they are,
  // also when a later allocation fails: the caller then fits again to a shape it can have (a setter: without its feature, which only
  // frees) or releases the set (slot 1: all or nothing).
  hipError_t fit(const PathShape& want) {
    hipError_t e = hipSuccess;
    auto get = [&](auto& a, size_t count) { if (!count) a.release(); else if (e == hipSuccess) e = a.resize(count); };
    const size_t n = want.paths;
    shape = PathShape();
    get(lr, n); get(le, n); get(alb, n); get(nrm, n);
    for (int k = 0; k < 2; ++k) { get(rays[k], n); get(state[k], n); get(shadow[k], n); }
    get(hits, n); get(perm, n);
    get(aov_pos, want.aov_pos ? n : 0); get(aov_ids, want.aov_ids ? n : 0); get(groups, n * want.groups);
    if (e == hipSuccess) shape = want;
    return e;
  }
  void release() { (void)fit(PathShape()); }
  Queues queues() const { return Queues{{rays[0].ptr, rays[1].ptr}, {state[0].ptr, state[1].ptr}, hits.ptr, perm.ptr, {shadow[0].ptr, shadow[1].ptr}}; }
  void fill(PathState* ps) const {  // the pointers of a PathState that differ between the slots (an array that is off is null)
    ps->radiance = lr.ptr; ps->radiance_env = le.ptr; ps->albedo = alb.ptr; ps->normal = nrm.ptr;
    ps->aov_pos = aov_pos.ptr; ps->aov_ids = aov_ids.ptr; ps->groups = groups.ptr;
  }
};

// Two frame slots: consecutive updates are independent except for the order in which their samples are folded into the
// accumulated images, so untimed updates alternate between two slots and the start of one runs beside the end of the other (`lead`).  A
// slot owns what one update in flight needs: a stream, a stack spill area, the per-path state and the queues (`set`), and a control block
// (hala_rt_renderer::d_ctl[slot]).  An update waits for the previous use of its slot by stream order; between the slots there is one
// dependency: the resolve (and the Cryptomatte fold) of an update waits for `folded` of the update before it.  While slot 1 is open the
// renderer's stream has not waited for it: every entry point joins it first (ensure_device), except update and render.
// Slot 1's set is allocated when an update first finds slot 0 busy, and fitted again when it is found stale (pick_slot); LDS-staged trees
// never allocate it: their updates on slot 1 use slot 0's set.
struct FrameSlot {
  hipStream_t stream = nullptr;  // slot 0: hala_rt_renderer::stream, which the renderer creates and destroys; slot 1: owned here
  WavefrontSet set;
  DeviceArray<uint2> spill;      // stack spill area of the slot's traversal launches (slot 0's also serves hala_rt_trace_rays: ScratchOrder)
  hipEvent_t folded = nullptr;   // behind the resolve and the Cryptomatte fold of the slot's latest update
  hipEvent_t lead = nullptr;     // behind the shade kLeadBounces before the last of the slot's latest update: where the next update starts
  // not owned: the frame_end event of the slot's latest update, which lives in the statistics ring.  A ring entry is recorded again 16
  // updates later; by then its slot has run a newer update (updates alternate, and every serial one runs on slot 0, so no slot sits out
  // 16 updates while the other runs) and `end` has moved on — except slot 1's while slot 1 is unused, which is waited for only while
  // `open` (before the first join after slot 1's latest update) or as the end of the update before this one (`last` == 1: it is the
  // latest update's, recorded once since)
  hipEvent_t end = nullptr;
};
struct FrameSlots {
  uint32_t in_flight = 2;          // hala_rt_set_frames_in_flight: 1 = one slot, one stream
  FrameSlot slot[2];
  hipEvent_t forked = nullptr;     // the renderer's stream as the last join left it: where slot 1 starts again
  bool open = false;               // slot 1 holds work the renderer's stream has not waited for
  bool fork = true;                // the renderer's stream holds work slot 1 has not waited for
  bool second_failed = false;      // slot 1's set could not be had: one slot until the sets are sized again
  int last = 1;                    // slot of the latest update (the next overlapped one takes the other)
  unsigned long long second_updates = 0;  // updates that ran on slot 1 (hala_rt_frames_in_flight_info)
  int last_folded = -1;            // slot whose `folded` is the latest
  int join(hipStream_t renderer_stream) {
    if (open) RT_HIP(hipStreamWaitEvent(renderer_stream, slot[1].end, 0));
    open = false; fork = true;
    return HALA_OK;
  }
  void release() {  // the events and slot 1's stream; slot 0's stream is the renderer's, `end` the statistics ring's
    for (hipEvent_t e : {slot[0].folded, slot[1].folded, slot[0].lead, slot[1].lead, forked}) if (e) (void)hipEventDestroy(e);
    if (slot[1].stream) (void)hipStreamDestroy(slot[1].stream);
  }
};

// shutter motion blur (RENDER_SPEC §18; hala_rt_set_shutter, hala_rt_set_*_keys).  `rec` is what the setters recorded (edits), `act` what the last hala_rt_refit applied: the update path only reads `act`.
struct ShutterState {
  ShutterKeys rec, act;
  uint32_t step = kShutterNoStep;  // the step the scene stands at
  float time = 0.0f;
  unsigned long long steps = 0;    // steps performed since create
  // the recorded node transforms and materials as the last refit found them: what a step fits to (RefitInputs), so that edits recorded
  // since do not ride along with it
  std::vector<Mat4> locals;
  std::vector<hala_material_desc> materials;
  std::vector<uint32_t> stale;     // primitives whose arena range the next refit uploads again from the host copy
  DeviceArray<uint32_t> d_flags;   // one overflow word per launch of k_shutter_lerp
  void off() { rec = ShutterKeys(); act = ShutterKeys(); step = kShutterNoStep; time = 0.0f; locals.clear(); materials.clear(); stale.clear(); }
};

// The instance levels of a two-level tree built on the GPU (hala_rt_build_options::instance_levels = 1; bvh_instances.hip): what survives
// between refits, so that a refit allocates nothing.  Everything releases itself.
struct InstanceLevels {
  uint32_t requested = 0;  // hala_rt_build_options::instance_levels as last set
  uint32_t mode = 0;       // as the last commit applied it: 0 built on the host (bvh_tlas.cpp), 1 on the GPU
  BuildOptions opt;        // the builder the commit chose: what the arena is sized for
  uint32_t items = 0, world_item = 0;  // items of the levels; 1: the first one is the world tree's
  DeviceArray<char> arena;             // all a build carves (item boxes, hierarchy, collapse), sized from the item count
  DeviceArray<InstItem> d_items;       // per item: its instance and its tree — a pose does not change them
  DeviceArray<InstTree> d_trees;       // per tree below the levels: where it starts, its bounds, need and depth
  std::vector<InstTree> trees;         // what d_trees holds
  bool refs_on_host = true;            // hala_rt_renderer::inst_refs holds what d_inst_refs holds (a GPU build only writes the latter)
  void release() { arena.release(); d_items.release(); d_trees.release(); trees.clear(); items = world_item = 0; refs_on_host = true; }
};

// node batches (RENDER_SPEC §20; hala_rt_bind_nodes, hala_rt_refit_nodes): the bound set, what the bind-time analysis found, the device
// tables of the kernels in node_batch.hip, and the two flags that keep host and device copies honest.  `mirror_stale`: a device-path call
// moved the world transforms on the device only — HostNode::world, HostScene::instances[].transform and instance_3x4 lag behind until
// hala_rt_renderer::sync_host_mirror recomputes them from the locals (which the call keeps current).  `tables_current`: d_locals / d_worlds
// hold what the trees stand at; every host refit clears it (refit_geometry), the next device-path call uploads them again.  Never both stale.
struct NodeBatchState {
  std::vector<uint32_t> bound;          // node indices in the bound order; empty: nothing bound
  bool analysed = false;                // the tables below belong to the trees as they stand (build_bvh clears it)
  std::vector<uint32_t> level_first;    // [levels + 1] into d_levels
  uint32_t affected_nodes = 0, affected_instances = 0;
  bool moves_camera_or_light = false;   // a camera or a light hangs at or below a bound node
  bool moves_flattened = false;         // two-level trees: an affected instance lies in the world tree
  DeviceArray<uint32_t> d_bound, d_mismatch;
  DeviceArray<NodeBatchNode> d_levels;
  DeviceArray<NodeBatchInst> d_insts;
  DeviceArray<float> d_locals, d_worlds, d_in;  // 16 floats per node / per node / per bound node (host input staged)
  float* h_stage = nullptr;             // pinned, 16 floats per bound node: host input on its way up, device input on its way down
  uint32_t* h_word = nullptr;           // pinned: the classification word as the call's one look found it
  bool tables_current = false, mirror_stale = false;
  uint32_t last_path = 0, last_reason = 0;
  unsigned long long device_refits = 0, host_refits = 0;
  uint32_t levels() const { return level_first.empty() ? 0u : (uint32_t)level_first.size() - 1u; }
  void release() {  // drops the binding; the counters are the renderer's (the caller has made the host mirror current)
    bound.clear(); analysed = false; level_first.clear(); affected_nodes = affected_instances = 0;
    moves_camera_or_light = moves_flattened = false;
    d_bound.release(); d_mismatch.release(); d_levels.release(); d_insts.release(); d_locals.release(); d_worlds.release(); d_in.release();
    if (h_stage) (void)hipHostFree(h_stage);
    if (h_word) (void)hipHostFree(h_word);
    h_stage = nullptr; h_word = nullptr;
    tables_current = false; mirror_stale = false;
  }
};

// tree quality and the refit policy (RENDER_SPEC §4.6; hala_rt_set_refit_policy, hala_rt_get_tree_quality).  `trees` is empty while the
// policy is off or nothing is committed; otherwise one entry per measured tree in the order of hala_rt_renderer::trees.
struct QualityState {
  uint32_t mode = 0;
  float max_inflation = 0.0f;
  std::vector<hala_tree_quality> trees;
  unsigned long long refits_measured = 0, trees_rebuilt = 0;
  DeviceArray<unsigned long long> d_out;  // three words per tree (launch_tree_cost)
  DeviceArray<unsigned long long> d_partials;  // its scratch, shared by the launches of one measurement
  unsigned long long* h_out = nullptr;    // pinned, as many words: the copy back needs no staging
  size_t h_words = 0;
  ~QualityState() { if (h_out) (void)hipHostFree(h_out); }
};

enum class Changed { Commit, Refit, Views, Aovs };  // hala_rt_renderer::invalidate

}  // namespace rt

#pragma GCC visibility pop

using namespace rt;  // (every unit that includes this header is written inside the library's namespace)

struct hala_rt_renderer {
  std::string name;
  uint32_t width = 0, height = 0;
  int device = 0;
  uint32_t max_depth = 0, rr_depth = 0;
  bool enable_tonemap = false, enable_aces = false, use_simple_aces = false;
  uint64_t max_frames = 0;
  hipStream_t stream = nullptr;  // the renderer's stream, which is frame slot 0's (slots.slot[0].stream)
  uint32_t cu_count = 256;

  float ground[4] = {1.0f, 1.0f, 1.0f, 1.0f};  // src/rt_renderer.rs:799
  float sky[4] = {0.5f, 0.7f, 1.0f, 1.0f};     // :800
  float env_intensity = 1.0f, exposure = 1.0f, env_rotation = 0.0f;  // :798-803

  uint32_t n_raygen = 0, n_miss = 0, n_callable = 0, n_hit = 0;
  DeviceArray<uint8_t> blue_noise;
  uint32_t blue_w = 0, blue_h = 0;

  bool has_scene = false, committed = false;
  HostScene hs;
  DeviceArray<hala_vertex> d_vertices;
  DeviceArray<uint32_t> d_indices;
  std::vector<size_t> prim_vertex_offset, prim_index_offset;
  hala_vertex* arena(uint32_t prim) const { return d_vertices.ptr + prim_vertex_offset[prim]; }  // the primitive's range of the vertex arena
  DeviceArray<hala_gpu_camera> d_cameras;
  DeviceArray<hala_gpu_light> d_lights;
  DeviceArray<hala_gpu_material> d_materials;
  DeviceArray<uint8_t> d_material_kind;
  std::vector<uint8_t> material_kind;  // host copy: a refit restamps the triangles when an edit changed a material's shading kind
  bool shade_sort = false, simple_materials = false, scatter_media = false;
  DeviceArray<hala_gpu_mesh_data> d_instances;
  DeviceArray<uint32_t> d_inst_first_tri;
  DeviceArray<float4> d_tex_arena;
  DeviceArray<uint32_t> d_tex_arena8;  // 8-bit images: RGBA bytes, tiled 4x4 (RENDER_SPEC 7.4)
  DeviceArray<float> d_srgb_lut, d_srgb_thr;
  DeviceArray<TexDesc> d_textures;
  std::vector<TexDesc> host_textures;
  BundleState bundles;

  // The scene's trees as a whole: what the readers outside the builder want of them (configure_traversal, view(), hala_rt_get_bvh_info,
  // rt_post.hip) and the build options (hala_rt_set_build_options), which every tree and the instance levels are built by
  struct TreeTotals {
    uint32_t node_count = 0, tri_count = 0;  // of the node / triangle arrays (two-level: the reserved ranges included)
    uint32_t max_depth = 0, stack_need = 0;  // from the root, through the instance levels
    float scene_min[3] = {}, scene_max[3] = {};
    BuildOptions opt;
  } bvh;
  // Every tree of the scene lives in `trees`, as a sub-range of the node / triangle / shading-record arrays: [0] the world-space tree
  // over the triangles of all instances that are NOT instanced (if any), then one object-space tree per instanced primitive.  A scene in
  // which some primitive is referenced by several instances is two-level (RENDER_SPEC 4.5): its trees stand behind the instance levels
  // (the first tlas_capacity nodes), which are rebuilt whenever a node moves (on the host, or on the GPU: `levels`).  Any other scene is
  // one-level: one world tree at node 0 and triangle 0 that holds every instance and reads the scene's own instance tables (d_instances,
  // d_inst_first_tri) in place of the four below.
  struct Tree {
    BvhBuffers b{};
    uint32_t node_off = 0, tri_off = 0, node_cap = 0;
    bool object_space = false;
    uint32_t prim = 0;                      // object_space: the primitive (index into hs.prims)
    std::vector<uint32_t> insts;            // world tree: the instances it holds, in instance order
    DeviceArray<hala_gpu_mesh_data> d_md;
    DeviceArray<uint32_t> d_first, d_gid, d_inst;
    ~Tree() { if (b.topology) bvh_free_topology(b.topology); }
  };
  std::vector<std::unique_ptr<Tree>> trees;
  bool two_level = false;
  // the world tree of a two-level scene, which has instance tables of its own; null: every instance is instanced, or the scene is one-level
  Tree* world_tree() const { return two_level && !trees.empty() && !trees[0]->object_space ? trees[0].get() : nullptr; }
  uint32_t instancing_mode = 0;            // hala_rt_build_options::instancing: 0 automatic (by size), 1 never (everything flattened), 2 by the rule of RENDER_SPEC 4.5
  std::vector<uint8_t> inst_instanced;     // per instance: intersected in object space
  std::vector<int32_t> prim_tree;          // per primitive: index into trees, -1
  uint32_t tlas_capacity = 0, tlas_nodes = 0, stored_tris = 0;
  std::vector<InstRef> inst_refs;          // (levels.refs_on_host tells whether its contents are current)
  DeviceArray<InstRef> d_inst_refs;
  InstanceLevels levels;
  DeviceArray<InstInfo> d_inst_info;
  DeviceArray<Tri> d_tris_by_id, d_tris;
  DeviceArray<Tri> d_tris_any;
  DeviceArray<ShadeTri> d_shade_tris;
  DeviceArray<BvhNode4> d_nodes;
  uint32_t lds_nodes = 0, lds_tris = 0;
  bool staged = false;  // whole BVH staged in LDS by the traversal kernels
  uint32_t leaf_max_built = 0;
  float ray_eps = 0.0f;
  LaunchCfg lcfg{};  // (spill: frame slot 0's area)
  uint32_t fuse_mode = 1;  // hala_rt_set_pass_fusion: 0 never, 1 untimed updates, 2 always (shadow passes of bounce d + closest-hit pass of bounce d + 1 in one launch)

  bool has_env = false;
  uint32_t env_w = 0, env_h = 0;
  DeviceArray<float4> d_env;
  DeviceArray<float> d_env_total, d_marginal, d_conditional;
  float env_total_sum = 0.0f;

  // tile shard (RENDER_SPEC §9)
  uint32_t real_pixels = 0;  // pixels among the rank's slot_count slots that exist in the frame
  uint32_t rank = 0, world = 1, tile_size = 32, tiles_x = 0, tiles_y = 0, tiles_per_rank = 0, perm_a_inv = 0, perm_b = 7;
  uint32_t slot_count = 0;      // pixel slots of this rank
  uint32_t blocks_x = 0;        // world == 1: 8 x 8 pixel blocks per row of blocks (hala_types.h: kPixelBlock)
  // pixels of this rank's image buffers: its tile slots when sharded, the row-major frame otherwise (whose path slots may hold padding)
  size_t image_pixels() const { return world <= 1 ? (size_t)width * height : (size_t)slot_count; }
  uint32_t batch_capacity = 1;  // paths per pixel slot the wavefront buffers can hold in flight: samples x views (hala_rt_update_batch)
  // views (RENDER_SPEC §12): the packed camera of each; view v's images follow view 0's in img_local, image_pixels() apart
  std::vector<uint32_t> views{0u};
  DeviceArray<ViewConst> d_views;  // what the kernels read when views.size() > 1 (rebuilt when a camera's yfov changes)
  std::vector<ViewConst> views_uploaded;
  uint32_t view_count() const { return (uint32_t)views.size(); }
  size_t image_alloc() const { return (size_t)slot_count + (size_t)(view_count() - 1) * image_pixels(); }  // view 0 keeps its slot_count

  DeviceArray<float4> img_local[6];  // accum, albedo, normal, final, position, ids (slot order); 4 and 5 only while that AOV is on
  DeviceArray<float4> img_full[6];   // row-major, only after scatter_gathered_tiles (world > 1)
  bool full_valid[6] = {false, false, false, false, false, false};
  // first-hit AOVs (RENDER_SPEC §13): bit 0 position (image 4), bit 1 ids (image 5); hala_rt_set_aovs
  uint32_t aov_mask = 0;
  bool has_image(int which) const { return which >= 0 && (which < 4 || (which < 6 && ((aov_mask >> (which - 4)) & 1u))); }
  DeviceArray<uint32_t> d_inst_node, d_light_node;  // per instance / per light: the scene node it came from
  LightGroupState groups;
  CryptoState crypto;
  bool wants_ids() const { return (aov_mask & 2u) || crypto.mask; }
  DenoiseBuffers denoise;      // RENDER_SPEC 10: allocated by the first hala_rt_denoise
  bool denoised = false;       // denoise.out holds a result
  AdaptiveState adaptive;      // RENDER_SPEC 11: allocated by the first hala_rt_set_adaptive_sampling that enables it
  TemporalState temporal;      // RENDER_SPEC 16: allocated by hala_rt_set_temporal
  DeformState deform;          // RENDER_SPEC 17: one deformer per primitive (hala_rt_set_deformer)
  ShutterState shutter;        // RENDER_SPEC 18: keys and shutter (hala_rt_set_shutter)
  RigState rig;                // RENDER_SPEC 19: the rig whose bindings are deformers here (hala_rt_set_rig)
  NodeBatchState nodes;        // RENDER_SPEC 20: the bound node set (hala_rt_bind_nodes)
  QualityState quality;        // RENDER_SPEC 4.6: the refit policy and what it measured (hala_rt_set_refit_policy)
  DeviceArray<Control> d_ctl;  // one per frame slot
  DeviceArray<WorkCounters> d_batch_work;
  // hala_rt_trace_rays, RENDER_SPEC 4.2: the caller's batch with far origins re-based, and how far each was moved (grown on demand)
  DeviceArray<hala_ray> d_batch_rays;
  DeviceArray<float> d_batch_moved;
  // hala_rt_distance_grid, RENDER_SPEC 4.9: the rows' crossing bits of a signed grid (grown on demand)
  DeviceArray<uint32_t> d_grid_bits;
  // hala_rt_occlusion, RENDER_SPEC 4.10: the mask words of a batch whose caller wants none (grown on demand)
  DeviceArray<uint32_t> d_occlusion_masks;
  // hala_rt_bake_samples / hala_rt_bake_occlusion, RENDER_SPEC 4.11 (grown on demand): the owner map (tiled 8 x 8) and its blocks' ownership
  // words, the per-triangle block counts with their prefix sum and its scratch, and the sample buffer of a baked occlusion map
  DeviceArray<uint32_t> d_bake_owner;
  DeviceArray<unsigned long long> d_bake_counts, d_bake_offsets, d_bake_block_bits;
  DeviceArray<uint8_t> d_bake_scan;
  DeviceArray<hala_occlusion_sample> d_bake_samples;
  // hala_rt_bake_atlas_*, RENDER_SPEC 4.12 (grown on demand): the chart of every instance, and the owned-texel list of a baked atlas with
  // the per-block counts and offsets it is built from
  DeviceArray<BakeChartDev> d_bake_charts;
  DeviceArray<uint32_t> d_bake_list, d_bake_list_counts, d_bake_list_offsets;
  // hala_rt_bake_transfer, RENDER_SPEC 4.13 (grown on demand): the target ranges of a call that has more than two
  DeviceArray<uint2> d_bake_targets;

  uint64_t total_frames = 0;
  bool counting = false;
  hala_global_uniform last_uniform{};
  TraceEvents ring[kStatRing];
  int ring_pos = 0;
  // recorded by the edit entry points, read and cleared by hala_rt_refit alone (a step of the shutter passes its own: RefitInputs)
  bool vertices_dirty = false;       // the vertex arena changed since the tree was fitted to it
  bool materials_dirty_any = false;  // a material edit touched an opacity-0 material (old or new)
  bool nodes_dirty = false;          // a node's local transform was written outside hala_rt_refit_nodes (which then takes the host path)
  bool materials_dirty = false;      // ... or a material was
  bool build_options_dirty = false;  // hala_rt_set_build_options since the trees were built or refitted: a refit may rebuild by them
  bool any_invisible = false;   // the scene has invisible or translucent materials: the any-hit launches traverse d_tris_any (RENDER_SPEC 7.1d)
  bool any_translucent = false; // ... translucent ones: the ALPHA variants of the any-hit kernels
  DeviceArray<uint8_t> d_material_any_class;
  std::vector<uint8_t> material_any_class;
  uint32_t launch_event_period = 0;  // per-launch timing events on every n-th update (hala_rt_set_launch_timing_period; 0: none)
  unsigned long long update_counter = 0;
  hala_rt_statistics stats{};
  ScratchOrder scratch;
  ExchangeState exchange;
  FrameSlots slots;

  ~hala_rt_renderer() {
    if (device >= 0) (void)hipSetDevice(device);
    for (const FrameSlot& s : slots.slot) if (s.stream) (void)hipStreamSynchronize(s.stream);
    for (auto& t : ring) {
      for (auto e : t.ev) (void)hipEventDestroy(e);
      if (t.frame_begin) (void)hipEventDestroy(t.frame_begin);
      if (t.frame_end) (void)hipEventDestroy(t.frame_end);
      if (t.host_totals) (void)hipHostFree(t.host_totals);
      if (t.host_sizes) (void)hipHostFree(t.host_sizes);
    }
    scratch.release();
    exchange.release();
    nodes.release();
    // images first, then everything else (src/rt_renderer.rs:620-633)
    for (auto& i : img_local) i.release();
    for (auto& i : img_full) i.release();
    trees.clear();
    slots.release();
    if (stream) (void)hipStreamDestroy(stream);
  }

  SceneView view() const {
    SceneView sv{};
    sv.nodes = d_nodes.ptr; sv.tris = d_tris.ptr; sv.tris_any = any_invisible ? d_tris_any.ptr : d_tris.ptr; sv.tris_by_id = d_tris_by_id.ptr; sv.shade_tris = d_shade_tris.ptr;
    sv.inst_first_tri = d_inst_first_tri.ptr; sv.primitives = d_instances.ptr; sv.materials = d_materials.ptr; sv.material_kind = d_material_kind.ptr;
    sv.lights = d_lights.ptr; sv.cameras = d_cameras.ptr;
    sv.textures = d_textures.ptr; sv.tex_arena = d_tex_arena.ptr; sv.tex_arena8 = d_tex_arena8.ptr; sv.tex_lut = d_srgb_lut.ptr; sv.texture_count = (uint32_t)host_textures.size();
    if (!bundles.host.empty()) { sv.bundles = bundles.d_descs.ptr; sv.bundle_arena = bundles.d_arena.ptr; sv.material_bundle = bundles.d_material.ptr; }
    sv.shade_sort = shade_sort ? 1u : 0u; sv.simple_materials = simple_materials ? 1u : 0u; sv.scatter_media = scatter_media ? 1u : 0u; sv.any_translucent = any_translucent ? 1u : 0u;
    sv.env_pixels = reinterpret_cast<const float*>(d_env.ptr); sv.env_marginal = d_marginal.ptr; sv.env_conditional = d_conditional.ptr;
    sv.node_count = bvh.node_count; sv.tri_count = bvh.tri_count; sv.lds_nodes = lds_nodes; sv.lds_tris = lds_tris;
    sv.inst_refs = d_inst_refs.ptr; sv.inst_info = d_inst_info.ptr; sv.instance_count = (uint32_t)hs.instances.size(); sv.two_level = two_level ? 1u : 0u;
    sv.ray_eps = ray_eps;
    {  // RENDER_SPEC 4.2, far origins: from the bounds as they stand (a refit moves them, and the builders' pad with them)
      float amax = 0.0f;
      for (int k = 0; k < 3; ++k) {
        sv.box_min[k] = bvh.scene_min[k]; sv.box_max[k] = bvh.scene_max[k];
        amax = std::max(amax, std::max(std::fabs(bvh.scene_min[k]), std::fabs(bvh.scene_max[k])));
      }
      const float ex = bvh.scene_max[0] - bvh.scene_min[0], ey = bvh.scene_max[1] - bvh.scene_min[1], ez = bvh.scene_max[2] - bvh.scene_min[2];
      sv.far_limit = kRebaseK * amax;
      sv.box_diag = std::sqrt(std::fmaf(ez, ez, std::fmaf(ey, ey, ex * ex)));
    }
    sv.staged = staged ? 1u : 0u;
    return sv;
  }
  // the traversal launches of an update on frame slot `slot`: with the slot's spill area
  LaunchCfg launch_cfg(int slot) const {
    LaunchCfg lc = lcfg;
    if (lcfg.spill) lc.spill = slots.slot[slot].spill.ptr;
    return lc;
  }
  // the scratch scope of a query batch on the caller's stream (null: the renderer's own)
  BatchScope batch(void* hip_stream) { return BatchScope(scratch, d_batch_work.ptr, hip_stream ? static_cast<hipStream_t>(hip_stream) : stream); }
  // what a path slot holds with `capacity` paths per pixel slot in flight: the one place that says so
  PathShape path_shape(uint32_t capacity) const { return PathShape{(size_t)slot_count * capacity, (aov_mask & 1u) != 0u, wants_ids(), groups.count}; }
  PathShape path_shape() const { return path_shape(batch_capacity); }
  // Slot 0's set follows a setter that changed the shape (the setters have joined slot 1 and waited; slot 1's set catches up when an
  // update next wants it: pick_slot).  It fails only where the new shape adds an array: the setter then turns its feature off and fits again
  hipError_t fit_paths() { return slots.slot[0].set.fit(path_shape()); }
  Queues queues(int slot) const { return slots.slot[slot].set.queues(); }
  PathState path_state(int slot) const {
    PathState ps{};  // what the slots share: the node tables and the light groups' tables (null and 0 while the groups are off)
    ps.inst_node = d_inst_node.ptr; ps.light_node = d_light_node.ptr;
    ps.light_group = groups.d_light_group.ptr; ps.material_group = groups.d_material_group.ptr;
    ps.group_count = groups.count; ps.group_stride = groups.count ? (uint32_t)path_shape().paths : 0u; ps.env_group = groups.env_group;
    slots.slot[slot].set.fill(&ps);
    return ps;
  }

  // RENDER_SPEC §5 / §7.4 for packed camera `cam`: tan(yfov / 2) and the angular size of one pixel
  ViewConst view_const(uint32_t cam, float height) const {
    ViewConst v{};
    float sn = 0.0f, cs = 1.0f;
    if (cam < hs.cameras.size()) h_sincos_rad(0.5f * hs.cameras[cam].yfov, &sn, &cs);
    v.camera = cam;
    v.tan_half = sn / cs;
    v.pixel_spread = 2.0f * v.tan_half / height;
    return v;
  }
  FrameConst frame_const(const hala_global_uniform& u, uint32_t samples = 1) const {
    FrameConst fc{};
    fc.u = u;
    fc.aspect = u.resolution[0] / u.resolution[1];
    const ViewConst v0 = view_const(views[0], u.resolution[1]);
    fc.tan_half = v0.tan_half;
    fc.pixel_spread = v0.pixel_spread;
    fc.views = view_count();
    fc.view_pixels = (uint32_t)image_pixels();
    fc.view_table = fc.views > 1u ? d_views.ptr : nullptr;
    fc.width = width; fc.height = height;
    fc.tile_size = tile_size; fc.tiles_x = tiles_x; fc.tiles_y = tiles_y; fc.world = world; fc.rank = rank; fc.blocks_x = blocks_x;
    fc.tiles_per_rank = tiles_per_rank; fc.perm_a = perm_a_inv; fc.perm_b = perm_b;
    fc.pixel_slots = slot_count; fc.samples = samples; fc.slot_count = slot_count * samples * fc.views;
    if (adaptive.enabled) {  // RENDER_SPEC 11: slots for the active blocks only (one view)
      fc.block_list = adaptive.lists[adaptive.cur].ptr;
      fc.pixel_slots = adaptive.active_blocks * kPixelBlock * kPixelBlock;
      fc.slot_count = fc.pixel_slots * samples;
    }
    return fc;
  }

  void reset_accumulation() {  // statistics.reset() of the device-lost path (src/rt_renderer.rs:557)
    total_frames = 0;
    for (bool& v : full_valid) v = false;
    adaptive.restart(width * height);
    crypto.ready = false;
  }
  // frames folded into the pixels that are still traced (every pixel with adaptive sampling off)
  uint32_t rendered_frames() const { return (uint32_t)std::min(total_frames, max_frames); }

  // RENDER_SPEC §20: the host copies of the world transforms, made current again after device-path calls of hala_rt_refit_nodes — the
  // hierarchy and the instance records recomputed from the locals, which is what the device computed, bit for bit.  Every reader of
  // HostNode::world, HostScene::instances[].transform or instance_3x4 calls it first, and so does every writer of HostNode::local: the
  // locals must still be the ones the trees stand at when it runs.
  void sync_host_mirror() {
    if (!nodes.mirror_stale) return;
    hs.update_node_hierarchies(hs.locals());
    hs.pack_instance_transforms();
    nodes.mirror_stale = false;
  }

  // What a change makes stale, feature by feature; the caller restarts the accumulation.  A new feature hooks in here.
  void invalidate(Changed c) {
    // RENDER_SPEC §15: the next update hashes the committed scene's names
    if (c == Changed::Commit || c == Changed::Refit) crypto.tables = false;
    // RENDER_SPEC §16: after a commit instance and material indices mean something else, and the history is validated against images 4 and
    // 5; a refit packed the instance transforms and the cameras again, and view 0 may render another camera: only the table follows
    if (c == Changed::Commit || (c == Changed::Aovs && (aov_mask & 3u) != 3u)) temporal.drop_history();
    else if (c == Changed::Refit || c == Changed::Views) temporal.table_dirty = true;
    if (c == Changed::Views) groups.relit_valid = false;
  }
  // the renderer's output settings, as an update uploads them
  void output_settings(hala_global_uniform* u) const {
    u->exposure_value = exposure; u->enable_tonemap = enable_tonemap; u->enable_aces = enable_aces; u->use_simple_aces = use_simple_aces;
  }
};

#pragma GCC visibility push(hidden)
namespace rt {

// ---- what several units need of each other ----------------------------------------------------------------------------------------
// renderer.hip.  join = false: update and render only, which leave slot 1 running (FrameSlots)
int ensure_device(hala_rt_renderer* r, bool join = true);
int alloc_frame_buffers(hala_rt_renderer* r);
std::string file_stem(const char* path);
// rt_scene.hip
int upload_packed(hala_rt_renderer* r, bool geometry = true);
int upload_textures(hala_rt_renderer* r);
int update_texture_bundles(hala_rt_renderer* r, bool fresh);
// rt_trees.hip.  build_bvh: all trees anew from the packed scene, the instance levels, the traversal configuration, the quality baseline.
// attach_any_triangles, classify_instances: the records half of a refit (refit_geometry) runs them again to see what an edit changed.
// instancing_candidates: per instance, would classify_instances test its transform (hala_rt_refit_nodes runs that test on the device)
int build_bvh(hala_rt_renderer* r);
int attach_any_triangles(hala_rt_renderer* r);
void classify_instances(hala_rt_renderer* r, std::vector<uint8_t>* flags);
void instancing_candidates(const hala_rt_renderer* r, std::vector<uint8_t>* considered);
// The refit sequence: the trees `moved` (indices into hala_rt_renderer::trees) are fitted to what the device tables hold, measured and,
// with `policy` (RENDER_SPEC 4.6), rebuilt when due (*rebuilt: build_bvh ran, nothing is left to do); then the instance levels
// (two-level) and the traversal configuration.  published: the caller's kernels wrote the moved transforms into the trees' instance
// tables (hala_rt_refit_nodes), so nothing is uploaded and no field of Tree::b is set again — every edit that changes anything else a
// tree is published with takes that call's host path (rt_nodes.hip: host_reason).
int refit_trees(hala_rt_renderer* r, const std::vector<uint32_t>& moved, bool published, bool policy, bool* rebuilt);
// rt_deform.hip.  deform_pose: every (deformer, parameters) of `items` posed into the arena, on an idle stream -> HALA_OK; kDeformOverflow:
// a posed position is not finite, the arena is put back and synchronised, `overflowed` (where given) names the offending items, the
// message is set; HALA_ERR: a device error (or the refusal after one).  It keeps Deformer::applied / posed, the temporal marks and the
// launch counters; Deformer::pending and dirty are the callers'.  deform_refit: hala_rt_refit's list — the holders of `keyed` (by
// primitive: the shutter's state at the refit's time), every other dirty deformer and those of `again` with their pending parameters —
// and what becomes of dirty and pending; *moved: the arena changed.  deform_registered: is a deformer registered on the primitive
constexpr int kDeformOverflow = 2;
struct DeformPose { Deformer* d; const Deformer::Params* p; };
int deform_pose(hala_rt_renderer* r, const std::vector<DeformPose>& items, std::vector<size_t>* overflowed);
int deform_refit(hala_rt_renderer* r, const std::map<uint32_t, Deformer::Params>& keyed, const std::vector<uint32_t>& again, bool* moved);
bool deform_registered(const hala_rt_renderer* r, uint32_t prim);
// rt_scene.hip: hala_rt_refit without the restart — hierarchies, packed records, the trees that moved (refit_trees; all rebuilt when the
// instancing flags change) — fitted to what `in` names; it reads and clears nothing of what the caller recorded
struct RefitInputs {
  const std::vector<Mat4>& locals;                    // one per node
  const std::vector<hala_material_desc>& materials;
  bool arena_changed;                                 // the vertex arena changed since the tree was fitted
  bool opacity0_edit;                                 // a material edit touched an opacity-0 material
  bool policy = false;                                // RENDER_SPEC 4.6: hala_rt_refit's own call — measure what was refitted, rebuild if due
};
int refit_geometry(hala_rt_renderer* r, const RefitInputs& in);
// rt_shutter.hip (RENDER_SPEC §18).  shutter_refit: hala_rt_refit's geometry part with the recorded keys applied, the scene left at step
// 0; shutter_step: moves the scene to step `j` between two frames of one accumulation (update_impl, while the shutter is active)
int shutter_refit(hala_rt_renderer* r);
int shutter_step(hala_rt_renderer* r, uint32_t j);
// rt_cryptomatte.hip
int crypto_prepare(hala_rt_renderer* r);
// rt_tiles.hip
void compute_tiling(hala_rt_renderer* r);

// ---- shared by the units that answer query batches (rt_rays.hip, rt_queries.hip, rt_bake.hip) ---------------------------------------------
// The refusals they share.  one_level: what the feature calls itself, where it is built for one-level trees only
inline int check_committed(const hala_rt_renderer* r, const char* one_level = nullptr) {
  if (!r->committed) RT_FAIL("The top level acceleration structure is none!");  // src/rt_renderer.rs:284
  if (one_level && r->two_level) RT_FAIL(std::string(one_level) + " are not built for two-level trees: commit the scene flattened (instancing = 0).");
  return HALA_OK;
}
inline int check_occlusion_rays(uint32_t rays) {
  if (rays == 0 || rays > HALA_MAX_OCCLUSION_RAYS) RT_FAIL("The occlusion ray count must be 1.." + std::to_string(HALA_MAX_OCCLUSION_RAYS) + ".");
  return HALA_OK;
}
inline int check_occlusion_size(uint64_t samples, uint32_t rays, const char* too_large) {  // a ray's index is 32 bits
  if (samples * rays >= (1ull << 32)) RT_FAIL(too_large);
  return HALA_OK;
}
// The device twin of an optional host output array, for the host form of a call: `n` records where the host pointer is given, none (and a
// null device pointer) where it is not.  host_form below allocates the twins, makes the call and reads them back.
template <class T>
struct HostOut {
  T* host;
  size_t n;
  DeviceArray<T> dev;
  HostOut(T* host_ptr, size_t count) : host(host_ptr), n(count) {}
  hipError_t stage() { return host ? dev.resize(n) : hipSuccess; }
  hipError_t fetch(hipStream_t s) { return host ? hipMemcpyAsync(host, dev.ptr, n * sizeof(T), hipMemcpyDeviceToHost, s) : hipSuccess; }
  T* ptr() const { return host ? dev.ptr : nullptr; }
};
// The host form of a call whose device form `call` runs on `s`: stage the outputs, call, read them back, wait — the one place that waits.
// -> HALA_OK, or HALA_ERR with the message set (by `call`, where it refused)
template <class Call, class... Outs>
int host_form(hipStream_t s, Call call, Outs&... outs) {
  hipError_t e = hipSuccess;
  ((e = e == hipSuccess ? outs.stage() : e), ...);
  RT_HIP(e);
  if (call() != HALA_OK) return HALA_ERR;
  ((e = e == hipSuccess ? outs.fetch(s) : e), ...);
  RT_HIP(e);
  RT_HIP(hipStreamSynchronize(s));
  return HALA_OK;
}

// ---- shared by the units that edit and pose vertices (rt_scene.hip, rt_deform.hip, rt_shutter.hip, rt_rig.hip) ---------------------------
inline int find_primitive(hala_rt_renderer* r, uint32_t mesh_index, uint32_t primitive_index, uint32_t* prim) {
  if (mesh_index + 1u >= r->hs.mesh_first_prim.size() || mesh_index == 0xffffffffu) RT_FAIL("The mesh does not exist.");
  const uint32_t first = r->hs.mesh_first_prim[mesh_index], end = r->hs.mesh_first_prim[mesh_index + 1u];
  if (primitive_index >= end - first) RT_FAIL("The primitive does not exist.");
  *prim = first + primitive_index;
  return HALA_OK;
}
// RENDER_SPEC §16: no motion is known under a deformation; every instance of the primitive starts without history
inline void mark_no_history(hala_rt_renderer* r, uint32_t prim) {
  if (!r->temporal.enabled) return;
  for (size_t i = 0; i < r->hs.instance_prim.size() && i < r->temporal.inst_marked.size(); ++i)
    if (r->hs.instance_prim[i] == prim) { r->temporal.inst_marked[i] = 1; r->temporal.table_dirty = true; }
}
// Overflow words of a group of launches (k_deform, k_shutter_lerp: a launch sets its word to 1): `n` words of `words` are cleared,
// `launch(words.ptr)` queues the kernels on `s`, and where `flags` is given they are read back behind them (one copy, one wait) and
// *any says whether one is set.  -> HALA_OK, or HALA_ERR with the message set
template <class Launch>
int launch_flagged(DeviceArray<uint32_t>& words, size_t n, hipStream_t s, Launch launch, std::vector<uint32_t>* flags, bool* any) {
  RT_HIP(words.resize(n));
  RT_HIP(hipMemsetAsync(words.ptr, 0, n * 4, s));
  if (launch(words.ptr) != HALA_OK) return HALA_ERR;
  if (!flags) return HALA_OK;
  flags->resize(n);
  RT_HIP(hipMemcpyAsync(flags->data(), words.ptr, n * 4, hipMemcpyDeviceToHost, s));
  RT_HIP(hipStreamSynchronize(s));
  for (uint32_t f : *flags) *any = *any || f != 0u;
  return HALA_OK;
}

}  // namespace rt
#pragma GCC visibility pop
