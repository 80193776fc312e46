// kernels.h — host-callable launchers of the HIP kernels of libhalart.so.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "hala_types.h"

namespace rt {

struct LaunchCfg {
  uint32_t persistent_blocks;  // grid of the persistent traversal kernels
  uint2* spill;                // global stack spill area or nullptr (stack need <= kStackLds)
  uint32_t refill;             // a wave refills its idle lanes once this many are idle (64 = whole-wave batches)
  size_t smem;                 // dynamic LDS bytes of the traversal kernels: a staged BVH + traverse_fixed_lds_bytes
};

// The forms of tree the traversal kernels are built for, each with its own kernel variants: a large one-level tree, a one-level tree
// staged whole in LDS, a two-level tree (RENDER_SPEC 4.5)
enum class TreeForm { Large, Staged, TwoLevel };
inline TreeForm tree_form(const SceneView& sv) { return sv.staged ? TreeForm::Staged : (sv.two_level ? TreeForm::TwoLevel : TreeForm::Large); }

// trace_closest.hip (the traverse_* answers, the closest-hit launches, the RENDER_SPEC 4.2 pair) and trace_shadow.hip (the two shadow launches)
size_t traverse_fixed_lds_bytes(TreeForm tree);  // LDS bytes of one workgroup besides a staged BVH: per-lane stacks (+ leaf work lists)
uint32_t traverse_stack_lds_levels(TreeForm tree);  // stack entries kept in LDS
uint32_t traverse_max_leaf(TreeForm tree);  // largest leaf (triangles) the traversal variant accepts
uint32_t traverse_stack_spill_levels();  // deeper entries spilled to global scratch (8 B each, per lane)
uint32_t traverse_blocks_per_cu(size_t dynamic_lds_bytes, TreeForm tree);  // resident workgroups per CU (occupancy query)
void launch_trace_batch(const LaunchCfg& lc, const SceneView& sv, const hala_ray* rays, hala_hit* hits, const uint32_t* n_ptr,
                        uint32_t n_imm, WorkCounters* work, Control* ctl, bool any, bool count, bool account, hipStream_t s);
void launch_trace_shadow(const LaunchCfg& lc, const SceneView& sv, const Queues& q, const PathState& ps, Control* ctl, uint32_t depth,
                         uint32_t kind /* 0 light, 1 environment */, bool count, hipStream_t s);
// the last shadow pass of bounce `depth` and the closest-hit traversal of bounce depth + 1 as ONE persistent launch (false: not fusable)
bool launch_trace_shadow_then_batch(const LaunchCfg& lc, const SceneView& sv, const Queues& q, const PathState& ps, Control* ctl, uint32_t depth,
                                    uint32_t kinds /* bit 0 light, bit 1 environment connections */, bool with_closest, hipStream_t s);
void launch_trace_primary(const LaunchCfg& lc, const SceneView& sv, const FrameConst& fc, hala_hit* hits, WorkCounters* work, Control* ctl,
                          uint32_t n_account /* real paths among fc.slot_count */, bool count, bool far_camera /* RENDER_SPEC 4.2 */, hipStream_t s);
// RENDER_SPEC 4.2 around a caller's batch: out = the batch with far origins re-based, moved[i] = how far; then moved[i] back on the closest hits' t
void launch_rebase_batch(const SceneView& sv, const hala_ray* rays, hala_ray* out, float* moved, uint32_t n, hipStream_t s);
void launch_unbase_hits(hala_hit* hits, const float* moved, uint32_t n, hipStream_t s);
// trace_multi.hip — RENDER_SPEC 4.7: the k nearest hits of each of n rays, sorted, at hits[i * k ..]; counts (or null) gets the number found.
// The kernel has its own LDS size and occupancy; its grid never exceeds lc.persistent_blocks (the spill area).  false: it fits no compute unit.
bool launch_trace_multi(const LaunchCfg& lc, const SceneView& sv, uint32_t cu_count, const hala_ray* rays, hala_hit* hits, uint32_t* counts,
                        uint32_t n, uint32_t k, WorkCounters* work, hipStream_t s);
void launch_unbase_multi(hala_hit* hits, const float* moved, uint32_t n, uint32_t k, hipStream_t s);  // moved[i] back on every record of ray i
// closest_point.hip — RENDER_SPEC 4.8: the nearest surface point of each of n queries on a one-level tree (staged or large), at out[i].
// Launched like the multi-hit kernel (own LDS size and occupancy, a grid within lc.persistent_blocks).  counters (or null): 2 x uint64,
// node visits and triangle tests are added to them.  false: it fits no compute unit, or the tree is a two-level one.
bool launch_closest_point(const LaunchCfg& lc, const SceneView& sv, uint32_t cu_count, const hala_point_query* queries, hala_closest_point* out,
                          uint32_t n, WorkCounters* work, unsigned long long* counters, hipStream_t s);
// distance_grid.hip — RENDER_SPEC 4.9: the distance field of the scene on a voxel grid, on a one-level tree (staged or large).  Launched
// like the closest-point kernel.  launch_grid_rows leaves in `bits` (zeroed by the caller: ny * nz rows of `words` words) the suffix
// parities of every row's crossings; launch_distance_grid writes distance[nz][ny][nx] (and prim, or null) by method 1 (a voxel per lane)
// or 2 (a 4 x 4 x 4 brick per wave), and flips the sign of the voxels that `inside` (those bits, or null: unsigned) marks.  counters (or
// null): 6 x uint64, see hala_rt_distance_grid_counted.  false: the kernel fits no compute unit, or the tree is a two-level one.
struct GridView {
  float origin[3], spacing, band;
  uint32_t nx, ny, nz;
  uint32_t words;  // of a row's bit array: (nx + 1 + 31) / 32
};
bool launch_grid_rows(const LaunchCfg& lc, const SceneView& sv, uint32_t cu_count, const GridView& g, uint32_t* bits, WorkCounters* work,
                      unsigned long long* counters, hipStream_t s);
bool launch_distance_grid(const LaunchCfg& lc, const SceneView& sv, uint32_t cu_count, const GridView& g, uint32_t method, float* distance, uint32_t* prim,
                          const uint32_t* inside, WorkCounters* work, unsigned long long* counters, hipStream_t s);
// occlusion.hip — RENDER_SPEC 4.10: `rays` any-hit rays over the hemisphere of each of `count` samples (count * rays < 2^32), generated
// in the lanes that trace them; masks (count * ceil(rays / 32) words, zeroed by the caller) gets the occluded bits, out[i] the record.
// Launched like an any-hit batch of launch_trace_batch (sv.tris_any, lc's grid and LDS, the ALPHA variants for translucent materials), on
// every tree form; then one lane per sample reduces the masks.
void launch_trace_occlusion(const LaunchCfg& lc, const SceneView& sv, const hala_occlusion_sample* samples, hala_occlusion* out, uint32_t* masks,
                            uint32_t count, uint32_t rays, uint32_t seed, WorkCounters* work, hipStream_t s);
// bake.hip — RENDER_SPEC 4.11: the W x H bake map of one instance of a one-level scene.  launch_bake_samples clears the owner map, folds
// the instance's triangles in (count, prefix sum, one (triangle, 8 x 8 block) pair per wave step) and writes sample y * W + x (and its
// texel record, or null); launch_bake_dilate then fills the ownerless texels of `out` (the records of those samples) from the owner map
// the first call left in `sc`.  The scratch is the caller's: owner bake_owner_words() words (block_bits a 64th of that), counts and offsets tri_count + 1 entries
// each, scan_tmp bake_scan_bytes(tri_count) bytes.  Nothing is synchronised.
struct BakeView {
  uint32_t width, height, blocks_x, blocks_y;  // (blocks: filled in by the launchers)
  uint32_t first_tri, tri_count;               // the instance's range of global ids
  uint32_t flags, margin;
  float bias, reach;
};
struct BakeScratch {
  uint32_t* owner;
  unsigned long long *counts, *offsets;
  unsigned long long* block_bits;  // one word per 8 x 8 block of the owner map (the dilation's)
  void* scan_tmp;
  size_t scan_bytes;
};
size_t bake_owner_words(const BakeView& bv);
size_t bake_scan_bytes(uint32_t tri_count);
hipError_t launch_bake_samples(const SceneView& sv, uint32_t cu_count, const BakeView& bv, const BakeScratch& sc, hala_occlusion_sample* samples,
                               hala_bake_texel* texels, hipStream_t s);
void launch_bake_dilate(const BakeView& bv, const BakeScratch& sc, hala_occlusion* out, hala_bake_texel* texels, hipStream_t s, bool bits_ready = false);
// bake.hip — RENDER_SPEC 4.12: the atlas form.  `charts` has one entry per instance of the scene (charted = 0: the instance is not in the
// atlas); bv.first_tri / tri_count span the charted instances' ranges (the triangles of uncharted instances in between count no pairs) and
// bv.flags is not read: the flags are each chart's.  launch_bake_list turns the owner map launch_bake_samples_atlas left in `sc` into the
// list of owned texels — their row-major indices in block-major order at sc.list, their number at sc.list_offsets[blocks] — without a word
// to the host, leaves the ownership words in sc.block_bits (launch_bake_dilate: bits_ready) and writes the invalid record to every
// ownerless texel of `out`.  Scratch on top of the above: list W * H words, list_counts and list_offsets blocks + 1 words each, scan_tmp
// bake_list_scan_bytes(blocks) bytes.
struct BakeChartDev {
  float sx, sy, ox, oy;
  uint32_t flags, charted, pad0, pad1;
};  // 32 B
struct BakeListScratch {
  uint32_t *list, *list_counts, *list_offsets;
};
size_t bake_list_scan_bytes(size_t blocks);
hipError_t launch_bake_samples_atlas(const SceneView& sv, uint32_t cu_count, const BakeView& bv, const BakeScratch& sc, const BakeChartDev* charts,
                                     hala_occlusion_sample* samples, hala_bake_texel* texels, hipStream_t s);
hipError_t launch_bake_list(const BakeView& bv, const BakeScratch& sc, const BakeListScratch& ls, hala_occlusion* out, hipStream_t s);
// occlusion.hip — the listed form of launch_trace_occlusion: only the samples list[0 .. *count) are traced and resolved (out[list[c]]; the
// other records are not touched), *count read on the device (<= max_count, which sizes the resolve's grid and the masks: max_count *
// ceil(rays / 32) words, zeroed by the caller).  Stream and any-hit key of a ray are its sample's, not its list position's: the records
// are those of the unlisted pass.  One-level trees only.
void launch_trace_occlusion_listed(const LaunchCfg& lc, const SceneView& sv, const hala_occlusion_sample* samples, const uint32_t* list, const uint32_t* count,
                                   uint32_t max_count, hala_occlusion* out, uint32_t* masks, uint32_t rays, uint32_t seed, WorkCounters* work, hipStream_t s);
// trace_transfer.hip — RENDER_SPEC 4.13: texel i of a bake map (samples[i], as launch_bake_samples left it) projected from `front` ahead
// of its surface along -normal onto the triangles whose global ids lie in `targets`, t in (0, tmax); out[i] gets the whole 32-B record
// (the trace kernel its first half, then one lane per texel the normal and the height).  Launched like the multi-hit kernel (own LDS
// size and occupancy, a grid within lc.persistent_blocks), on one-level trees.  false: the kernel fits no compute unit, or the tree is
// a two-level one.
// The target table: merged, sorted, disjoint [lo, hi) ranges of global triangle ids.  Up to two ranges travel as kernel arguments (an
// unused one is [0, 0)); more are read from `table` (count entries of (lo, hi), device memory), which is then the only copy consulted.
// A concept of its own: nothing in it knows about bake maps.
struct TransferTargets {
  uint32_t count;
  uint32_t lo0, hi0, lo1, hi1;
  const uint2* table;
};
bool launch_trace_transfer(const LaunchCfg& lc, const SceneView& sv, uint32_t cu_count, const hala_occlusion_sample* samples, const TransferTargets& targets,
                           float front, float tmax, hala_bake_transfer_hit* out, uint32_t count, WorkCounters* work, hipStream_t s);
// bake.hip — the dilation of RENDER_SPEC 4.11 on the 32-B records of 4.13 (the ownership words are made here: no bits_ready)
void launch_bake_dilate_transfer(const BakeView& bv, const BakeScratch& sc, hala_bake_transfer_hit* out, hala_bake_texel* texels, hipStream_t s);
// shade.hip
void launch_shade(const FrameConst& fc, const SceneView& sv, const Queues& q, const PathState& ps, Control* ctl, uint32_t depth, hipStream_t s);
// resolve.hip
// pos / ids: the first-hit AOV images of RENDER_SPEC §13 (nullptr: off; both off: the kernel variant without them).  group_images: the
// light-group images of §14, group g at group_images + g * group_stride (read only while ps.groups is set: the GROUPS variants)
void launch_resolve(const FrameConst& fc, const PathState& ps, float4* accum, float4* albedo, float4* normal, float4* final_img, float4* pos,
                    uint4* ids, float4* group_images, size_t group_stride, hipStream_t s);
// RENDER_SPEC §14 relight: n pixels of the group images (group g at group_images + g * group_stride) -> linear R and tonemapped R * exposure
struct RelightScales { float s[kMaxLightGroups][3]; };
void launch_relight(const hala_global_uniform& u, const float4* group_images, size_t group_stride, uint32_t group_count, const RelightScales& sc,
                    uint32_t n, float4* linear, float4* toned, hipStream_t s);
void launch_scatter_tiles(const FrameConst& fc, const float4* gathered, float4* full, hipStream_t s);
void launch_sample_texture(const SceneView& sv, uint32_t tex, const float* uvl, uint32_t n, float4* out, hipStream_t s);

// variants.cpp — the variant ledger (hala_rt_variant_ledger): the families in the order of the entry point's `family`; the flags of each in the order of
// its launcher's dispatch call (variants.h).  false: no such family.  Per process; `reset` clears the family's launched mask after reading it.
enum : uint32_t { kFamilyTracePrimary, kFamilyTraceBatch, kFamilyTraceShadow, kFamilyTraceShadowThenBatch, kFamilyShade, kFamilyResolve, kVariantFamilies };
bool variant_ledger(uint32_t family, uint64_t* launched, uint64_t* built, bool reset);

// texture.hip — K8: one level of the mip chain (2x2 box filter over linear RGBA32F texels)
void launch_mip_downsample(const float4* src, uint32_t sw, uint32_t sh, float4* dst, uint32_t dw, uint32_t dh, hipStream_t s);
// 8-bit images: row-major bytes -> 4x4-tiled level 0; tiled level l - 1 -> tiled level l (decode, box filter, encode)
void launch_tile8(const uint32_t* src, uint32_t w, uint32_t h, uint32_t* dst, hipStream_t s);
void launch_mip_downsample8(const uint32_t* src, uint32_t sw, uint32_t sh, uint32_t* dst, uint32_t dw, uint32_t dh, uint32_t format, const float* lut,
                            const float* thr, hipStream_t s);
// texel bundles: one tiled 8-bit level -> lane `lane` of the bundle level of the same size (dst: its first 16-B texel)
void launch_bundle_interleave(const uint32_t* src, uint32_t w, uint32_t h, uint4* dst, uint32_t lane, hipStream_t s);

// bvh_build.hip (with bvh_sah.hip, bvh_ploc.hip) — K1/K3/K4: flatten instances to world space, build the hierarchy (SAH | PLOC | LBVH),
// collapse it to 4-wide nodes, pack them level by level; refit re-flattens and re-packs the kept topology
// How commit() builds the hierarchy (hala_rt_set_build_options; 0 = the default everywhere).  The driver fields only change HOW the
// host walks the rounds of a build, never the tree (tests/test_gpu_parity.py::test_ploc_drivers_build_the_same_tree).
struct BuildOptions {
  uint32_t builder = 0;              // 0 auto (full-sweep SAH from 4096 triangles, LBVH below) | 1 SAH | 2 PLOC | 3 LBVH
  uint32_t ploc_tail = 0;            // 0 / 1: the last PLOC rounds (<= 512 clusters) inside one workgroup | 2: every round its own launch
  uint32_t ploc_look_every = 0;      // PLOC rounds between two looks of the host at the device's counters (default 6)
  uint32_t collapse_look_every = 0;  // levels of the 4-wide collapse between two looks (default 8)
};
struct BvhBuffers {
  // inputs (device): the instances whose triangles this tree holds, in instance order
  const hala_gpu_mesh_data* primitives;  // per listed instance
  const uint32_t* inst_first_tri;        // [instance_count + 1] prefix of triangle counts WITHIN this tree
  uint32_t instance_count;
  uint32_t tri_count;
  // trees over a subset of the scene (RENDER_SPEC 4.5): null = the whole scene, flattened (triangle k of the tree has global id k)
  const uint32_t* gid_first = nullptr;   // per listed instance: global id of its first triangle
  const uint32_t* inst_index = nullptr;  // per listed instance: its index in the scene's instance list (kAbsent: shared by several)
  bool object_space = false;             // the tree of an instanced primitive: vertex positions as they are, triangle ids local
  // outputs (device, allocated by the caller)
  Tri* tris_by_id;         // [tri_count]
  Tri* tris;               // [tri_count] BVH order
  Tri* tris_any = nullptr; // [tri_count] BVH order: triangles of invisible materials degenerate, of translucent ones flagged (RENDER_SPEC 7.1d);
                           // null: the scene has neither
  const uint8_t* material_any_class = nullptr;  // per material: 0 blocks always, 1 invisible, 2 translucent (for tris_any)
  uint32_t material_count = 0;
  const uint8_t* material_kind = nullptr;       // per material: shading kind (hala_types.h: shade_kind_of), stamped into word 11 of the BVH-order triangles
  ShadeTri* shade_tris;    // [tri_count] global-id order
  BvhNode4* nodes;         // capacity >= max(tri_count - 1, 1)
  void* topology = nullptr;  // builder state kept for refit (freed with bvh_free_topology)
  BuildOptions opt;
  // results
  uint32_t node_count;
  uint32_t max_depth;    // levels of the emitted tree
  uint32_t stack_need;   // traversal stack entries a ray can need
  float scene_min[3], scene_max[3];
};
// Builds everything; returns "" on success or an error message.  Synchronises the stream before returning.
std::string bvh_build(BvhBuffers& b, uint32_t leaf_max, hipStream_t s);
// Re-flattens (instance transforms / vertices may have changed) and refits the existing topology bottom-up.
std::string bvh_refit(BvhBuffers& b, hipStream_t s);
// A tree built into a sub-range of the scene's node / triangle arrays numbers its nodes and triangles from 0: make its child references
// absolute (inner: += node_offset, leaf: first triangle += tri_offset).  After every bvh_build / bvh_refit of such a tree.
std::string bvh_relocate(BvhBuffers& b, uint32_t node_offset, uint32_t tri_offset, hipStream_t s);
void bvh_free_topology(void* topology);
// hala_rt_selftest_collapse (halart.h): the collapse of a build on a binary tree from host memory, already checked by the caller
struct CollapseSelftest {
  uint32_t n, leaf_max;
  const uint32_t *left, *right, *node_parent, *leaf_parent, *first, *last;
  const float *node_boxes, *leaf_boxes;
  float* costs;
  uint32_t *choices, *keep, *refs4, *node_count, *levels;
};
std::string collapse_selftest(const CollapseSelftest& job);
// hala_rt_selftest_hierarchy (halart.h): one hierarchy builder of a build on boxes from host memory, already checked by the caller;
// what it leaves is what collapse_selftest takes
struct HierarchySelftest {
  uint32_t n;
  const float* boxes;  // [n][6] by id
  float pad;
  uint32_t builder, ploc_tail, ploc_look_every;  // BuildOptions; builder 1 .. 3
  uint32_t *sorted_ids, *left, *right, *first, *last, *node_parent, *leaf_parent;
  float* node_boxes;
};
std::string hierarchy_selftest(const HierarchySelftest& job);

// bvh_quality.hip — the tree cost of RENDER_SPEC 4.6 of the tree of `node_count` nodes whose root is `root` (references may be absolute:
// only boxes, presence, the leaf bit and the leaf counts are read): out3[0] = node_q, out3[1] = tri_q, out3[2] = valid (all three 0 for
// an invalid tree; out3 is left alone when node_count is 0).  partials: kTreeCostPartialWords words of scratch, free again once the
// launches have run (calls on one stream may share it).  Nothing is synchronised.
constexpr uint32_t kTreeCostPartialWords = 2048;
void launch_tree_cost(const BvhNode4* root, uint32_t node_count, unsigned long long* partials, unsigned long long* out3, hipStream_t s);

// bvh_tlas.cpp — the instance levels of a two-level tree (RENDER_SPEC 4.5), built on the host.  An item is a world-space box with the
// child reference a node slot gets for it: an instance leaf (kInstLeafTag | InstRef index) or the root node of a subtree that needs no
// transform; `need` = traversal stack entries a ray can need behind it.  Returns the node count (nodes in breadth-first order, root 0).
struct TlasItem { float mn[3], mx[3]; uint32_t ref, need; };
uint32_t tlas_build(const std::vector<TlasItem>& items, std::vector<BvhNode4>& out, uint32_t* levels, uint32_t* stack_need);

// bvh_instances.hip — the same levels built on the GPU (hala_rt_build_options::instance_levels = 1): items, scene bounds, hierarchy
// (BuildOptions::builder as for triangles), collapse and level pack all run on the device, out of an arena the caller keeps.
// What the host knows of one tree below the instance levels, rewritten only after that tree was built or refitted
struct InstTree {
  uint32_t node_off, tri_off;  // its root node; its first shading record (= first stored triangle)
  uint32_t need, depth;        // traversal stack entries a ray can need in it; its levels
  float mn[3], mx[3];          // its exact bounds, in its own space
};
struct InstItem { uint32_t inst, tree; };  // instance (kAbsent: the item of the world-space tree, which comes first) and its tree
struct InstanceLevelsJob {
  uint32_t n, world_item;                // items; 1: item 0 is the world tree's
  const InstItem* items;                 // [n] device, written at commit
  const InstTree* trees;                 // device
  const hala_gpu_mesh_data* instances;   // the packed instances (object -> world), device
  const uint32_t* inst_first_tri;
  InstRef* inst_refs;                    // out [n - world_item]
  BvhNode4* nodes;                       // out, breadth-first, root 0
  uint32_t node_capacity;
  void* arena;                           // instance_levels_arena_bytes(n, opt) bytes, reused by every build
  size_t arena_bytes;
  BuildOptions opt;
  // results
  uint32_t node_count, levels;
  float scene_min[3], scene_max[3];      // RENDER_SPEC 4.5
};
size_t instance_levels_arena_bytes(uint32_t n, const BuildOptions& opt);
// "" or an error message.  Synchronises the stream before returning.
std::string instance_levels_build(InstanceLevelsJob& job, hipStream_t s);

// envmap.hip — A1: EnvMap::build_distribution_maps (src/envmap.rs:239-388) on the GPU
// d_rgba: W*H float4; outputs device pointers: total_sum[1], marginal[H], conditional[W*H]
std::string envmap_build_distribution(const float4* d_rgba, uint32_t width, uint32_t height, float* d_total_sum, float* d_marginal,
                                      float* d_conditional, hipStream_t s);

}  // namespace rt
