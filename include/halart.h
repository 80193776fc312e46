/*
 * halart.h — C ABI of libhalart.so, the MI355X-native replacement for the hot path of
 * hala-renderer's ray-tracing renderer (reference: src/rt_renderer.rs, src/raytracing_program.rs,
 * src/envmap.rs, src/scene/loader/gpu_uploader.rs).
 *
 * The reference has no FFI boundary of its own: its "operator API" is the public Rust surface
 * `HalaRenderer` / `HalaRayTracingProgram` / `cpu::HalaScene`.  Every export below is what an
 * `extern "C"` Rust shim with those names would bind to; the reference item each entry point
 * replaces is cited as file:line (relative to the reference checkout).
 *
 * Conventions (reference: src/error.rs:5-22 — every fallible method returns Result<_, HalaRendererError>):
 *   - every fallible function returns an int status: 0 = Ok, non-zero = Err; the message of the last
 *     error on the calling thread is returned by hala_last_error_message() (== HalaRendererError::message()).
 *   - nothing aborts or throws across the boundary.
 *   - one handle <-> one host thread <-> one GPU (the reference is !Send/!Sync: src/renderer.rs:44).
 *   - all pointers are plain host pointers unless the name says `_device`/`d_` (then a HIP device pointer).
 *   - the library REQUIRES a HIP device: there is no CPU execution path in it.
 */
#ifndef HALART_H
#define HALART_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HALA_OK 0
#define HALA_ERR 1

#define HALA_INVALID_INDEX 0xffffffffu /* u32::MAX "none" marker (src/scene/cpu/node.rs:23-25) */
#define HALA_MAX_CAMERA_COUNT 8        /* src/scene/loader/gpu_uploader.rs:39 */
#define HALA_MAX_LIGHT_COUNT 32        /* src/scene/loader/gpu_uploader.rs:40 */
#define HALA_MAX_MORPH_TARGETS 64      /* morph targets of one deformer (docs/RENDER_SPEC.md 17) */
#define HALA_MAX_JOINTS 256            /* joint matrices of one deformer's palette */

/* ------------------------------------------------------------------------------------------------
 * Byte-exact device records (what the reference's shaders read).  Sizes/offsets are static_asserted
 * in hala-renderer_amd/csrc/hala_types.h and checked from Python in tests/test_layouts.py.
 * ---------------------------------------------------------------------------------------------- */

/* src/scene/vertex.rs:2-9 — 44 B */
typedef struct hala_vertex {
  float position[3];
  float normal[3];
  float tangent[3];
  float tex_coord[2];
} hala_vertex;

/* src/scene/gpu/camera.rs:10-20 — 80 B, align 16 */
typedef struct hala_gpu_camera {
  float position[3]; float _pad0;
  float right[3];    float _pad1;
  float up[3];       float _pad2;
  float forward[3];
  float yfov;
  float focal_distance_or_xmag;
  float aperture_or_ymag;
  uint32_t type; /* 0 perspective, 1 orthographic */
  uint32_t _pad3;
} hala_gpu_camera;

/* src/scene/gpu/light.rs:7-32 — 80 B, align 16 */
typedef struct hala_gpu_light {
  float intensity[3]; float _pad0;
  float position[3];  float _pad1;
  float u[3];         float _pad2;
  float v[3];
  float radius;
  float area;
  uint32_t type; /* 0 point, 1 directional, 2 spot, 3 quad, 4 sphere (src/scene/cpu/light.rs:7-12) */
  uint32_t _pad3[2];
} hala_gpu_light;

/* light AABB, `HalaAABB` of the absent hala-gfx crate: fields min/max per gpu_uploader.rs:169-180 — 24 B */
typedef struct hala_aabb {
  float min[3];
  float max[3];
} hala_aabb;

/* src/scene/gpu/material.rs:6-48 — 144 B, align 16 */
typedef struct hala_gpu_material {
  /* HalaMedium, 32 B */
  float medium_color[3];
  float medium_density;
  float medium_anisotropy;
  uint32_t medium_type;
  float _medium_padding[2];

  float base_color[3];
  float opacity;
  float emission[3];
  float anisotropic;
  float metallic;
  float roughness;
  float subsurface;
  float specular_tint;
  float sheen;
  float sheen_tint;
  float clearcoat;
  float clearcoat_roughness;
  float clearcoat_tint[3];
  float specular_transmission;
  float ior;
  float ax;
  float ay;
  uint32_t base_color_map_index;
  uint32_t normal_map_index;
  uint32_t metallic_roughness_map_index;
  uint32_t emission_map_index;
  uint32_t type; /* 0 diffuse, 1 disney (src/scene/cpu/material.rs:7-9) */
} hala_gpu_material;

/* src/scene/gpu/mesh.rs:32-39 — 96 B (glam::Mat4 is 16-aligned) */
typedef struct hala_gpu_mesh_data {
  float transform[16]; /* column-major object->world */
  uint32_t material_index;
  uint32_t _pad0;
  uint64_t vertices; /* device address of this primitive's hala_vertex[] */
  uint64_t indices;  /* device address of this primitive's uint32_t[]    */
  uint64_t _pad1;
} hala_gpu_mesh_data;

/* src/rt_renderer.rs:44-65 — 112 B, filled per frame at :408-427 */
typedef struct hala_global_uniform {
  float ground_color[4];
  float sky_color[4];
  float resolution[2];
  uint32_t max_depth;
  uint32_t rr_depth;
  uint32_t frame_index;
  uint32_t camera_index;
  uint32_t env_type; /* 0 SKY, 1 MAP (src/rt_renderer.rs:24-28) */
  uint32_t env_map_width;
  uint32_t env_map_height;
  float env_total_sum;
  float env_rotation; /* degrees / 360 (src/rt_renderer.rs:420) */
  float env_intensity;
  float exposure_value;
  uint32_t enable_tonemap;
  uint32_t enable_aces;
  uint32_t use_simple_aces;
  uint32_t num_of_lights;
  uint32_t _pad[3];
} hala_global_uniform;

/* ------------------------------------------------------------------------------------------------
 * Borrowed view of cpu::HalaScene (src/scene/cpu/scene.rs:17-26).  The renderer copies what it
 * needs during hala_rt_set_scene; the caller keeps ownership (as with `&mut cpu::HalaScene`).
 * ---------------------------------------------------------------------------------------------- */

/* src/scene/cpu/node.rs:2-12.  world transforms are recomputed by the library exactly as
 * update_node_hierarchies does (src/scene/cpu/scene.rs:99-114): parents must precede children. */
typedef struct hala_node_desc {
  const char* name;
  int32_t parent;            /* -1 == None */
  float local_transform[16]; /* column-major glam::Mat4 */
  uint32_t mesh_index;       /* HALA_INVALID_INDEX == none */
  uint32_t camera_index;
  uint32_t light_index;
} hala_node_desc;

/* src/scene/cpu/mesh.rs:6-13 (meshlet fields are rasterizer-only and omitted) */
typedef struct hala_primitive_desc {
  const uint32_t* indices;
  uint32_t index_count;
  const hala_vertex* vertices;
  uint32_t vertex_count;
  uint32_t material_index;
} hala_primitive_desc;

typedef struct hala_mesh_desc {
  const hala_primitive_desc* primitives;
  uint32_t primitive_count;
} hala_mesh_desc;

/* src/scene/cpu/material.rs:24-50, :75-80 */
typedef struct hala_material_desc {
  uint32_t type; /* 0 DIFFUSE, 1 DISNEY; anything else is an error (from_u8 panics in the reference) */
  float base_color[3];
  float opacity;
  float emission[3];
  float anisotropic;
  float metallic;
  float roughness;
  float subsurface;
  float specular_tint;
  float sheen;
  float sheen_tint;
  float clearcoat;
  float clearcoat_roughness;
  float clearcoat_tint[3];
  float specular_transmission;
  float ior;
  uint32_t medium_type; /* 0 NONE, 1 ABSORB, 2 SCATTER, 3 EMISSIVE */
  float medium_color[3];
  float medium_density;
  float medium_anisotropy;
  uint32_t base_color_map_index;
  uint32_t emission_map_index;
  uint32_t normal_map_index;
  uint32_t metallic_roughness_map_index;
} hala_material_desc;

/* src/scene/cpu/light.rs:30-39 */
typedef struct hala_light_desc {
  float color[3];
  float intensity;
  uint32_t light_type; /* 0..4 */
  float param0;
  float param1;
} hala_light_desc;

/* src/scene/cpu/camera.rs:4-29 */
typedef struct hala_camera_desc {
  uint32_t type; /* 0 perspective, 1 orthographic */
  float aspect;
  float yfov;
  float znear;
  float zfar;
  float focal_distance;
  float aperture;
  float xmag;
  float ymag;
} hala_camera_desc;

/* src/scene/cpu/image_data.rs:14-20; format codes are this library's own small enum */
#define HALA_FORMAT_R8G8B8A8_UNORM 0
#define HALA_FORMAT_R8G8B8A8_SRGB 1        /* glTF 8-bit RGB(A) images (src/scene/loader/gltf_loader.rs:395-396) */
#define HALA_FORMAT_R32G32B32A32_SFLOAT 2
#define HALA_FORMAT_B8G8R8A8_UNORM 3       /* files loaded through cpu::HalaImageData: RGBA bytes tagged BGRA without
                                              a swizzle (src/scene/cpu/image_data.rs:39-43) — red and blue swap */
typedef struct hala_image_desc {
  uint32_t format;
  uint32_t width;
  uint32_t height;
  const void* data;
  size_t num_of_bytes;
} hala_image_desc;

typedef struct hala_index_pair {
  uint32_t key;
  uint32_t value;
} hala_index_pair;

typedef struct hala_scene_desc {
  const hala_node_desc* nodes;         uint32_t node_count;
  const hala_mesh_desc* meshes;        uint32_t mesh_count;
  const hala_material_desc* materials; uint32_t material_count;
  const hala_light_desc* lights;       uint32_t light_count;
  const hala_camera_desc* cameras;     uint32_t camera_count;
  const hala_index_pair* texture2image_mapping; uint32_t texture_count; /* BTreeMap<u32,u32>, ascending key */
  const hala_index_pair* image2data_mapping;    uint32_t image_count;
  const hala_image_desc* image_data;   uint32_t image_data_count;
} hala_scene_desc;

/* cpu::HalaScene::new (src/scene/cpu/scene.rs:40-55) + HalaGltfLoader::load (src/scene/loader/gltf_loader.rs:121-227): loads
 * a `.gltf` file (external or base64 buffers; PNG images) into an owned scene whose borrowed description is what
 * hala_rt_set_scene takes.  Error messages are the reference's ("Unsupported file ...", "No scene in glTF file ...",
 * "Read indices from mesh ... failed.", "Invalid material type.", "Unsupported image format.", ...). */
typedef struct hala_scene hala_scene;
int hala_scene_load_gltf(const char* path, hala_scene** out);
const hala_scene_desc* hala_scene_get_desc(const hala_scene* scene);
void hala_scene_free(hala_scene* scene);

/* ------------------------------------------------------------------------------------------------
 * The rig of a glTF file (docs/RENDER_SPEC.md 19; no reference equivalent): skins, morph targets and animation clips as plain C
 * arrays, with every index already a scene index (hala_scene_load_gltf renumbers the file's nodes breadth-first).  A host that has
 * its own parser fills the same struct.  Every count is 0 when the file has nothing to pose.
 * ---------------------------------------------------------------------------------------------- */
#define HALA_RIG_STEP 0u
#define HALA_RIG_LINEAR 1u
#define HALA_RIG_CUBICSPLINE 2u
#define HALA_RIG_TRANSLATION 0u
#define HALA_RIG_ROTATION 1u
#define HALA_RIG_SCALE 2u
#define HALA_RIG_WEIGHTS 3u
typedef struct hala_rig_node {
  int32_t parent;            /* scene node index, -1: none (parents precede children) */
  uint32_t is_matrix;        /* 1: the file gave a `matrix` (no clip may touch the node); 0: the TRS below */
  float local_transform[16]; /* as hala_node_desc::local_transform: what a node no clip touches keeps, byte for byte */
  float translation[3];
  float rotation[4];         /* x y z w */
  float scale[3];
} hala_rig_node; /* 112 B */
typedef struct hala_rig_skin {
  uint32_t joint_count;
  uint32_t reserved;
  const uint32_t* joints;             /* scene node indices */
  const float* inverse_bind_matrices; /* joint_count column-major 4 x 4; the identity where the file has none */
} hala_rig_skin; /* 24 B */
/* one primitive that has a skin or morph targets */
typedef struct hala_rig_binding {
  uint32_t mesh_index, primitive_index;
  uint32_t node;                       /* the scene node that instantiates the mesh (the first one, should there be several) */
  uint32_t node_count;                 /* how many nodes instantiate it: hala_rt_set_rig accepts 1 */
  uint32_t skin;                       /* of that node, or HALA_INVALID_INDEX */
  uint32_t vertex_count;
  uint32_t influence_sets;             /* JOINTS_n / WEIGHTS_n sets the file has; set 0 is read, the others are counted only */
  uint32_t target_count;
  const uint16_t* joints;              /* [vertex][4] (JOINTS_0), NULL without a skin */
  const float* weights;                /* [vertex][4] (WEIGHTS_0, as given) */
  const float* target_position_deltas; /* [target][vertex][3], as hala_deformer_desc takes them; NULL when target_count is 0 */
  const float* target_normal_deltas;   /* or NULL */
  const float* target_tangent_deltas;  /* or NULL */
  const float* default_weights;        /* target_count: the mesh's `weights`, or zeros */
  uint32_t weight_first;               /* where this binding's weights start in a packed pose (floats) */
  uint32_t palette_first;              /* where its palette starts in a packed pose (floats; 12 per joint) */
} hala_rig_binding; /* 88 B */
typedef struct hala_rig_sampler {
  const float* times;     /* key_count, finite and strictly increasing */
  const float* values;    /* key_count * width floats; CUBICSPLINE: key_count * 3 * width (in-tangent, value, out-tangent) */
  uint32_t key_count;     /* >= 1 */
  uint32_t interpolation; /* HALA_RIG_STEP / LINEAR / CUBICSPLINE */
  uint32_t width;         /* floats per value: 3, 4, or the target count */
  uint32_t reserved;
} hala_rig_sampler; /* 32 B */
typedef struct hala_rig_channel {
  uint32_t sampler; /* of the same clip */
  uint32_t node;    /* scene node index */
  uint32_t path;    /* HALA_RIG_TRANSLATION / ROTATION / SCALE / WEIGHTS */
  uint32_t reserved;
} hala_rig_channel; /* 16 B */
typedef struct hala_rig_clip {
  const char* name; /* "" when the file has none */
  const hala_rig_sampler* samplers;
  const hala_rig_channel* channels;
  uint32_t sampler_count, channel_count;
  float time_first, time_last; /* the first and last key time over the samplers its channels use (0, 0 without channels) */
} hala_rig_clip; /* 40 B */
typedef struct hala_rig_desc {
  uint32_t node_count;      /* the scene's node count, or 0 when there is nothing to pose */
  uint32_t gltf_node_count; /* length of node_of_gltf */
  const hala_rig_node* nodes;
  const uint32_t* node_of_gltf; /* glTF node index -> scene node index; HALA_INVALID_INDEX: in no scene */
  const hala_rig_skin* skins;
  const hala_rig_binding* bindings;
  const hala_rig_clip* clips;
  uint32_t skin_count, binding_count, clip_count;
  uint32_t weight_floats;  /* floats of a packed pose's weights: the sum of target_count over the bindings */
  uint32_t palette_floats; /* floats of a packed pose's palettes: 12 per joint of every skinned binding */
  uint32_t reserved;
} hala_rig_desc; /* 72 B */
/* The rig of a loaded file: borrowed, owned by the scene.  Loading fails ("... glTF rig ...") on a joint or channel node out of range,
 * an inverse-bind count that differs from the joint count, key times that are not finite or do not strictly increase, a sampler
 * output whose count does not match its input (3 per key for CUBICSPLINE), a `weights` channel on a node without a mesh or whose
 * width differs from the mesh's target count, primitives of one mesh with different target counts, target or joint accessors whose
 * count differs from the vertex count, and a channel on a node given as `matrix`. */
const hala_rig_desc* hala_scene_get_rig(const hala_scene* scene);
/* Evaluates clip `clip` at `time` on the host (RENDER_SPEC 19; float64, each result rounded once): the local transform of every
 * node (node_count * 16 floats, column-major), the morph weights of every binding (weight_floats) and the joint palette of every
 * binding (palette_floats; row-major 3 x 4 per joint, as hala_rt_update_deformer takes them), each output optional (NULL).
 * clip == HALA_INVALID_INDEX: the file's own pose.  Fails on a clip that does not exist, a time that is not finite, a malformed
 * description (an index out of range) and a mesh node whose world transform is singular.  Needs no renderer and no GPU. */
int hala_rig_sample_clip(const hala_rig_desc* rig, uint32_t clip, float time, float* locals, float* weights, float* palettes);

/* ------------------------------------------------------------------------------------------------
 * Errors
 * ---------------------------------------------------------------------------------------------- */
/* HalaRendererError::message() (src/error.rs:23) of the last failed call on this thread. */
const char* hala_last_error_message(void);

/* ------------------------------------------------------------------------------------------------
 * HalaRenderer (src/rt_renderer.rs:568-1353, trait src/renderer.rs:210-324)
 * ---------------------------------------------------------------------------------------------- */
typedef struct hala_rt_renderer hala_rt_renderer;

/* HalaRenderer::new (src/rt_renderer.rs:650-813).  Headless: width/height replace gpu_req.{width,height}
 * (:661-662), device_ordinal replaces the winit window/swapchain.  max_frames == 0 => u64::MAX (:774). */
int hala_rt_create(const char* name, uint32_t width, uint32_t height, int device_ordinal,
                   uint32_t max_depth, uint32_t rr_depth, int enable_tonemap, int enable_aces,
                   int use_simple_aces, uint64_t max_frames, hala_rt_renderer** out);
/* Drop order of src/rt_renderer.rs:620-633: images, then everything else. */
void hala_rt_destroy(hala_rt_renderer* r);

/* push_general_shader{,_with_file} (src/rt_renderer.rs:925-995) and push_hit_shaders{,_with_file}
 * (:1003-1112).  SPIR-V has no meaning for HIP kernels: the call is validated, recorded (so that
 * commit can enforce "at least one raygen shader was pushed" like the reference pipeline would) and
 * otherwise ignored.  stage: 0 raygen, 1 miss, 2 callable. */
int hala_rt_push_general_shader(hala_rt_renderer* r, const void* code, size_t code_size, int stage,
                                const char* debug_name);
int hala_rt_push_general_shader_with_file(hala_rt_renderer* r, const char* file_path, int stage,
                                          const char* debug_name);
int hala_rt_push_hit_shaders(hala_rt_renderer* r, const void* closest_hit, size_t closest_hit_size,
                             const void* any_hit, size_t any_hit_size, const void* intersection,
                             size_t intersection_size, const char* debug_name);
int hala_rt_push_hit_shaders_with_file(hala_rt_renderer* r, const char* closest_hit_path,
                                       const char* any_hit_path, const char* intersection_path,
                                       const char* debug_name);

/* load_blue_noise_texture (src/rt_renderer.rs:1117-1156).  Optional here (mandatory at commit in the
 * reference, :319).  The image is decoded, validated and uploaded like the reference does, and then IGNORED:
 * the built-in integrator draws every sample from a counter-based hash RNG keyed by (pixel id, frame index)
 * (docs/RENDER_SPEC.md 2.3), which is what makes a pixel's value independent of tiling, batching and ranks. */
int hala_rt_load_blue_noise_texture(hala_rt_renderer* r, const char* path); /* PNG / JPEG, like HalaImageData::new_with_file */
int hala_rt_load_blue_noise_pixels(hala_rt_renderer* r, const uint8_t* rgba8, uint32_t width,
                                   uint32_t height);

/* set_scene (src/rt_renderer.rs:1161-1178) -> HalaSceneGPUUploader::upload(.., false, false, true)
 * (src/scene/loader/gpu_uploader.rs:63-545, :774-967).  Refused (the reference would hand them to the driver unchecked): primitives
 * without a material, indices out of range, vertex positions that are not finite. */
int hala_rt_set_scene(hala_rt_renderer* r, const hala_scene_desc* scene);

/* set_envmap (src/rt_renderer.rs:1184-1195) -> EnvMap::new_with_file (src/envmap.rs:38-232).
 * _pixels takes the already decoded image (RGB or RGBA f32, row 0 = top) and applies the same
 * validation (NaN/Inf rejection :63-71), alpha := 1 repack (:72-89) and table build (:239-388);
 * _file decodes Radiance .hdr (RGBE), .pfm or OpenEXR (scanline or single-level tiled; NONE / RLE / ZIPS / ZIP / PIZ; half, float) itself and honours
 * ./out/<stem>.dist_cache (:90-142). */
int hala_rt_set_envmap_pixels(hala_rt_renderer* r, const float* pixels, uint32_t channels,
                              uint32_t width, uint32_t height, float rotation_degrees);
int hala_rt_set_envmap_file(hala_rt_renderer* r, const char* path, float rotation_degrees);

/* src/rt_renderer.rs:1199-1219 */
void hala_rt_set_ground_color(hala_rt_renderer* r, const float rgba[4]);
void hala_rt_set_sky_color(hala_rt_renderer* r, const float rgba[4]);
void hala_rt_set_env_intensity(hala_rt_renderer* r, float intensity);
void hala_rt_set_exposure_value(hala_rt_renderer* r, float exposure_value);

/* commit (src/rt_renderer.rs:136-379): fails with "The scene in GPU is none!" without a scene (:138).
 * Here it also flattens the instances to world space, builds the BVH on the GPU (the work the
 * reference hands to vkCmdBuildAccelerationStructuresKHR: gpu_uploader.rs:784-811, :937-959) and
 * allocates the wavefront queues. */
int hala_rt_commit(hala_rt_renderer* r);
/* How commit() builds the acceleration structure — the HalaAccelerationStructure build flags of gpu_uploader.rs:784-811 /
 * :937-959 (PREFER_FAST_TRACE there).  Every field: 0 = the default.  The *_look_every / ploc_tail fields only change how the host
 * drives the rounds of a build (test hooks: the tree is the same for every value).  Takes effect at the next commit. */
typedef struct hala_rt_build_options {
  uint32_t builder;             /* 0 auto: full-sweep SAH from 4096 triangles, LBVH below | 1 SAH (fast trace) | 2 PLOC (fast build) | 3 LBVH */
  uint32_t ploc_tail;           /* 0 / 1: the last PLOC rounds in one workgroup | 2: every round its own launch */
  uint32_t ploc_look_every;     /* PLOC rounds between two host looks at the device counters (default 6) */
  uint32_t collapse_look_every; /* levels of the 4-wide collapse between two host looks (default 8) */
  uint32_t instancing;          /* what becomes of a primitive that several instances reference (RENDER_SPEC 4.5; the reference's BLAS /
                                 * TLAS split, gpu_uploader.rs:782-815, :843-885, :937-959):
                                 *  2: two-level tree — the primitive gets ONE object-space tree, its instances are leaves of instance
                                 *     levels that are rebuilt on the host when a node moves; every instanced primitive is stored once;
                                 *  1: every instance is flattened to world space, one tree over all triangles: the faster tree on this
                                 *     hardware (configs[3]: 9.7 instead of 11.8 ms per frame), at the full triangle count in memory;
                                 *  0: automatic — 1 unless the flattened scene holds more than 2^26 triangles (about 15 GB of tree), then 2.
                                 * The two forms intersect instanced geometry in different spaces: images agree to rounding, not bit for bit;
                                 * hala_bvh_info::instance_ref_count tells which one a commit chose. */
  uint32_t texture_bundles;     /* texel bundles: the co-sized 8-bit maps of a material (at least two of base colour, normal, metallic-
                                 * roughness, emission; equal width and height) are also stored interleaved, 16 B per texel position, and
                                 * the shade kernels fetch all of them with one load per texel.  Not observable in any image (RENDER_SPEC
                                 * 7.4); costs 16 B per texel of every bundled tuple beside the textures themselves.
                                 *  0: automatic — on, unless the bundle memory cannot be had (then silently off);  1: off.
                                 * hala_rt_texture_bundle_info tells what a commit built. */
  uint32_t instance_levels;     /* where the instance levels of a two-level tree are built, at commit and again at every refit and shutter
                                 * step of such a scene (RENDER_SPEC 4.5 fixes their format, not their shape; images do not depend on it):
                                 *  0: on the host (one thread, full-sweep SAH over the instances);
                                 *  1: on the GPU, by the builder `builder` selects with instances in the place of triangles (automatic:
                                 *     LBVH below 4096 instances, full-sweep SAH from there).  A refit then allocates nothing.
                                 * Choose 1 from a few thousand instances (MI355X; profiles/instance_levels_timing.json: N instances of a
                                 * 1 280-triangle primitive; host build against GPU build, ms):
                                 *    N        commit         refit, one node moved   refit, all moved   1080p frame
                                 *    1 024    1.6 / 0.9      1.2 / 0.45              1.2 / 0.43         3.03 / 3.39
                                 *   16 384    39 / 4.0       38 / 3.8                39 / 3.5           4.35 / 4.40
                                 *  131 072    952 / 7.6      962 / 10.9              855 / 10.6         5.11 / 5.16
                                 * From 4096 instances, where the automatic builder is SAH, the GPU-built tree renders like the host's
                                 * (+0.05 ms, 1 %, with the automatic builder; +0.004 ms with builder = 1 on both sides; repeated host-tree
                                 * frames spread by 0.02 ms).  Below 4096 the automatic builder is LBVH: builds win from the smallest count
                                 * measured, but at 1 024 its tree renders 12 % slower than the host's; builder = 1 there gives the host's
                                 * frame time (2.86 / 2.85 ms) and a slower build than the host's (refit 1.8 against 1.2 ms), so small scenes
                                 * keep 0.  builder = 2 and 3 (PLOC, LBVH) build the levels fastest (131 072: refit 7.9 and 6.7 ms, most of
                                 * it the host's own work per instance) and render 38 % and 15 % slower there: for edits, not for stills. */
  uint32_t reserved[1];         /* must be 0 */
} hala_rt_build_options;
int hala_rt_set_build_options(hala_rt_renderer* r, const hala_rt_build_options* options);

/* update (src/rt_renderer.rs:387-471): pre_update bookkeeping (src/renderer.rs:266-281), the
 * `total_frames > max_frames` early-out (:394-396), the HalaGlobalUniform fill (:408-427) and one
 * trace_rays(width, height, 1) (:458-464) == one sample per pixel.  ui_fn is dropped. */
int hala_rt_update(hala_rt_renderer* r, double delta_time, uint32_t width, uint32_t height);
/* `frames` consecutive update() calls executed as ONE wavefront pass with `frames` paths per pixel in flight (in
 * chunks of at most 16).  Result, frame bookkeeping and max_frames behaviour are bit-identical to calling
 * hala_rt_update `frames` times; what changes is the launch count and the size of each launch (288 GB of HBM hold
 * the extra path state; the per-launch tail of the longest ray is amortised over `frames` times more rays). */
int hala_rt_update_batch(hala_rt_renderer* r, uint32_t frames);
/* render (src/rt_renderer.rs:475-502): no swapchain to present to.  Like submit_and_present_frame, which blocks only on the fence of
 * the swapchain image it is about to reuse, it bounds the updates in flight to two: it returns once the update BEFORE the latest has
 * finished.  Readers (read_image, save_images, get_statistics, wait_idle) wait for everything themselves. */
int hala_rt_render(hala_rt_renderer* r);
/* wait_idle (src/renderer.rs:251-256) */
int hala_rt_wait_idle(hala_rt_renderer* r);

/* save_images (src/rt_renderer.rs:1224-1352): <stem>_color.pfm (accum, tonemapped on the host exactly
 * as :1256-1316), <stem>_albedo.pfm, <stem>_normal.pfm; PFM layout of :1318-1334. */
int hala_rt_save_images(hala_rt_renderer* r, const char* path);

/* Test/bench access to what save_images reads back (:1239-1254): which = 0 accum, 1 albedo, 2 normal
 * (RGBA32F, 4*W*H floats, row 0 = top), 3 final (tonemapped RGBA32F the raygen stage writes, :688). */
int hala_rt_read_image(hala_rt_renderer* r, int which, float* dst_rgba32f);

/* Views (docs/RENDER_SPEC.md 12; no reference equivalent — the reference always renders camera 0, src/rt_renderer.rs:415).  Every
 * update renders one sample per pixel for each of `count` (1..8) views; view v uses packed camera camera_indices[v] (< 8; duplicates
 * render identical views) with that camera's own yfov.  The default is one view of camera 0.  The RNG is keyed by pixel and frame only,
 * so view v equals a single-view render of its camera bit for bit and the noise of the views is correlated.  Refused, with the renderer
 * left as it was: a null list, count 0 or > 8, an index >= 8, and count > 1 on a sharded renderer (world > 1) or with adaptive sampling
 * on (hala_rt_set_tile_shard and hala_rt_set_adaptive_sampling refuse the other order).  A successful call joins the tail of the last
 * update, sizes the images for count views (new views start at zero) and restarts the accumulation like hala_rt_commit.  An update
 * whose views name a camera the committed scene does not have fails before any device work.  Chunks of hala_rt_update_batch hold at
 * most 16 / count frames; statistics count every view (rays_primary_total grows by W*H*count per frame); camera_index of
 * hala_rt_get_global_uniform is view 0's camera.  read_image, save_images, hala_rt_denoise and the tile entry points act on view 0. */
int hala_rt_set_views(hala_rt_renderer* r, const uint32_t* camera_indices, uint32_t count);
/* read_image for view `view` (< count of hala_rt_set_views): waits like hala_rt_read_image.  Another view's PFMs or denoised image come
 * from hala_write_pfm and hala_denoise_images on what this returns. */
int hala_rt_read_view_image(hala_rt_renderer* r, uint32_t view, int which, float* dst_rgba32f);

/* First-hit AOVs (docs/RENDER_SPEC.md 13; no reference equivalent — there an application writes its own closest-hit and raygen shaders,
 * which this integrator validates and ignores).  mask bit 0 = image 4 `position`, bit 1 = image 5 `ids`; the default is 0.  The first
 * hit of a sample is its camera ray's nearest triangle or hittable light (QUAD, SPHERE): the surface whose albedo and normal go to
 * images 1 and 2.
 *   4 position (RGBA32F): the running mean, in frame order, of (P.xyz, 1) on a hit and (0, 0, 0, 0) on a miss, P = madd(d, t, o) of the
 *     camera ray.  .w is the pixel's coverage; xyz / w is the mean hit point of the samples that hit.
 *   5 ids (4 x uint32 per pixel in the same 16-B slots; read with read_image and reinterpret): the first hit of the sample of frame 0 of
 *     the accumulation, kept after that.  Triangle: (node, instance, material, global triangle id), the instance in the order of
 *     hala_rt_get_packed_primitives and the node it came from.  Light: (node of the light, 0xFFFFFFFF, 0xFFFFFFFF, 0x80000000 | light
 *     index).  Miss: all 0xFFFFFFFF.
 * They follow the tile layout, the views, adaptive sampling and update_batch like images 0-3.  Bits above 1 are refused with the
 * renderer left as it was.  A successful call joins the second frame slot, allocates or frees images 4 / 5 of every view and
 * 16 B per path slot each, and restarts the accumulation.  read_image, read_view_image, tile_buffer, the scatter and exchange entry
 * points take `which` 4 / 5 and the all-gather masks bits 4 / 5 while that AOV is on, and refuse them while it is off.  Not built:
 * save_images does not write them (hala_write_pfm does), no depth image (view depth follows from position and the camera), no
 * deep ids (coverage per id over every sample: hala_rt_set_cryptomatte), no motion vectors, no denoiser guided by position. */
int hala_rt_set_aovs(hala_rt_renderer* r, uint32_t mask);

/* Light groups (docs/RENDER_SPEC.md 14; no reference equivalent): the beauty image split by emitter, so that a converged frame can be
 * relit without rendering it again.  The sources are each packed light k (the order of hala_rt_get_packed_lights), the environment (SKY
 * or MAP) and each material m (its surface emission, emission map included, and the glow of its EMISSIVE medium).  The descriptor maps
 * every source to one group 0 .. group_count-1 (group_count 1..8); NULL turns the feature off, the default.  Images 0-5, statistics
 * and the RNG are the same with groups on or off.
 * Image g of a view is the running mean (in frame order, RGBA32F, alpha 1, laid out like accum) of S_g: the terms of RENDER_SPEC 6
 * whose source is in g, added in the order 6 adds them to L, plus Le (the environment connections) for the environment's group
 * when an environment map is set.  A non-finite S_g is replaced by 0 on its own.  Image g equals the accum image of the same renderer
 * on the isolated scene of g (every light outside g at intensity 0, env_intensity 0 unless the environment is in g, every material
 * outside g with emission 0 and, if its medium is EMISSIVE, medium colour 0) bit for bit, except in samples where a zeroed term is
 * non-finite (0 * inf).  The images follow the views, adaptive sampling (converged blocks keep theirs), update_batch (k frames equal k
 * updates) and two updates in flight like accum.
 * Refused, with the renderer left as it was and before any device work: group_count 0 or > 8, a group index >= group_count, a null
 * table with a nonzero count (these are checked before the handle is looked at), a sharded renderer (world > 1; hala_rt_set_tile_shard
 * refuses the other order), and more than 2^29 - 1 path slots (pixels x samples x views: light connections carry the group in the top
 * bits of their slot word).  An update whose committed scene has more lights or materials than the tables cover fails before any
 * device work.  A successful call joins the second frame slot, allocates (12 B per path slot and group, 16 B per pixel, view
 * and group) or frees the buffers and restarts the accumulation.  Not built: gathering the images across ranks, groups in save_images,
 * light path expressions beyond the emitter. */
typedef struct hala_light_groups {
  uint32_t group_count;          /* 1..8 */
  uint32_t environment_group;
  uint32_t light_count;          /* entries of light_group: packed light index -> group */
  uint32_t material_count;       /* entries of material_group: material index -> group */
  const uint32_t* light_group;
  const uint32_t* material_group;
} hala_light_groups;             /* 32 B */
int hala_rt_set_light_groups(hala_rt_renderer* r, const hala_light_groups* g);
/* image `group` of view `view` (W*H*4 floats, row 0 = top); waits like hala_rt_read_image.  Refused while groups are off or for a
 * view / group that does not exist. */
int hala_rt_read_light_group(hala_rt_renderer* r, uint32_t view, uint32_t group, float* dst_rgba32f);
/* Relight view `view`: R = sum over g ascending of s_g * I_g from 0, per channel acc = acc + s * I (no fma); rgb_scales holds
 * 3 * group_count finite floats (negative ones accepted), group_count must equal the descriptor's.  Writes the linear R (alpha 1) and
 * tonemap(R * exposure_value) with the renderer's operators, exactly as the final image is written.  Stream-ordered on the renderer's
 * stream; refused while groups are off or for a view that does not exist. */
int hala_rt_relight(hala_rt_renderer* r, uint32_t view, const float* rgb_scales, uint32_t group_count);
/* the last relit image: which 0 linear, 1 tonemapped (W*H*4 floats); refused before the first hala_rt_relight */
int hala_rt_read_relit(hala_rt_renderer* r, int which, float* dst_rgba32f);
/* zero-copy: device address and byte size of a relit image (valid until the next hala_rt_set_light_groups, or destroy) */
int hala_rt_get_relit_buffer(hala_rt_renderer* r, int which, void** d_ptr, size_t* bytes);

/* Cryptomatte ID mattes (docs/RENDER_SPEC.md 15; no reference equivalent): per pixel, view and layer, a table of id -> coverage over every
 * sample of the accumulation, in the Cryptomatte form (Psyop, 2015) that Nuke, Blender, Fusion and Houdini read.  Layers: bit 0 object
 * (the name of the node a hit triangle's instance or a hit light came from; a null or empty name is node<k>), bit 1 material (material<m>,
 * or the caller's name for m; a light has none), bit 2 asset (the object name of the node's root).  A name is hashed as its UTF-8 bytes
 * with MurmurHash3_x86_32, seed 0; bit 23 of the hash is flipped when its exponent bits are 0 or 255, and the result is the stored id.
 * Each sample's first hit (RENDER_SPEC 13; a miss has no id) is folded in frame order into one 64-B record per pixel, view and layer:
 * [n, other, (id, count) x 7] as uint32, entries by count descending then id ascending, a sample whose id finds no room counts in other.
 * Ranked output: ranks 0..5 as (id as float bits, count / n), sublayer k = ranks 2k and 2k + 1 as R, G, B, A.  Images 0-5, the
 * statistics, the RNG and every existing refusal are the same with the feature on or off.  The records follow the views, adaptive sampling
 * (converged blocks keep theirs), update_batch (k frames equal k updates) and two updates in flight; every restart of the accumulation empties
 * them at the next frame 0.  NULL turns the feature off, the default.
 * Refused, with the renderer left as it was and before any device work: layer_mask 0 or > 7, a null name table with a nonzero count,
 * reserved words not 0 (these are checked before the handle is looked at), a sharded renderer (world > 1; hala_rt_set_tile_shard refuses
 * the other order).  A successful call joins the second frame slot, allocates (64 B per pixel, view and layer, and the 16-B
 * first-hit record per path slot while image 5 is off) or frees the records and restarts the accumulation.  Cost: one HBM-bound fold
 * launch per update right behind the resolve.  Not built: gathering the records across ranks, deep EXR, coverage
 * through transparent surfaces, pixel filters other than the camera jitter's box, a preview channel, material names from glTF. */
typedef struct hala_cryptomatte_desc {
  uint32_t layer_mask;               /* bit 0 object, bit 1 material, bit 2 asset */
  uint32_t material_name_count;      /* entries of material_names: material index -> UTF-8 name (NULL or "": material<m>) */
  const char* const* material_names;
  uint32_t reserved[2];              /* must be 0 */
} hala_cryptomatte_desc;             /* 24 B */
int hala_rt_set_cryptomatte(hala_rt_renderer* r, const hala_cryptomatte_desc* d);
/* layer 0 object, 1 material, 2 asset of view `view`: the three ranked sublayers, image k (ranks 2k and 2k + 1 as R, G, B, A = id, coverage,
 * id, coverage) at dst + k * W * H * 4, W*H*12 floats in all, row 0 = top; waits like hala_rt_read_image.  Refused while the layer is off,
 * for a view that does not exist and before the first update after a restart of the accumulation. */
int hala_rt_read_cryptomatte(hala_rt_renderer* r, uint32_t view, uint32_t layer, float* dst);
/* the raw records of the same (W*H*16 uint32, row-major: n, other, id_0, count_0, ..., id_6, count_6), for tests and tools */
int hala_rt_read_cryptomatte_records(hala_rt_renderer* r, uint32_t view, uint32_t layer, uint32_t* dst);
/* the layer's manifest: the JSON object {"name":"xxxxxxxx",...} (8 lowercase hex digits of the id) of every name the committed scene can
 * produce in it, in ascending byte order.  *length = its byte count without the terminating 0; dst NULL asks for the length only, else dst
 * gets the text and a 0 (capacity >= length + 1, else refused).  Refused while the layer is off. */
int hala_rt_get_cryptomatte_manifest(hala_rt_renderer* r, uint32_t layer, char* dst, size_t capacity, size_t* length);
/* single-part scanline OpenEXR 2.0, ZIP (16 lines per block): R, G, B, A = the view's linear accum, and per enabled layer <Layer>00.R ...
 * <Layer>02.A (CryptoObject, CryptoMaterial, CryptoAsset), all FLOAT, with the string attributes cryptomatte/<key>/name, /hash
 * (MurmurHash3_32), /conversion (uint32_to_float32) and /manifest; key = the first 7 hex digits of the raw hash of the layer name.
 * Refused like hala_rt_read_cryptomatte. */
int hala_rt_save_cryptomatte(hala_rt_renderer* r, uint32_t view, const char* path);

/* info()/statistics() (src/renderer.rs:212-218, :135-207) */
typedef struct hala_rt_info {
  uint32_t width;
  uint32_t height;
} hala_rt_info;
typedef struct hala_rt_statistics {
  uint64_t total_frames;       /* HalaRendererStatistics::total_frames */
  double last_gpu_ms;          /* GPU time of the last update (get_gpu_frame_time, renderer.rs:275) */
  uint64_t rays_last_update;   /* closest-hit + shadow traversals launched by the last update */
  uint64_t rays_total;
  double traverse_ms_last_update; /* time inside the traversal kernels only (HIP events on the renderer's stream) */
  /* totals since create / the last accumulation reset */
  double gpu_ms_total;
  double traverse_closest_ms_total;   /* k_trace_batch<closest> launches, HIP events on the renderer's stream */
  double traverse_shadow_ms_total;    /* k_trace_shadow launches (one event pair per depth brackets the light and the
                                       * environment launch; traverse_shadow_launches counts the launches as issued) */
  uint64_t traverse_closest_launches;
  uint64_t traverse_shadow_launches;
  uint64_t updates_rendered;
  uint64_t rays_closest_total;
  uint64_t rays_shadow_total;
  /* only counted while hala_rt_set_counting(r, 1): BVH nodes visited / triangles tested per kernel, and the
   * rays those counts belong to */
  uint64_t nodes_closest_total, tris_closest_total, nodes_shadow_total, tris_shadow_total;
  uint64_t rays_closest_counted, rays_shadow_counted;
  /* counting launches, wave level (SIMT utilisation): wave steps = node visits issued by a 64-lane wave (lane
   * utilisation of the node path = nodes / (64 * wave_steps)); leaf passes = executions of a leaf-test copy by a
   * wave, leaf lanes = lanes taking part in them (utilisation of the leaf path = leaf_lanes / (64 * leaf_passes)) */
  uint64_t wave_steps_closest_total, leaf_passes_closest_total, leaf_lanes_closest_total;
  uint64_t wave_steps_shadow_total, leaf_passes_shadow_total, leaf_lanes_shadow_total;
  /* the depth-0 share of traverse_closest_*: launches of the kernel that generates the camera rays it traces
   * (k_trace_primary); the rest are k_trace_batch launches over the bounce-ray queues */
  double traverse_primary_ms_total;
  uint64_t traverse_primary_launches;
  uint64_t nodes_primary_total, tris_primary_total, rays_primary_counted; /* counting launches, camera rays only */
  uint64_t rays_primary_total; /* camera rays of all updates (part of rays_closest_total) */
  /* rays of the updates whose launches carried timing events (hala_rt_set_launch_timing_period): the rays the
   * traverse_*_ms_total / *_launches figures belong to.  Equal to the *_total fields while every update is timed. */
  uint64_t rays_closest_timed, rays_primary_timed, rays_shadow_timed;
  /* the shade launches between the closest-hit and the shadow launches of the timed updates (k_shade: closest-hit shading,
   * miss, NEE set-up, BSDF sampling, queue compaction) */
  double shade_ms_total;
  uint64_t shade_launches;
  /* timed updates that ran with fused passes (hala_rt_set_pass_fusion(r, 2)): the launches of k_trace_shadow_then_batch — the shadow
   * passes of bounce d and the closest-hit pass of bounce d + 1 in one persistent launch — and the rays they traced from each queue
   * (bounce rays / connections).  Such updates add nothing to traverse_shadow_* and only their depth-0 launch to traverse_closest_*. */
  double traverse_fused_ms_total;
  uint64_t traverse_fused_launches;
  uint64_t rays_fused_closest_timed, rays_fused_shadow_timed;
} hala_rt_statistics;
int hala_rt_get_info(hala_rt_renderer* r, hala_rt_info* out);
int hala_rt_get_statistics(hala_rt_renderer* r, hala_rt_statistics* out);
/* HalaRendererStatistics::reset (src/renderer.rs:168-174), which the reference calls on the device-lost path
 * (src/rt_renderer.rs:557): total_frames := 0, so the next update() renders frame_index 0 and the running
 * means restart. */
int hala_rt_reset_accumulation(hala_rt_renderer* r);
/* enable = 1: update() launches the counting variants of the traversal kernels (BVH nodes visited and
 * triangles tested per ray — the inputs of the algorithmic-bytes figure). Slower; off by default. */
int hala_rt_set_counting(hala_rt_renderer* r, int enable);
/* Per-launch timing (the traverse_*_ms_total statistics) brackets every traversal launch with two HIP events, i.e. ~22 barrier
 * packets per update (70 us of a 2.25 ms frame on MI355X).  period = 0 (default): none; 1: every update is timed; n > 1: every n-th.
 * The frame-level figures (last_gpu_ms, gpu_ms_total, ray counts) are always collected. */
int hala_rt_set_launch_timing_period(hala_rt_renderer* r, uint32_t period);
/* Pass fusion: the shadow passes of bounce d and the closest-hit pass of bounce d + 1 are independent and can run as ONE persistent
 * launch (one tail of long rays per bounce instead of three).  mode 0: never; 1 (default): every update except the timed ones, which
 * keep one launch per pass so that every measured launch is one kernel symbol with the chip to itself; 2: always — timed updates then
 * fill the traverse_fused_* statistics.  Counting updates (hala_rt_set_counting) never fuse.  Images do not depend on the mode. */
int hala_rt_set_pass_fusion(hala_rt_renderer* r, uint32_t mode);
/* The variant ledger.  The traversal, shade and resolve kernels are compiled once per combination of launch-time flags; the library
 * notes on the host which combinations it has launched, so that a test suite can tell which of the compiled kernels it ran.
 * family and its flags, first flag = bit 0 of a combination's index:
 *   0 k_trace_primary            COUNT, STAGED, INST, VIEWS, FAR
 *   1 k_trace_batch              ANY, COUNT, ALPHA, STAGED, INST
 *   2 k_trace_shadow             COUNT, ALPHA, STAGED, INST, GROUPS
 *   3 k_trace_shadow_then_batch  ALPHA, STAGED, INST, GROUPS
 *   4 k_shade                    PRIMARY, SIMPLE, SCATTER, AOV, GROUPS
 *   5 k_resolve                  AOV, GROUPS
 * *launched: bit i is set if the kernel of combination i has been launched; *built: bit i is set if such a kernel exists (no kernel is
 * both STAGED and INST, ALPHA needs ANY, SIMPLE has no SCATTER, AOV needs PRIMARY).  Either pointer may be null.  reset != 0 clears the
 * family's launched bits after they were read.  The ledger is per process, not per renderer: every renderer of the process, on any
 * thread, adds to the same bits, and no call needs a renderer or a device.  An unknown family is an error. */
int hala_rt_variant_ledger(uint32_t family, uint64_t* launched, uint64_t* built, int reset);
/* Self-test of the exact-math helpers.  The kernels compute 1.0f / x and sqrtf(x) by a short sequence on the hardware's approximate
 * reciprocal and reciprocal square root (csrc/rt_math.h rcp_rn, sqrt_rn) that must give the bits of the IEEE expression for EVERY input.
 * which 0: the reciprocal, 1: the square root.  One kernel evaluates the helper and the plain expression for the `count` consecutive
 * binary32 bit patterns from `first` (first + count <= 2^32; the whole sweep is 2^32 patterns, in as many calls as the caller likes) and
 * returns through *mismatches how many patterns differ (two NaNs count as equal) and through *first_bad the lowest differing pattern,
 * 0xffffffff if there is none.  Either pointer may be null.  Runs on the calling thread's current device and needs no renderer.
 * _values: the same kernel on a list of `count` patterns in host memory (at most 2^28); it also writes, where the pointer is not null,
 * the bits the helper and the plain expression gave for each pattern to host arrays of `count` entries. */
int hala_rt_selftest_math(int which, uint32_t first, uint64_t count, uint64_t* mismatches, uint32_t* first_bad);
int hala_rt_selftest_math_values(int which, const uint32_t* patterns, uint32_t count, uint32_t* helper_bits, uint32_t* reference_bits,
                                 uint64_t* mismatches, uint32_t* first_bad);
/* Self-test of the collapse of a binary hierarchy into 4-wide nodes (csrc/bvh_build.hip: k_collapse_cost, k_collapse_level) on a small
 * tree from host memory: `leaves` >= 2 leaves at sorted positions 0 .. leaves - 1 and leaves - 1 inner nodes, node 0 the root.
 * left / right [leaves - 1]: child references (bit 31 set: the leaf at that sorted position, else an inner node); node_parent
 * [leaves - 1] (0xffffffff for the root) and leaf_parent [leaves]; first / last [leaves - 1]: the sorted positions below each node;
 * node_boxes [leaves - 1][6] and leaf_boxes [leaves][6]: min xyz, max xyz.  The tree is checked on the host (every node and leaf reached
 * once from the root, parents and ranges consistent, finite boxes); 1 <= leaf_max <= 8, leaf_max < leaves <= 2^20.  Runs the cost pass
 * and the level launches exactly as a build does and returns, where the pointer is not null: costs [leaves - 1][3] = C(node, 1 .. 3),
 * choices [leaves - 1] (the choice words), keep [leaves - 1], refs4 [leaves - 1][4] of which the first *node_count rows are the 4-nodes
 * in breadth-first order (0xffffffff: an empty slot), *levels.  Runs on the calling thread's current device and needs no renderer. */
int hala_rt_selftest_collapse(uint32_t leaves, uint32_t leaf_max, const uint32_t* left, const uint32_t* right, const uint32_t* node_parent,
                              const uint32_t* leaf_parent, const uint32_t* first, const uint32_t* last, const float* node_boxes,
                              const float* leaf_boxes, float* costs, uint32_t* choices, uint32_t* keep, uint32_t* refs4, uint32_t* node_count,
                              uint32_t* levels);
/* Self-test of the hierarchy builders (csrc/bvh_sah.hip, bvh_ploc.hip, and k_morton, the radix sort, k_hierarchy and k_fit of
 * bvh_build.hip): the binary tree one of them builds over `count` boxes from host memory, boxes [count][6] = min xyz, max xyz by id.
 * builder 1: SAH, 2: PLOC, 3: LBVH; ploc_tail / ploc_look_every as in hala_rt_build_options (0: the default; they change how PLOC's
 * rounds are driven, never the tree).  The call runs the functions a build runs, on the scene bounds a build would find: the exact union
 * of the boxes.  Out, to host arrays, in the form hala_rt_selftest_collapse takes: sorted_ids [count] (the id at every sorted position),
 * left / right / first / last / node_parent [count - 1] and leaf_parent [count] as described there (node 0 is the root), node_boxes
 * [count - 1][6]: per node the union of the boxes at its sorted positions first .. last, every min lowered and every max raised by `pad`
 * in one binary32 operation each.  The same boxes, pad and builder give the same bytes in every call.  Refused before anything runs on
 * the device: count < 2 or > 2^20, a null array, a box that is not finite or has min > max, a pad that is negative or not finite, a
 * builder outside 1 .. 3, ploc_tail > 2, ploc_look_every > 64.  Runs on the calling thread's current device and needs no renderer. */
int hala_rt_selftest_hierarchy(uint32_t count, const float* boxes, float pad, uint32_t builder, uint32_t ploc_tail, uint32_t ploc_look_every,
                               uint32_t* sorted_ids, uint32_t* left, uint32_t* right, uint32_t* first, uint32_t* last, uint32_t* node_parent,
                               uint32_t* leaf_parent, float* node_boxes);
/* Frames in flight.  Consecutive updates are independent except for the order in which their samples are folded into the accumulated
 * images, so updates without per-launch timing or counting alternate between two frame slots, each with its own stream, control block,
 * stack spill area, per-path state and queues: update k + 1 starts beside the last bounces of update k (its dense camera-ray launch and
 * depth-0 shade fill the chip the short last queues leave idle); its resolve and Cryptomatte fold wait for those of update k.  n = 2
 * (default): as described; hala_rt_render keeps bounding the updates in flight to two.  n = 1: strictly serial, one slot on the
 * renderer's stream.  Images, AOVs and ray counts do not depend on n, bit for bit.  Memory: the second slot doubles the wavefront
 * buffers (about 250 B per path: 2.1 -> 4.2 GB for a 1080p batch of four samples); it is allocated the first time an update finds the
 * other slot busy, and if that allocation fails the renderer keeps working with one slot.  gpu_ms_total sums the spans of the updates,
 * which overlap: it can exceed wall time.  The call joins both slots, then applies; n = 1 frees the second slot's buffers. */
int hala_rt_set_frames_in_flight(hala_rt_renderer* r, uint32_t n);
/* How many updates ran on the second frame slot since the renderer was created, and whether the second set of wavefront buffers is
 * allocated (LDS-staged scenes never allocate it: their updates share one set).  Either pointer may be null. */
int hala_rt_frames_in_flight_info(hala_rt_renderer* r, unsigned long long* second_slot_updates, uint32_t* second_buffers);
/* the 112-B record the last update uploaded (src/rt_renderer.rs:408-427) */
int hala_rt_get_global_uniform(hala_rt_renderer* r, hala_global_uniform* out);

/* What upload() packed (gpu_uploader.rs:99-122 cameras, :148-303 lights + AABBs, :306-331 materials,
 * :843-885 primitives/instances) — read back from the device for parity tests. Each call copies
 * min(capacity, count) records and returns the count through *count. */
int hala_rt_get_packed_cameras(hala_rt_renderer* r, hala_gpu_camera* dst, uint32_t capacity, uint32_t* count);
int hala_rt_get_packed_lights(hala_rt_renderer* r, hala_gpu_light* dst, hala_aabb* dst_aabbs, uint32_t capacity, uint32_t* count);
int hala_rt_get_packed_materials(hala_rt_renderer* r, hala_gpu_material* dst, uint32_t capacity, uint32_t* count);
int hala_rt_get_packed_primitives(hala_rt_renderer* r, hala_gpu_mesh_data* dst, float* dst_instance_3x4, uint32_t capacity, uint32_t* count);
/* env tables of set_envmap (src/envmap.rs:239-388): total_sum, marginal[H], conditional[W*H] */
int hala_rt_get_env_distribution(hala_rt_renderer* r, float* total_sum, float* marginal, float* conditional);

/* Textures of set 2 binding 0 (src/rt_renderer.rs:197-226) as uploaded by gpu_uploader.rs:334-403: every texture is a
 * full mip chain (gen_mipmaps, :400); the sampler is linear / linear-mip / REPEAT (:341-353).  8-bit images stay 8-bit at
 * every level (RGBA8 in HBM, decoded at fetch: docs/RENDER_SPEC.md 7.4), float images are RGBA32F.  Introspection + a stand-alone
 * fetch for parity tests: read_texture_level returns the level's texel VALUES (decoded to linear RGBA32F), uv_lod holds (u, v, lod)
 * triples. */
int hala_rt_get_texture_info(hala_rt_renderer* r, uint32_t texture, uint32_t* width, uint32_t* height, uint32_t* mips);
int hala_rt_read_texture_level(hala_rt_renderer* r, uint32_t texture, uint32_t level, float* dst_rgba32f);
/* Texel bundles of the committed scene (hala_rt_build_options::texture_bundles), as the last commit or refit left them: materials whose
 * maps are fetched from a bundle, materials with at least one map that are not (one map only, maps of different sizes, a float image,
 * bundles off), and the bytes of the bundle arena.  Fails before the first commit. */
typedef struct hala_texture_bundle_info {
  uint32_t bundle_count;
  uint32_t bundled_materials;
  uint32_t unbundled_textured_materials;
  uint32_t reserved;
  unsigned long long bundle_bytes;
} hala_texture_bundle_info;
int hala_rt_texture_bundle_info(hala_rt_renderer* r, hala_texture_bundle_info* info);
int hala_rt_sample_texture_host(hala_rt_renderer* r, uint32_t texture, const float* uv_lod, uint32_t count, float* dst_rgba32f);

/* Multi-GPU pixel-tile sharding (no reference equivalent; BASELINE.json north_star).  The frame is cut
 * into tile_size x tile_size tiles; tile t belongs to rank perm(t) % world (perm = fixed bijective
 * scramble).  After this call update() renders only this rank's tiles into a tile-major buffer;
 * hala_rt_tile_buffer gives its device address + byte size (per AOV) for the RCCL all-gather, and
 * hala_rt_scatter_gathered_tiles de-interleaves the gathered [world][tiles_per_rank][ts*ts][4] buffer (inside a tile the pixels
 * come in 8 x 8 blocks when ts is a multiple of 8: docs/RENDER_SPEC.md 9) into the row-major images of this renderer.  The renderer works on its own HIP stream: wait (hala_rt_wait_idle, or a stream
 * dependency on hala_rt_get_stream) before another stream reads the tile buffer — hala_rt_render does not flush.
 * world > 1 is refused while adaptive sampling is on (hala_rt_set_adaptive_sampling) or while the renderer has several views
 * (hala_rt_set_views). */
int hala_rt_set_tile_shard(hala_rt_renderer* r, uint32_t rank, uint32_t world, uint32_t tile_size);
int hala_rt_tile_buffer(hala_rt_renderer* r, int which, void** d_ptr, size_t* bytes);
/* the hipStream_t every launch of this renderer goes to (for stream-ordered hand-overs: hipStreamWaitEvent both ways).  Exception: every
 * other update without per-launch timing runs, from its camera-ray launch to the tail of its resolve, on a second stream beside the update
 * before it (hala_rt_set_frames_in_flight); every call into the library other than update and render first puts the renderer's stream
 * behind it, this one included — fetch the stream after the updates a hand-over is to cover. */
int hala_rt_get_stream(hala_rt_renderer* r, void** hip_stream);
int hala_rt_scatter_gathered_tiles(hala_rt_renderer* r, int which, const void* d_gathered, size_t bytes);

/* The exchange step itself (ncclAllGather over xGMI), inside the library so that a Rust / C host has a multi-GPU
 * path without any Python.  librccl is resolved on the first hala_rt_comm_* call (dlopen; the instance already in the process is
 * preferred, so a communicator handed to hala_rt_comm_attach meets the RCCL it came from): a host that renders on one GPU loads
 * libhalart.so without RCCL installed.  One process (or thread) per GPU; every rank calls the same sequence.
 *   hala_rt_comm_unique_id   : ncclGetUniqueId — rank 0 makes the 128-byte id and hands it to the other ranks over the host
 *                               application's own channel (MPI, a socket, torch.distributed.broadcast ...)
 *   hala_rt_comm_init_rank   : ncclCommInitRank on the renderer's device; rank / world must equal hala_rt_set_tile_shard's.
 *   hala_rt_comm_attach      : use a communicator the caller owns (an ncclComm_t) instead; it is not destroyed by the library.
 *   hala_rt_tile_allgather   : aov_mask bit k = AOV k (0 accum, 1 albedo, 2 normal, 3 final).  Gathers the rank's tile buffers and
 *                               de-interleaves them into this renderer's row-major images (read_image / save_images then work on
 *                               every rank).  Stream-ordered, never blocks the host: the collective runs on a side stream behind
 *                               the updates enqueued so far, and the renderer's stream waits for it.
 *   _begin / _finish         : the pipelined form: begin(k) snapshots the tile buffers (frame k + 1 may then overwrite them) and
 *                               starts the collective; it runs beside the rendering of frame k + 1 until finish() — called by the
 *                               next begin(), or explicitly — de-interleaves.  xGMI is point-to-point: a ring all-gather of
 *                               N x 33 MB is bound by one link per hop and can take as long as rendering a rank's share.
 *   hala_rt_get_gathered_buffer: the [world][tiles_per_rank][ts][ts][4] receive buffer of the last collective (tests).
 *   hala_rt_tile_allgather_begin_external + hala_rt_get_exchange_buffers: the same pipeline with the exchange done by the CALLER —
 *                               another transport (MPI, a CPU rehearsal of N ranks on one GPU), no communicator needed: begin_external
 *                               snapshots the tile buffers exactly like _begin; the caller then moves every rank's staging buffer
 *                               (rank k's at offset k x staged_bytes) into the receive buffer, stream-ordered on the exchange stream
 *                               the call returns, and calls _finish.
 * hala_rt_set_tile_shard completes a collective in flight and refuses to change rank / world while a communicator is attached. */
#define HALA_COMM_UNIQUE_ID_BYTES 128
int hala_rt_comm_unique_id(void* out_128_bytes);
int hala_rt_comm_init_rank(hala_rt_renderer* r, const void* unique_id_128_bytes, uint32_t rank, uint32_t world);
int hala_rt_comm_attach(hala_rt_renderer* r, void* nccl_comm);
int hala_rt_comm_destroy(hala_rt_renderer* r);
int hala_rt_tile_allgather(hala_rt_renderer* r, uint32_t aov_mask);
int hala_rt_tile_allgather_begin(hala_rt_renderer* r, uint32_t aov_mask);
int hala_rt_tile_allgather_finish(hala_rt_renderer* r);
int hala_rt_get_gathered_buffer(hala_rt_renderer* r, int which, void** d_ptr, size_t* bytes);
int hala_rt_tile_allgather_begin_external(hala_rt_renderer* r, uint32_t aov_mask);
int hala_rt_get_exchange_buffers(hala_rt_renderer* r, int which, void** d_staged, size_t* staged_bytes, void** d_receive, size_t* receive_bytes,
                                 void** hip_stream);
/* the same launched on a stream of the caller's (NULL: the renderer's): the de-interleave of frame k can then run beside the rendering
 * of frame k + 1.  The caller orders it against the renderer's stream (hala_rt_get_stream) before anything reads the images. */
int hala_rt_scatter_gathered_tiles_on_stream(hala_rt_renderer* r, int which, const void* d_gathered, size_t bytes, void* hip_stream);

/* ------------------------------------------------------------------------------------------------
 * The ray-batch operator under the renderer: what vkCmdTraceRaysKHR + the closest-hit stage do for
 * one batch (src/rt_renderer.rs:458-464, src/raytracing_program.rs:330-340).
 * ---------------------------------------------------------------------------------------------- */
typedef struct hala_ray {
  float origin[3];
  float tmin;        /* a negative tmin is clamped to +0 when the ray is set up (RENDER_SPEC 4.2: rays start at or after their origin) —
                      * in every traversal variant, whatever the scene's size */
  float direction[3];
  float tmax;
} hala_ray; /* 32 B */

typedef struct hala_hit {
  float t;       /* < 0 => miss */
  float u;
  float v;
  uint32_t prim; /* global triangle id (instance order, then triangle order); HALA_INVALID_INDEX on miss */
} hala_hit; /* 16 B */

/* mode 0: closest hit; mode 1: any hit (shadow): t = 1 if occluded else -1. Rays/hits are DEVICE
 * pointers (coalesced 32-B / 16-B records). If d_counters != NULL (device, 2 x uint64) the kernel
 * also adds the number of BVH nodes visited and triangles tested (for the algorithmic-bytes figure).
 * Streams: hip_stream = NULL launches on the renderer's stream.  The launch uses per-renderer scratch (work counters,
 * step counters, the traversal-stack spill area) that update() uses too, so all update / trace_rays launches of ONE
 * renderer are serialised on the device: a call on another stream first makes that stream wait (hipStreamWaitEvent)
 * for the previous such launch, wherever it ran, and records an event behind its own.  Calls may come from one host
 * thread at a time (the reference's renderer is !Send / !Sync too).
 * Far origins (RENDER_SPEC 4.2): a ray that starts beyond 16x the scene's largest absolute coordinate is traced from a point within one
 * scene diagonal of the scene box, and its hit carries the distance from the origin as given; the batch itself is not written to (the
 * renderer keeps a re-based copy of `count` rays, 36 B each). */
int hala_rt_trace_rays(hala_rt_renderer* r, const hala_ray* d_rays, hala_hit* d_hits, uint32_t count,
                       int mode, uint64_t* d_counters, void* hip_stream);
/* trace_rays_indirect (src/raytracing_program.rs:338-340): d_indirect points at a device-resident
 * VkTraceRaysIndirectCommandKHR {uint32 width, height, depth}; width*height*depth rays are traced. */
int hala_rt_trace_rays_indirect(hala_rt_renderer* r, const hala_ray* d_rays, hala_hit* d_hits,
                                const uint32_t* d_indirect, int mode, void* hip_stream);
/* Host-pointer convenience wrapper used by the tests (copies in/out around the same kernel). */
int hala_rt_trace_rays_host(hala_rt_renderer* r, const hala_ray* rays, hala_hit* hits, uint32_t count,
                            int mode, uint64_t counters[2]);

/* Multi-hit ray batches (RENDER_SPEC 4.7): the k nearest hits of every ray, 1 <= k <= HALA_MAX_MULTI_HITS.  Ray i gets the records
 * d_hits[i*k .. i*k + k): every triangle the test of 4.2 accepts inside (tmin, tmax), ascending by t, equal t by ascending triangle id,
 * cut after k; the rest of the slice are miss records {-1, 0, 0, HALA_INVALID_INDEX}.  d_counts (device, `count` words, or NULL) gets
 * the number of hit records of each ray; a count equal to k means "possibly more".  Materials play no part (an invisible or translucent
 * triangle is a triangle), k = 1 is mode 0 of hala_rt_trace_rays bit for bit, and the answer does not depend on how the tree was built.
 * Everything else is the contract of hala_rt_trace_rays: a committed scene, count == 0 a no-op, the renderer's scratch and its stream
 * order, the scene as it stands at the renderer's shutter step, far origins re-based in the renderer's own copy of the batch (every
 * reported t is the distance from the origin as given).  Refused with a message and without touching anything: k outside 1..16, a null
 * batch, no committed scene, count * k beyond 2^32 records.  A caller who continues a full list with tmin = the last t loses the other
 * triangles at exactly that t. */
#define HALA_MAX_MULTI_HITS 16
int hala_rt_trace_rays_multi(hala_rt_renderer* r, const hala_ray* d_rays, hala_hit* d_hits /* count*k */, uint32_t* d_counts /* or NULL */,
                             uint32_t count, uint32_t k, void* hip_stream);
int hala_rt_trace_rays_multi_host(hala_rt_renderer* r, const hala_ray* rays, hala_hit* hits, uint32_t* counts, uint32_t count, uint32_t k);

/* Closest-point query batches (RENDER_SPEC 4.8): for every point, the nearest point of the scene's surface within `radius` of it.
 * Query i is answered in d_out[i]: the distance, the barycentrics (u, v) with the meaning they have in hala_hit, the global triangle id,
 * the surface point itself and the region of the triangle it lies in (0 face; 1 / 2 / 3 edge AB / AC / BC; 4 / 5 / 6 vertex A / B / C).
 * Among the triangles whose squared distance is at most radius * radius, the least (squared distance, triangle id) wins: ties go to the
 * lower id, so the answer does not depend on how the tree was built.  A query that nothing answers (a NaN or negative radius among them)
 * gets the miss record {-1, 0, 0, HALA_INVALID_INDEX, 0, 0, 0, 0}; a radius of FLT_MAX or +inf means "no limit".  Materials play no part.
 * Everything else is the contract of hala_rt_trace_rays: a committed scene, count == 0 a no-op, the renderer's scratch and its stream
 * order, the scene as it stands at the renderer's shutter step, after the last refit.  There is no far-origin re-basing (a point has no
 * direction to slide along): the per-triangle arithmetic is the spec's at any distance.  Refused with a message and without touching
 * anything: a null batch, no committed scene, a two-level tree (hala_bvh_info::instance_ref_count > 0: distances in an instance's object
 * space are not world distances under a non-uniform transform).  Not built: closest points on two-level trees — commit such a scene
 * flattened (instancing = 0, the automatic and faster form). */
typedef struct hala_point_query {
  float point[3];
  float radius;
} hala_point_query; /* 16 B */
typedef struct hala_closest_point {
  float distance; /* < 0 => miss */
  float u;
  float v;
  uint32_t prim;  /* global triangle id; HALA_INVALID_INDEX on miss */
  float point[3]; /* the nearest surface point */
  uint32_t region;
} hala_closest_point; /* 32 B */
int hala_rt_closest_points(hala_rt_renderer* r, const hala_point_query* d_queries, hala_closest_point* d_out, uint32_t count, void* hip_stream);
int hala_rt_closest_points_host(hala_rt_renderer* r, const hala_point_query* queries, hala_closest_point* out, uint32_t count);
/* The same batch through the counting variant of the kernel: d_counters (device, 2 x uint64, or NULL) is set to the number of BVH nodes
 * visited and of triangles tested.  For measurements (scripts/closest_point_timing.py); the answers are the same bytes. */
int hala_rt_closest_points_counted(hala_rt_renderer* r, const hala_point_query* d_queries, hala_closest_point* d_out, uint32_t count,
                                   uint64_t* d_counters, void* hip_stream);

/* Signed distance grids (RENDER_SPEC 4.9): the scene's distance field on a grid of cubic voxels.  Voxel (i, j, k) stands at
 * p = fma((float)index, spacing, origin) per axis (`origin` is the centre of voxel (0, 0, 0)); d_distance[(k * ny + j) * nx + i] is the
 * distance hala_rt_closest_points answers the query (p, band) with, bit for bit, or `band` where it has no answer; d_prim (or NULL) gets
 * the answer's triangle id, or HALA_INVALID_INDEX.  `band` is >= 0 or +inf and holds for the whole grid; each of dims is 1 .. 1024.
 * flags: bit 0 HALA_GRID_SIGNED — a voxel is inside iff the ray from it along +x (a mode-0 ray from the row's voxel 0, far-origin rule
 * included) crosses the scene an odd number of times beyond it, and inside flips the value's sign bit (so -band and -0 occur).  That sign
 * is exact for closed surfaces, arbitrary but pinned for open ones, and a row that runs exactly through a shared edge counts it twice:
 * keep `origin` off the vertices' coordinates.  Bits 1-2 choose the kernel of the distance pass: 0 automatic, 1 one voxel per lane, 2 one
 * 4 x 4 x 4 brick per wave; the result does not depend on it, nor on the builder or the tree form.  Everything else is the contract of
 * hala_rt_trace_rays: a committed scene, the renderer's scratch and its stream order, the scene as it stands at the renderer's shutter
 * step, after the last refit.  Refused with a message and without touching anything: a null description or output, no committed scene, a
 * two-level tree (as for closest points), a dim of 0 or above 1024, a spacing that is not finite and positive, a NaN or negative band, any
 * other flag bit.  Not built: two-level trees, per-axis spacing, sparse or brick-list output, gradients, a sign from pseudo-normals or
 * winding numbers, seeding a brick's limit from its neighbour. */
typedef struct hala_distance_grid_desc {
  float origin[3];
  float spacing;
  uint32_t dims[3]; /* nx, ny, nz */
  float band;
  uint32_t flags;
} hala_distance_grid_desc; /* 36 B */
#define HALA_GRID_SIGNED 1u
#define HALA_GRID_METHOD_SHIFT 1 /* (flags >> 1) & 3: 0 automatic, 1 per lane, 2 per wave */
int hala_rt_distance_grid(hala_rt_renderer* r, const hala_distance_grid_desc* desc, float* d_distance, uint32_t* d_prim /* or NULL */, void* hip_stream);
int hala_rt_distance_grid_host(hala_rt_renderer* r, const hala_distance_grid_desc* desc, float* distance, uint32_t* prim /* or NULL */);
/* The same grid through the counting variants of the kernels: d_counters (device, 6 x uint64, or NULL) is set to
 *   [0] node visits and [1] triangle tests of the distance pass, each counted per lane that holds a voxel: in method 1 a lane's own
 *       visit of a node / its own test of a triangle; in method 2 every visit (test) of the wave counts once for each of its lanes that
 *       holds a voxel, since each of them runs the child keys (the triangle's arithmetic) — [0] / voxels and [1] / voxels are the
 *       arithmetic one voxel costs in either method;
 *   [2] node visits and [3] triangle tests of the row pass (per lane: one lane owns one row), 0 for an unsigned grid;
 *   [4] nodes and [5] triangles a wave FETCHED in method 2 (one fetch serves the wave's 64 lanes), 0 in method 1, where every count of
 *       [0], [1] is a fetch of its own.
 * For measurements (scripts/distance_grid_timing.py); the grid is the same bytes. */
int hala_rt_distance_grid_counted(hala_rt_renderer* r, const hala_distance_grid_desc* desc, float* d_distance, uint32_t* d_prim /* or NULL */,
                                  uint64_t* d_counters, void* hip_stream);

/* Occlusion batches (RENDER_SPEC 4.10): ambient occlusion and the bent normal at surface points.  Sample i is a point with a normal
 * (any length: it is normalised), a `bias` along that normal to the common origin o = fma(n, bias, point) of its rays, and a `reach`.
 * `rays` = N directions (1 <= N <= HALA_MAX_OCCLUSION_RAYS) are drawn cosine-distributed over the normal's hemisphere from the stream
 * (i, seed) of RENDER_SPEC 2.3, in the lanes that trace them: no ray is uploaded, copied or read back.  Ray j of sample i is the mode-1
 * (any-hit) ray (o, 0, d_j, reach) of hala_rt_trace_rays, entry i * N + j of a batch, and its occlusion bit is what that call answers
 * for it, ray for ray, on every tree form and builder: `reach` means what tmax means there (FLT_MAX or +inf: no limit; NaN or <= 0:
 * nothing occludes), far origins are re-based, invisible materials never block and translucent ones block by the ray's key; media play
 * no part.  d_out[i] = {visibility = unoccluded / N, bent = the normalised sum of the unoccluded directions in ascending j, or 0}.
 * d_masks (device, count * ceil(N / 32) words, or NULL: the renderer keeps them in a buffer of its own): bit j & 31 of word
 * i * ceil(N / 32) + (j >> 5) is set iff ray j is occluded, bits >= N are 0.  A sample whose normal has a squared length that is not
 * positive and finite, or whose point or bias is not finite, traces nothing: its record is {-1, 0, 0, 0} and its words are 0.
 * A bias of 0 puts the origin into the surface's own triangles, where rounding decides whether t > 0: the surface occludes itself at
 * random; use the scene's ray_eps (1e-5 of the scene box's diagonal, RENDER_SPEC 3) or more.
 * Everything else is the contract of hala_rt_trace_rays: a committed scene, count == 0 a no-op, the renderer's scratch and its stream
 * order, the scene as it stands at the renderer's shutter step, after the last refit.  Refused with a message and without touching
 * anything: rays outside 1..256, a null sample or output pointer, no committed scene, count * rays >= 2^32.
 * Not built: stratified or low-discrepancy directions, uniform-hemisphere weighting, a per-ray distance falloff, an AO image of the
 * frame from the first-hit AOVs, baking into a primitive's vertices in one call (into its texture: hala_rt_bake_occlusion below). */
#define HALA_MAX_OCCLUSION_RAYS 256
typedef struct hala_occlusion_sample { float point[3]; float bias; float normal[3]; float reach; } hala_occlusion_sample; /* 32 B */
typedef struct hala_occlusion { float visibility; /* < 0: invalid sample */ float bent[3]; } hala_occlusion;               /* 16 B */
int hala_rt_occlusion(hala_rt_renderer* r, const hala_occlusion_sample* d_samples, hala_occlusion* d_out,
                      uint32_t* d_masks /* count * ceil(rays/32) words, or NULL */, uint32_t count, uint32_t rays, uint32_t seed, void* hip_stream);
int hala_rt_occlusion_host(hala_rt_renderer* r, const hala_occlusion_sample* samples, hala_occlusion* out, uint32_t* masks /* or NULL */,
                           uint32_t count, uint32_t rays, uint32_t seed);

/* Bake maps (RENDER_SPEC 4.11): occlusion baked into the texture space of one instance, without leaving the device.  The instance's
 * triangles are rasterised into a `width` x `height` map by their texture coordinates (texel (x, y) has index y * width + x, row 0 is the
 * row of the smallest v, as the texture sampler reads it; no wrap: what lies outside [0, 1] falls off the map).  A texel whose centre a
 * triangle covers (edges included; of several, the lowest global triangle id) becomes the hala_occlusion_sample at the surface point
 * and normal found there: `normal` is cross(e1, e2) of the triangle (not normalised), or with HALA_BAKE_SHADING_NORMAL the interpolated
 * vertex normal moved to world space as the shade path does it; HALA_BAKE_FLIP_NORMAL negates either; `bias` and `reach` are copied
 * into every sample.  A texel nothing covers gets the all-zero sample, which is invalid and traces nothing.  d_texels (or NULL)
 * gets, per texel, the barycentrics and the triangle of its sample and `source`, the index of the texel its record came from.
 * hala_rt_bake_samples writes the samples (and ignores `margin`); they are what any later texture-space operator starts from.
 * hala_rt_bake_occlusion writes what hala_rt_occlusion answers for exactly that sample buffer with (rays, seed) — sample i is texel i —
 * and then fills the gutters: a texel without a sample takes the record of the nearest texel with one (least squared distance, then
 * least index) among those within `margin` texels in x and in y, and names it in `source`; with none, its record stays the invalid one
 * {-1, 0, 0, 0} and `source` 0xffffffff.  Samples, ownership and masks live in buffers the renderer owns, which grow on demand.
 * Everything else is the contract of hala_rt_trace_rays: the renderer's scratch and its stream order, no host synchronisation in the
 * device forms — except where one of the renderer's buffers has to grow (the first call, and the first at a larger map, ray count or
 * instance): freeing the smaller buffer waits for the device, as it does in hala_rt_occlusion without a mask array —, the scene as it
 * stands after the last refit.
 * Cost limit: a UV triangle so thin that rounding decides its coverage anywhere along its lines (|area| within 2^-17 of its box's
 * larger side squared, in texel units; exactly degenerate ones cover nothing and cost nothing) is tested against every 8 x 8 block of
 * the map, about 40 us each at 4096 x 4096 on an MI355X, all in one kernel launch that nothing cuts short: weld or drop such triangles
 * before baking a mesh that has thousands of them.  Refused with a message and without touching anything: a null description
 * or output, no committed scene, a two-level tree (the records of instanced primitives are in object space: commit with instancing =
 * 0), `instance` out of range, a dimension of 0 or above HALA_MAX_BAKE_DIM, `margin` above HALA_MAX_BAKE_MARGIN, an unknown flag bit,
 * a non-finite bias, rays outside 1..256, width * height * rays >= 2^32.
 * hala_rt_bake_occlusion hands every texel of the map to the occlusion pass, covered or not: a map with much gutter is baked faster as
 * an atlas of one chart (hala_rt_bake_atlas_occlusion below), which traces the covered texels only.
 * Not built: vertex baking, supersampled or conservative coverage, UV wrap, a second UV set, two-level trees. */
#define HALA_MAX_BAKE_DIM 4096
#define HALA_MAX_BAKE_MARGIN 16
#define HALA_BAKE_SHADING_NORMAL 1u
#define HALA_BAKE_FLIP_NORMAL 2u
typedef struct hala_bake_desc {
  uint32_t instance;      /* index in instance order (RENDER_SPEC 3) */
  uint32_t width, height; /* 1 .. HALA_MAX_BAKE_DIM */
  uint32_t flags;         /* HALA_BAKE_* */
  float bias, reach;      /* of every sample (RENDER_SPEC 4.10) */
  uint32_t margin;        /* dilation reach in texels, 0 .. HALA_MAX_BAKE_MARGIN */
} hala_bake_desc;         /* 28 B */
typedef struct hala_bake_texel { float u, v; uint32_t prim; uint32_t source; } hala_bake_texel; /* 16 B; no sample: {0, 0, ~0, ~0} */
int hala_rt_bake_samples(hala_rt_renderer* r, const hala_bake_desc* desc, hala_occlusion_sample* d_samples /* width * height */,
                         hala_bake_texel* d_texels /* width * height, or NULL */, void* hip_stream);
int hala_rt_bake_samples_host(hala_rt_renderer* r, const hala_bake_desc* desc, hala_occlusion_sample* samples, hala_bake_texel* texels /* or NULL */);
int hala_rt_bake_occlusion(hala_rt_renderer* r, const hala_bake_desc* desc, uint32_t rays, uint32_t seed, hala_occlusion* d_out /* width * height */,
                           hala_bake_texel* d_texels /* or NULL */, void* hip_stream);
int hala_rt_bake_occlusion_host(hala_rt_renderer* r, const hala_bake_desc* desc, uint32_t rays, uint32_t seed, hala_occlusion* out,
                                hala_bake_texel* texels /* or NULL */);

/* Bake atlases (RENDER_SPEC 4.12): several instances in one map.  `charts` is a host array of desc->chart_count entries, read before the
 * call returns; each places one instance of the scene: a triangle's texture coordinates go through uv * scale + offset (one fma per
 * component) before they are scaled to texels, and everything behind that is the bake map above — the coverage rule, the sample, the
 * texel record, with `flags` (HALA_BAKE_*) per chart since instances wind differently.  A texel that triangles of several charts cover
 * belongs to the lowest global triangle id among all of them, as within one instance.  A negative scale mirrors a chart, a zero scale
 * covers nothing.  An atlas of one chart with scale (1, 1) and offset (0, 0) is the bake map of that instance (bit for bit unless a
 * texture coordinate is -0, which the fma turns into +0).
 * hala_rt_bake_atlas_samples writes the samples and texel records (and ignores `margin`); hala_rt_bake_atlas_occlusion writes what
 * hala_rt_occlusion answers for exactly that sample buffer with (rays, seed), sample i being texel i, then the dilation over the whole
 * atlas.  Its occlusion pass traces only the texels that have a sample: their list is built on the device from the owner map, so a
 * texel of the gutter costs one store.  The list stays inside the renderer.  Scratch, stream order, growing buffers and the optional
 * d_texels are as for the bake maps.  Refused with a message and without touching anything: a null description, chart table or output,
 * no committed scene, a two-level tree, chart_count 0 or above the scene's instance count, an instance out of range or named twice, an
 * unknown flag bit, a non-finite scale, offset or bias, a dimension of 0 or above HALA_MAX_BAKE_DIM, `margin` above
 * HALA_MAX_BAKE_MARGIN, rays outside 1..256, width * height * rays >= 2^32.
 * Not built: packing charts into an atlas (the layout is the caller's), vertex baking, supersampled or conservative coverage, UV wrap, a
 * second UV set, two-level trees, handing the list of owned texels to the caller, compaction inside plain hala_rt_occlusion. */
typedef struct hala_bake_chart {
  uint32_t instance; /* index in instance order (RENDER_SPEC 3); at most one chart per instance */
  uint32_t flags;    /* HALA_BAKE_* */
  float scale[2];    /* of (u, v) */
  float offset[2];   /* of (u, v), in units of the atlas: [0, 1] is the map */
} hala_bake_chart;   /* 24 B */
typedef struct hala_bake_atlas_desc {
  uint32_t width, height; /* 1 .. HALA_MAX_BAKE_DIM */
  float bias, reach;      /* of every sample (RENDER_SPEC 4.10) */
  uint32_t margin;        /* dilation reach in texels, 0 .. HALA_MAX_BAKE_MARGIN */
  uint32_t chart_count;   /* 1 .. the scene's instances */
} hala_bake_atlas_desc;   /* 24 B */
int hala_rt_bake_atlas_samples(hala_rt_renderer* r, const hala_bake_atlas_desc* desc, const hala_bake_chart* charts,
                               hala_occlusion_sample* d_samples /* width * height */, hala_bake_texel* d_texels /* width * height, or NULL */,
                               void* hip_stream);
int hala_rt_bake_atlas_samples_host(hala_rt_renderer* r, const hala_bake_atlas_desc* desc, const hala_bake_chart* charts, hala_occlusion_sample* samples,
                                    hala_bake_texel* texels /* or NULL */);
int hala_rt_bake_atlas_occlusion(hala_rt_renderer* r, const hala_bake_atlas_desc* desc, const hala_bake_chart* charts, uint32_t rays, uint32_t seed,
                                 hala_occlusion* d_out /* width * height */, hala_bake_texel* d_texels /* or NULL */, void* hip_stream);
int hala_rt_bake_atlas_occlusion_host(hala_rt_renderer* r, const hala_bake_atlas_desc* desc, const hala_bake_chart* charts, uint32_t rays, uint32_t seed,
                                      hala_occlusion* out, hala_bake_texel* texels /* or NULL */);

/* Transfer bakes (RENDER_SPEC 4.13): every texel of one instance's bake map (the receiver: `desc` is the bake description above, with
 * its coverage rule, texel record and normal flags; `bias` must be finite and is otherwise not read, like `reach`) is projected onto
 * OTHER instances of the scene, the targets.  From the texel's surface point the ray starts `front` ahead along the unit normal n and
 * runs against it: o = point + front * n, d = -n, t in (0, front + back).  Only triangles of target instances are seen — the receiver's
 * own surface and every other instance let the ray through, whatever their materials — and the nearest of them by (t, triangle id)
 * is the texel's record: the hit as hala_rt_trace_rays reports it (t, u, v, prim), the target's interpolated vertex normal at (u, v)
 * in world space (unit length, as the shade path moves it there; not turned to face the ray, not affected by the receiver's flags) and
 * height = front - t, the signed offset of the target's surface from the receiver's along n: the displacement value.  A texel without
 * a sample, an invalid sample and a ray that meets no target all get {-1, 0, 0, ~0, {0, 0, 0}, 0}; d_texels (or NULL) tells them apart.
 * Then the dilation of the bake maps, over the 32-B records: a texel without a sample takes the record of the nearest texel with one,
 * hit or miss, within `margin`.
 * `targets` is a host array of transfer->target_count instance indices in instance order (RENDER_SPEC 3), read before the call
 * returns; their order does not matter.  target_count == 0 (then `targets` may be NULL) means every instance but the receiver.
 * Scratch, stream order, growing buffers and the optional d_texels are as for the bake maps.  Refused with a message and without
 * touching anything: everything hala_rt_bake_samples refuses, a null `transfer`, transfer->flags != 0, a negative or non-finite
 * `front`, a negative or NaN `back` (+inf is allowed), target_count above the scene's instance count, NULL `targets` with a count, a
 * target out of range or named twice, the receiver among the targets, a scene of one instance with target_count == 0.
 * Not built: any rule but the first hit seen from the cage (no nearest-to-the-receiver, no two-sided search); tangent-space encoding of
 * the normal (the texel record's (u, v, prim) and the world normal give a host what it needs); an atlas form; instance masks on plain
 * ray batches (hala_rt_trace_rays, hala_rt_trace_rays_multi); supersampling; two-level trees. */
typedef struct hala_bake_transfer_desc {
  float front, back;     /* distances along the normal: finite front >= 0; back >= 0 or +inf */
  uint32_t flags;        /* 0 */
  uint32_t target_count; /* 0: every instance but the receiver */
} hala_bake_transfer_desc; /* 16 B */
typedef struct hala_bake_transfer_hit {
  float t, u, v;
  uint32_t prim;
  float normal[3];
  float height;
} hala_bake_transfer_hit; /* 32 B; no hit: {-1, 0, 0, ~0, {0, 0, 0}, 0} */
int hala_rt_bake_transfer(hala_rt_renderer* r, const hala_bake_desc* desc, const hala_bake_transfer_desc* transfer, const uint32_t* targets,
                          hala_bake_transfer_hit* d_out /* width * height */, hala_bake_texel* d_texels /* or NULL */, void* hip_stream);
int hala_rt_bake_transfer_host(hala_rt_renderer* r, const hala_bake_desc* desc, const hala_bake_transfer_desc* transfer, const uint32_t* targets,
                               hala_bake_transfer_hit* out, hala_bake_texel* texels /* or NULL */);

/* BVH introspection for the oracle cross-check: 64-B nodes + 48-B triangles as laid out in HBM.
 * node_width is 4: compressed 4-wide nodes (docs/RENDER_SPEC.md §4.1b). */
typedef struct hala_bvh_info {
  uint32_t node_count;
  uint32_t triangle_count;
  uint32_t max_depth;
  uint32_t lds_node_count; /* nodes staged in LDS by the traversal kernel */
  float scene_min[3];
  float scene_max[3];
  uint32_t node_width;
  /* two-level trees (RENDER_SPEC 4.5; scenes in which several instances reference one primitive): the triangles the trees store (every
   * instanced primitive once; == triangle_count otherwise), the nodes of the instance levels (the first nodes of the array; 0: one-level
   * tree) and the instance references their leaves index */
  uint32_t stored_triangle_count;
  uint32_t instance_node_count;
  uint32_t instance_ref_count;
  uint64_t tree_bytes; /* device bytes of nodes + triangles (+ any-hit copy) + shading records + instance tables */
} hala_bvh_info;
int hala_rt_get_bvh_info(hala_rt_renderer* r, hala_bvh_info* out);
/* node_count nodes and stored_triangle_count triangles.  Two-level trees: child references are absolute; a reference with bits 31..28 = 0xF
 * is an instance leaf whose low 28 bits index the records of hala_rt_download_instance_refs (64 B each: 3 rows of world -> object and the
 * translation as 12 floats, then root node, global id of the instance's first triangle, first shading record, instance index); the
 * triangles of an instanced primitive are in object space and carry ids local to the primitive. */
int hala_rt_download_bvh(hala_rt_renderer* r, void* nodes_64B, void* triangles_48B);
int hala_rt_download_instance_refs(hala_rt_renderer* r, void* refs_64B, uint32_t capacity, uint32_t* count);
/* Refit after vertex/transform edits (north_star "BVH build/refit"; the reference rebuilds only):
 * re-flattens instances with the given node local transforms and refits AABBs bottom-up on the GPU.  The three hala_rt_update_* calls
 * need a committed scene (before hala_rt_commit they are refused) and take effect at the next hala_rt_refit: until then updates render
 * the scene as it was and keep accumulating.  A refused call changes nothing; the edits made before it still apply at the refit. */
int hala_rt_update_node_transform(hala_rt_renderer* r, uint32_t node_index, const float local_transform[16]);
/* Deforming geometry: replaces the vertices of primitive `primitive_index` of mesh `mesh_index` (indices into the scene handed
 * to hala_rt_set_scene, cpu/mesh.rs: HalaMesh::primitives).  The vertex count must be the primitive's own (the topology, i.e. the
 * index buffer, stays); host pointer, copied before the call returns.  Takes effect at the next hala_rt_refit. */
int hala_rt_update_vertices(hala_rt_renderer* r, uint32_t mesh_index, uint32_t primitive_index, const hala_vertex* vertices,
                            uint32_t vertex_count);
/* Replaces material `material_index` of the scene (cpu::HalaMaterial, the record hala_rt_set_scene took); texture indices must stay
 * within the scene's textures.  Takes effect at the next hala_rt_refit (which re-publishes the packed 144-B records; the geometry
 * is untouched, so is the tree). */
int hala_rt_update_material(hala_rt_renderer* r, uint32_t material_index, const hala_material_desc* material);
/* Applies the edits: node hierarchies, materials, camera / light / instance records, and — if an instance's transform or a primitive's vertices
 * changed — the tree (topology kept, boxes re-derived).  A move of camera or light nodes alone leaves the tree untouched.  The
 * accumulation restarts either way (every adaptive-sampling block is active again); the views, the AOV switches, the light-group
 * tables and the adaptive-sampling parameters are kept.  hala_rt_denoise is refused until new samples (and, sharded, a new gather)
 * arrive; hala_rt_read_denoised keeps returning the last denoised frame. */
int hala_rt_refit(hala_rt_renderer* r);

/* ------------------------------------------------------------------------------------------------
 * Deformers (docs/RENDER_SPEC.md 17; no reference equivalent): morph targets and a four-influence skin of one primitive, resident on
 * the GPU.  The rest pose, the deltas and the skin bindings are uploaded once; per frame the host hands over morph weights and joint
 * matrices (a few hundred bytes), and the next hala_rt_refit poses the vertices on the device just ahead of refitting the tree.
 * A renderer that never registers a deformer behaves exactly as before.
 * ---------------------------------------------------------------------------------------------- */
typedef struct hala_deformer_desc {
  uint32_t mesh_index, primitive_index;
  uint32_t target_count;               /* 0 .. HALA_MAX_MORPH_TARGETS */
  const float* target_position_deltas; /* [target][vertex][3] */
  const float* target_normal_deltas;   /* same shape, or NULL */
  const float* target_tangent_deltas;  /* same shape, or NULL */
  uint32_t joint_count;                /* 0: no skin; <= HALA_MAX_JOINTS */
  const uint16_t* joints;              /* [vertex][4], each < joint_count */
  const float* weights;                /* [vertex][4], used as given (not renormalised) */
} hala_deformer_desc; /* 64 B */
/* Registers a deformer on one primitive of the committed scene (before hala_rt_commit the call is refused like the other edits).  The
 * primitive's current vertices become the rest pose; host pointers, copied to the device before the call returns.  The weights start
 * at 0 and the palette at the identity: a refit right after the call changes nothing.  One deformer per primitive: a second call
 * replaces the first (the rest pose stays the one the first call took).  Refused, changing nothing: the mesh or primitive does not
 * exist; target_count above HALA_MAX_MORPH_TARGETS or joint_count above HALA_MAX_JOINTS; neither targets nor a skin; a joint index
 * >= joint_count; a delta or weight that is not finite (checked here, on the host).  hala_rt_set_scene drops every deformer. */
int hala_rt_set_deformer(hala_rt_renderer* r, const hala_deformer_desc* desc);
/* Records the pose of a deformer on the host: no device work, no synchronisation.  morph_weights (weight_count of them) and
 * joint_matrices_3x4 (joint_count row-major 3 x 4 matrices acting in the primitive's object space, after the morph) may each be NULL:
 * that part of the pose is kept.  Takes effect at the next hala_rt_refit: until then updates render the scene as it was and keep
 * accumulating.  Refused, changing nothing: the primitive has no deformer; weight_count differs from the registered target_count or
 * joint_count from the registered joint_count; a weight or matrix entry that is not finite. */
int hala_rt_update_deformer(hala_rt_renderer* r, uint32_t mesh_index, uint32_t primitive_index, const float* morph_weights,
                            uint32_t weight_count, const float* joint_matrices_3x4, uint32_t joint_count);
/* Removes the deformer of a primitive: the next hala_rt_refit restores the rest pose and frees the tables.  Refused when the primitive
 * has none.  While a primitive has a deformer, hala_rt_update_vertices on it is refused ("clear it first").
 * The refit contract: hala_rt_refit poses every deformer whose parameters changed (one launch of k_deform for all of them, one or many, on the renderer's stream)
 * and then refits as it does after hala_rt_update_vertices; every instance of a posed primitive starts without temporal history
 * (hala_rt_set_temporal) unless hala_rt_set_temporal_vertex_motion lets the history follow its triangles.  Finite parameters can still overflow: when a posed position is not finite, hala_rt_refit fails with
 * "Vertex position is not finite.", the vertices and the tree stay exactly as they were, the offending parameters fall back to the last
 * applied ones, and every other pending edit stays pending for the next refit. */
int hala_rt_clear_deformer(hala_rt_renderer* r, uint32_t mesh_index, uint32_t primitive_index);
/* Reads a primitive's vertices back from the device, behind everything enqueued on the renderer's stream: the posed mesh of a deformed
 * primitive (as the last refit left it), the uploaded vertices of any other.  Copies min(capacity, count) records; *count receives
 * the primitive's vertex count.  Needs a committed scene. */
int hala_rt_read_vertices(hala_rt_renderer* r, uint32_t mesh_index, uint32_t primitive_index, hala_vertex* dst, uint32_t capacity,
                          uint32_t* count);

/* Recomputed normals (docs/RENDER_SPEC.md 17 "Recomputed normals"), per deformer and opt-in.  In mode HALA_DEFORM_NORMALS_AS_POSED
 * (the default) a posed vertex carries the normal and tangent k_deform gives it: rest value plus deltas, times the skinning matrix.  In
 * mode HALA_DEFORM_NORMALS_RECOMPUTED every pose of the deformer — a refit, the batched launch of a rig, a shutter step — is followed
 * on the device by two more launches that derive each vertex's normal from the posed triangles around it (area-weighted; vertices whose
 * rest position and rest normal are bit-equal share one normal, so UV seams shade closed and hard edges stay hard) and re-orthogonalise
 * the tangent against it.  Position and tex_coord are unaffected. */
#define HALA_DEFORM_NORMALS_AS_POSED 0u
#define HALA_DEFORM_NORMALS_RECOMPUTED 1u
/* Switches the mode of the deformer on a primitive.  Mode 1 builds the adjacency tables from the rest pose on the host and uploads them;
 * mode 0 frees them (once a pose without them is on the device).  A call that changes the mode marks the deformer dirty: like every
 * edit it takes effect at the next hala_rt_refit, which poses the deformer again with its pending parameters; a call with the mode the
 * deformer already has does nothing.  A mode-1 refit under the identity pose does rewrite the normals from the triangles: it does not
 * give the rest normals back (mode 0, or hala_rt_clear_deformer, does).  The mode lives with the deformer: a replacing
 * hala_rt_set_deformer starts at mode 0, hala_rt_clear_deformer and hala_rt_set_scene drop it, a repeated hala_rt_commit keeps it.  The
 * deformers of a rig are switched one by one with this call after hala_rt_set_rig (hala_rig_binding::target_normal_deltas == NULL names
 * the ones that want it).  Refused, changing nothing, each with a message: no committed scene; the mesh or primitive does not exist;
 * the primitive has no deformer; a mode above HALA_DEFORM_NORMALS_RECOMPUTED; the deformer has shutter keys recorded or active ("clear
 * them and refit first"); an earlier device error left the vertex arena undefined ("set the scene again"). */
int hala_rt_set_deformer_normals(hala_rt_renderer* r, uint32_t mesh_index, uint32_t primitive_index, uint32_t mode);
typedef struct hala_deformer_normals_info {
  uint32_t mode;        /* as last set */
  uint32_t class_count; /* classes of the primitive's vertices; 0 in mode 0 */
  uint32_t entry_count; /* (triangle, corner) pairs in the classes' lists: 3 x triangles; 0 in mode 0 */
  uint32_t reserved;
  uint64_t launches;    /* launches of the two normals kernels by this renderer since hala_rt_create, all deformers: a pose adds 2 */
} hala_deformer_normals_info; /* 24 B */
/* Refused when there is no committed scene, the mesh or primitive does not exist, or the primitive has no deformer. */
int hala_rt_get_deformer_normals(hala_rt_renderer* r, uint32_t mesh_index, uint32_t primitive_index, hala_deformer_normals_info* out);

/* ------------------------------------------------------------------------------------------------
 * Shutter (docs/RENDER_SPEC.md 18; no reference equivalent): motion blur by accumulation.  Holders — a node's local transform, a
 * deformer's parameters, a primitive's vertices — carry two keys, the state at time 0 and at time 1.  While the shutter is on, frame k
 * of an accumulation renders the scene at the time of step k / time_stride, a stratified sequence over [shutter_open, shutter_close):
 * between two frames of different steps the library interpolates every keyed holder and refits the tree, without restarting the
 * accumulation.  All four setters are edits: they record on the host and take effect at the next hala_rt_refit, which leaves the
 * scene at step 0; until then updates render what they rendered and keep accumulating.  hala_rt_set_scene drops every key and the
 * shutter; hala_rt_commit keeps them.  A renderer that never sets a key or a shutter behaves exactly as before.
 * ---------------------------------------------------------------------------------------------- */
typedef struct hala_shutter_params {
  float shutter_open;   /* 0 <= shutter_open <= shutter_close <= 1 */
  float shutter_close;
  uint32_t time_stride; /* 1 ... 65536: consecutive frames that share one time */
  uint32_t reserved[5]; /* 0 */
} hala_shutter_params;  /* 32 B */
typedef struct hala_shutter_status {
  uint32_t enabled;     /* the shutter as the last hala_rt_refit applied it: 1 on, 0 off */
  uint32_t time_stride;
  uint32_t step;        /* the step the scene stands at; 0xFFFFFFFF: none (no key applied) */
  float time;           /* its time */
  uint64_t steps;       /* steps performed since hala_rt_create */
  uint32_t reserved[2];
} hala_shutter_status;  /* 32 B */
/* (0, 1, 1): the whole interval, a new time for every frame */
void hala_shutter_default_params(hala_shutter_params* out);
/* Records the shutter; NULL turns it off.  Takes effect at the next hala_rt_refit.  The time of step j is shutter_open + u_j *
 * (shutter_close - shutter_open) with u_j the base-2 radical inverse of j (24 bits).  The shutter is inactive — no step, no other
 * work on the update path — while it is off, while shutter_close == shutter_open, or while no holder has two keys that differ; a refit
 * then leaves the scene at time shutter_open (on) or 0 (off) for good.  While it is active, hala_rt_update_batch ends its chunks on
 * stride boundaries (the images equal those of single updates bit for bit), frames of one step overlap on the two frame slots as
 * always and frames of different steps do not, and an update whose step interpolates a position that is not finite fails with
 * "Vertex position is not finite.": nothing is rendered, the vertices and the tree are back at the previous step, the frame counter
 * stands.  Frames past max_frames take no step.  Ray batches, hala_rt_download_bvh, hala_rt_read_vertices and hala_rt_get_packed_*
 * see the scene at the step it stands at.  Refused, changing nothing: a NaN, shutter_open < 0, shutter_close > 1 or shutter_open >
 * shutter_close; time_stride outside 1 ... 65536; a reserved word that is not 0; temporal reprojection or adaptive sampling on (and
 * hala_rt_set_temporal / hala_rt_set_adaptive_sampling are refused while the shutter is on). */
int hala_rt_set_shutter(hala_rt_renderer* r, const hala_shutter_params* p);
/* the shutter and the step as the last hala_rt_refit and the updates since left them */
int hala_rt_get_shutter_status(hala_rt_renderer* r, hala_shutter_status* out);
/* Keys of a node's local transform (column-major 4 x 4, as hala_rt_update_node_transform takes it): any node of the committed scene,
 * so cameras and lights move too.  Both NULL clears the keys.  Takes effect at the next hala_rt_refit.  Setting keys makes the node's
 * local transform the open key; clearing leaves it there.  While a node has keys, hala_rt_update_node_transform on it is refused.
 * Refused, changing nothing: the node does not exist; one key NULL and one not; an entry that is not finite. */
int hala_rt_set_node_keys(hala_rt_renderer* r, uint32_t node_index, const float open[16], const float close[16]);
/* Keys of a deformer's pose: morph weights and / or joint matrices as hala_rt_update_deformer takes them, each part given for both
 * keys or for neither (that part then keeps the recorded pose at both ends); everything NULL clears the keys.  Takes effect at the
 * next hala_rt_refit.  Setting keys makes the open pose pending; clearing leaves it there.  Every weight and palette entry is
 * interpolated on the host, then k_deform poses the primitive from the rest pose as always.  While the keys are set,
 * hala_rt_update_deformer on the primitive is refused (and hala_rt_set_deformer / hala_rt_clear_deformer until a refit applied the
 * clearing).  Refused, changing nothing: the primitive has no deformer; one key of a part NULL and one not; weight_count differs
 * from the registered target_count or joint_count from the registered joint_count; a weight or matrix entry that is not finite. */
int hala_rt_set_deformer_keys(hala_rt_renderer* r, uint32_t mesh_index, uint32_t primitive_index, const float* weights_open,
                              const float* weights_close, uint32_t weight_count, const float* palette_open, const float* palette_close,
                              uint32_t joint_count);
/* Keys of a primitive's vertices, for a primitive without a deformer: position, normal and tangent are interpolated on the device
 * (k_shutter_lerp), tex_coord is the open key's.  Both keys are copied to the device before the call returns and stay there, 88 B
 * per vertex.  Both NULL clears the keys.  Takes effect at the next hala_rt_refit.  Setting keys acts as
 * hala_rt_update_vertices(open); clearing leaves the vertices there.  While the keys are set, hala_rt_update_vertices and
 * hala_rt_set_deformer on the primitive are refused.  Refused, changing nothing: the mesh or primitive does not exist; the primitive
 * has a deformer; one key NULL and one not; vertex_count differs from the primitive's; a position that is not finite.  Finite keys
 * can still overflow in between: hala_rt_refit (at step 0) or the update that takes the step then fails with "Vertex position is not
 * finite." and the vertices stay exactly as they were. */
int hala_rt_set_vertex_keys(hala_rt_renderer* r, uint32_t mesh_index, uint32_t primitive_index, const hala_vertex* open,
                            const hala_vertex* close, uint32_t vertex_count);

/* ------------------------------------------------------------------------------------------------
 * Node batches (docs/RENDER_SPEC.md 20; no reference equivalent): a crowd, a particle system or a rigid-body simulation binds its
 * nodes once and hands over one array of local transforms per frame, in host or in device memory.  hala_rt_refit_nodes(locals)
 * leaves the renderer in exactly the state that hala_rt_update_node_transform(indices[k], &locals[16 k]) for every k followed by
 * hala_rt_refit leaves it in: trees, instance references, bounds, packed primitives, images, the restarted accumulation, and the
 * behaviour of every later call.  Where it can, the library computes the node hierarchy and the instance transforms on the device
 * and runs its refits on them (the device path); otherwise it runs the ordinary sequence itself (the host path) and names the
 * reason in the status.  Both paths give the same bytes.
 * ---------------------------------------------------------------------------------------------- */
#define HALA_NODE_REFIT_PATH_NONE 0u
#define HALA_NODE_REFIT_PATH_DEVICE 1u
#define HALA_NODE_REFIT_PATH_HOST 2u
/* hala_node_refit_status::last_reason: why the host path was taken */
#define HALA_NODE_REFIT_PENDING_EDIT 1u    /* an edit waits for a refit: a node moved by another call, a material, vertices, a deformer,
                                              build options set since the trees were built */
#define HALA_NODE_REFIT_SHUTTER_KEYS 2u    /* shutter keys are recorded or active */
#define HALA_NODE_REFIT_CAMERA_OR_LIGHT 3u /* a camera or a light hangs at or below a bound node */
#define HALA_NODE_REFIT_HOST_LEVELS 4u     /* a two-level tree whose instance levels are built on the host (instance_levels = 0) */
#define HALA_NODE_REFIT_CLASSIFICATION 5u  /* a transform stopped being invertible, or is again: the trees are built anew */
typedef struct hala_node_refit_status {
  uint32_t bound_nodes, affected_nodes, affected_instances, levels; /* the binding: nodes bound; they and all below them; their
                                                                       instances; depth levels among the affected nodes */
  uint32_t last_path;   /* HALA_NODE_REFIT_PATH_*: of the last hala_rt_refit_nodes */
  uint32_t last_reason; /* why the host path was taken; 0 on the device path */
  unsigned long long device_refits, host_refits; /* calls by path since hala_rt_create */
} hala_node_refit_status; /* 40 B */
/* Binds an ordered set of nodes of the committed scene; node_indices NULL or count 0 unbinds.  The host analyses the set once — the
 * bound nodes and all their descendants by depth, their instances and the tree each sits in, whether a camera or a light rides
 * along — and uploads the tables.  hala_rt_set_scene and hala_rt_commit drop the binding.  Refused, changing nothing: no committed
 * scene; an index that does not exist; an index given twice; a node with shutter keys (hala_rt_update_node_transform's message). */
int hala_rt_bind_nodes(hala_rt_renderer* r, const uint32_t* node_indices, uint32_t count);
/* locals: one column-major 4 x 4 per bound node, in the bound order, as hala_rt_update_node_transform takes it.  where: 0 host
 * memory, 1 device memory of the renderer's device.  A device array is read on the renderer's stream (hala_rt_get_stream) behind the
 * join and the wait that hala_rt_refit performs: the caller produces it on that stream, orders its producer against it, or
 * synchronises before the call; the array may be reused when the call returns.  Refused, changing nothing: no committed scene;
 * nothing bound; locals NULL; a bound node that has got shutter keys since.  A call that fails later fails where hala_rt_refit
 * would: the recorded locals and the instance records are the new ones, the trees are not fitted to them and the status does not
 * count the call; the next successful hala_rt_refit, hala_rt_refit_nodes or hala_rt_commit fits them. */
int hala_rt_refit_nodes(hala_rt_renderer* r, const float* locals, int where);
int hala_rt_get_node_refit_status(hala_rt_renderer* r, hala_node_refit_status* out);
#define HALA_NODE_REFIT_POLICY_REBUILD 6u  /* last_reason beside the five above: the device path posed and refitted, the refit policy
                                              (below) then found a rebuild due and the trees were built anew, as hala_rt_refit would */

/* ------------------------------------------------------------------------------------------------
 * Tree quality and the refit policy (docs/RENDER_SPEC.md 4.6; no reference equivalent).  hala_rt_refit keeps the topology the last
 * build gave the tree and only re-derives its boxes; far from the pose it was built for the boxes grow and overlap, images stay
 * what they are and rays cost more.  The tree cost of RENDER_SPEC 4.6 — computed on the device from the published node format
 * alone (k_tree_cost), reproducible from hala_rt_download_bvh — tells, and a policy may build the trees anew when it has grown.
 * A tree: the whole node array of a one-level scene; of a two-level scene the world tree and each object-space tree (the instance
 * levels are built anew by every refit and are not measured).
 * ---------------------------------------------------------------------------------------------- */
#define HALA_REFIT_POLICY_OFF 0u          /* never measure, never rebuild: the default */
#define HALA_REFIT_POLICY_THRESHOLD 1u    /* measure; rebuild when a refitted tree's inflation exceeds max_inflation */
#define HALA_REFIT_POLICY_ALWAYS 2u       /* measure; rebuild at every refit that refitted a tree */
#define HALA_REFIT_POLICY_MEASURE 3u      /* measure only */
typedef struct hala_refit_policy {
  uint32_t mode;          /* HALA_REFIT_POLICY_* */
  float max_inflation;    /* mode 1: finite, >= 1; every other mode: must be 0.  inflation = cost_now / cost_built in double, cost =
                             node_q + tri_q.  There is no default on purpose.  Measured once (DESIGN.md 23,
                             profiles/tree_quality_timing.json: 1.0 M triangles, a 120 k-triangle floor displaced by noise, 1080p, a
                             rebuild of 18 - 21 ms against a refit of 0.4 ms): a rebuild repaid itself within about 80 frames
                             from inflation 2.3, 40 from 8.8, 10 from 60; above 200 the geometry itself had become the cost and
                             a rebuild won nothing.  For any other scene the value is unmeasured: measure with mode 3 first. */
  uint32_t reserved[2];   /* 0 */
} hala_refit_policy; /* 16 B */
/* Takes effect at once: on a committed renderer with mode != 0 whose trees are not yet measured, the trees as they stand are measured
 * and become the baseline (built = now); mode 0 forgets the numbers (the two counters stay).  Refused, changing nothing and doing no
 * device work: policy NULL; mode > 3; mode 1 with max_inflation not finite or < 1; another mode with max_inflation != 0; a reserved
 * word != 0. */
int hala_rt_set_refit_policy(hala_rt_renderer* r, const hala_refit_policy* policy);
typedef struct hala_tree_quality {
  uint32_t first_node, node_count; /* the tree: nodes [first_node, first_node + node_count) of hala_rt_download_bvh, root first */
  uint32_t valid;                  /* 0: the root box has no area; all sums 0, never rebuilt by the policy */
  uint32_t rebuilt_last_refit;     /* 1: the last hala_rt_refit / hala_rt_refit_nodes built this tree anew because the policy said so */
  unsigned long long node_q_built, tri_q_built; /* RENDER_SPEC 4.6, units of 2^-32: right after the tree was last built */
  unsigned long long node_q_now, tri_q_now;     /* ... and after the last refit that refitted it */
} hala_tree_quality; /* 48 B */
/* With mode != 0: hala_rt_commit and every rebuild measure the trees they built (built = now); hala_rt_refit and hala_rt_refit_nodes
 * measure every tree they refitted (now), then apply the policy: a rebuild builds ALL trees of the scene anew (build options that
 * wait take effect, as when a refit reclassifies instances) and invalidates what that rebuild invalidates.  A refit that moved only
 * cameras, lights or nodes of instanced primitives refits no tree and measures nothing; a step of the shutter never measures.
 * dst may be NULL; at most `capacity` trees are written, *tree_count is the number there are (0 with mode 0 or before a commit);
 * refits_measured: refits that measured at least one tree; trees_rebuilt_by_policy: trees built anew by policy rebuilds; both since
 * hala_rt_create.  Any of the three pointers may be NULL. */
int hala_rt_get_tree_quality(hala_rt_renderer* r, hala_tree_quality* dst, uint32_t capacity, uint32_t* tree_count,
                             unsigned long long* refits_measured, unsigned long long* trees_rebuilt_by_policy);

/* ------------------------------------------------------------------------------------------------
 * Rigs and clips (docs/RENDER_SPEC.md 19): a hala_rig_desc drives the deformers, node transforms and shutter keys above.
 * ---------------------------------------------------------------------------------------------- */
typedef struct hala_rig_status {
  uint32_t bindings;       /* of the rig hala_rt_set_rig registered; 0: none */
  uint32_t deformers;      /* deformers registered on the renderer, by hala_rt_set_rig or hala_rt_set_deformer */
  uint64_t pose_launches;  /* kernel launches that posed deformers, since hala_rt_create */
  uint64_t segments_posed; /* deformers those launches posed: one launch poses all the dirty ones of a refit */
  uint64_t batch_launches; /* those among pose_launches that posed two or more deformers */
} hala_rig_status; /* 32 B */
/* Registers one deformer (hala_rt_set_deformer) per binding of `rig` on the committed scene and keeps a copy of the rig's tables; the
 * caller's arrays may go.  NULL clears the rig: the deformers it registered (one that the host cleared or replaced since stays the
 * host's), the shutter keys hala_rt_key_rig set, and the nodes its poses moved, which go back to the file's transforms at the next
 * hala_rt_refit; it is refused, changing nothing, while one of its deformers has shutter keys that a refit has not yet cleared
 * (hala_rt_key_rig with HALA_INVALID_INDEX, then hala_rt_refit, first).  Refused, changing nothing, with a message that names
 * the mesh and primitive: a binding above HALA_MAX_JOINTS or HALA_MAX_MORPH_TARGETS; a bound mesh that more than one node
 * instantiates (the posed vertices are per primitive, not per instance); node, mesh, primitive, skin or vertex counts that do not
 * fit the committed scene; a primitive that already has a deformer or shutter vertex keys; a rig is set already (clear it first).
 * hala_rt_set_scene drops the rig with the deformers. */
int hala_rt_set_rig(hala_rt_renderer* r, const hala_rig_desc* rig);
/* Records the pose of clip `clip` at `time` (hala_rig_sample_clip): hala_rt_update_node_transform for every node a channel of the
 * clip touches and hala_rt_update_deformer for every binding; a node that an earlier pose of the rig wrote and this clip does not
 * touch goes back to the file's transform, so the scene stands at the pose hala_rt_get_rig_pose reports.  clip ==
 * HALA_INVALID_INDEX: the file's own pose, on every node any clip touches.  Takes effect at the next hala_rt_refit.  Refused, changing nothing: no rig; the clip does not exist; a singular
 * mesh node; a touched node or a binding's deformer that has shutter keys; a binding whose deformer the host cleared or replaced. */
int hala_rt_pose_rig(hala_rt_renderer* r, uint32_t clip, float time);
/* Evaluates the clip at t_open and t_close and sets the results as shutter keys (hala_rt_set_node_keys on the touched nodes,
 * hala_rt_set_deformer_keys on the bindings): with hala_rt_set_shutter the refit and the frames after it blur the clip over that
 * interval.  clip == HALA_INVALID_INDEX clears the keys this call set.  Refused, changing nothing, as hala_rt_pose_rig is. */
int hala_rt_key_rig(hala_rt_renderer* r, uint32_t clip, float t_open, float t_close);
/* What the last hala_rt_pose_rig (key 0) or hala_rt_key_rig (key 0: open, key 1: close) recorded, laid out as
 * hala_rig_sample_clip's outputs; each may be NULL.  *clip and *time receive what that call was given.  Refused before the first. */
int hala_rt_get_rig_pose(hala_rt_renderer* r, uint32_t key, uint32_t* clip, float* time, float* locals, float* weights, float* palettes);
int hala_rt_get_rig_status(hala_rt_renderer* r, hala_rig_status* out);

/* ------------------------------------------------------------------------------------------------
 * Denoising (docs/RENDER_SPEC.md 10; no reference equivalent): an edge-avoiding a-trous wavelet filter over the running
 * means, guided by the first-hit albedo and normal AOVs.  Opt-in: nothing is allocated for a renderer that never denoises.
 * ---------------------------------------------------------------------------------------------- */
typedef struct hala_denoise_params {
  uint32_t iterations;   /* N, 1..8: pass i gathers 5 x 5 taps 2^i pixels apart */
  float sigma_color;     /* colour tolerance of pass 0 (halves with each pass), in [1e-6, 1e6] */
  float sigma_albedo;    /* albedo tolerance, in [1e-6, 1e6] */
  uint32_t normal_power; /* exponent of the normal weight: a power of two, 1..128 */
  uint32_t demodulate;   /* 1: filter radiance / albedo and multiply the albedo back; 0: filter the radiance itself */
  uint32_t reserved[3];  /* must be zero */
} hala_denoise_params;   /* 32 B */
/* the defaults (DESIGN.md "Denoising" records the measurements behind them) */
void hala_denoise_default_params(hala_denoise_params* out);
/* Filters the renderer's accum / albedo / normal into its denoised image (RGBA32F, alpha 1).  Stream-ordered on the renderer's
 * stream behind the updates enqueued so far; returns without waiting when gpu_ms is NULL, else times its own launches with HIP
 * events, waits and stores the milliseconds.  Writes none of the four images.  Refused: no sample accumulated since creation,
 * hala_rt_reset_accumulation or hala_rt_set_tile_shard; a sharded renderer (world > 1) whose AOVs 0, 1 and 2 have not all been
 * gathered since the last update (then the gathered frame is filtered).  Parameters are validated before any device call. */
int hala_rt_denoise(hala_rt_renderer* r, const hala_denoise_params* p, float* gpu_ms);
/* the last denoised image: W*H*4 floats, linear, row 0 = top */
int hala_rt_read_denoised(hala_rt_renderer* r, float* dst_rgba32f);
/* zero-copy: its device address and byte size (valid until the next hala_rt_denoise that changes the size, or destroy) */
int hala_rt_get_denoised_buffer(hala_rt_renderer* r, void** d_ptr, size_t* bytes);
/* <stem>_denoised.pfm beside what save_images writes, tonemapped on the host like <stem>_color.pfm */
int hala_rt_save_denoised(hala_rt_renderer* r, const char* path);
/* the same filter on host images (e.g. the PFM trio of save_images, as hala_load_float_image reads it, widened to RGBA32F):
 * color / albedo / normal / dst are W*H*4 floats, row 0 = top.  Parameters are validated before any device call. */
int hala_denoise_images(int device_ordinal, const float* color, const float* albedo, const float* normal, uint32_t width,
                        uint32_t height, const hala_denoise_params* p, float* dst);

/* ------------------------------------------------------------------------------------------------
 * Adaptive sampling (docs/RENDER_SPEC.md 11; no reference equivalent): the 8 x 8 pixel blocks whose running mean has converged stop
 * being traced until the accumulation restarts.  Opt-in: nothing is allocated and no image changes for a renderer that never enables it.
 * ---------------------------------------------------------------------------------------------- */
typedef struct hala_adaptive_status {
  uint32_t enabled, active_blocks, total_blocks, active_pixels;
  uint32_t samples;       /* n: frames folded into the active blocks */
  uint32_t last_snapshot; /* s */
  uint32_t reserved[2];
} hala_adaptive_status;   /* 32 B */
typedef struct hala_adaptive_params {
  float threshold;        /* finite, > 0: a block converges when every pixel's error estimate is below it */
  uint32_t min_samples;   /* 2 ... 65536: the first check (the snapshot is taken at min_samples / 2) */
  uint32_t interval;      /* 1 ... 65536: samples between two checks */
  uint32_t reserved[5];   /* 0 */
} hala_adaptive_params;   /* 32 B */
/* the defaults (DESIGN.md "Adaptive sampling" records the measurements behind them) */
void hala_adaptive_default_params(hala_adaptive_params* out);
/* p: enable with these parameters; NULL: off.  Either way the accumulation restarts.  Refused, with the renderer left as it was:
 * invalid parameters (checked before the handle is looked at), a sharded renderer (world > 1), a renderer with several views
 * (hala_rt_set_views), a build with another pixel block size.
 * The first call that enables allocates the snapshot image and the block lists.  An update that ends on a check frame
 * (n = min_samples + j * interval) waits for the check and reads two counts back; every other update stays asynchronous. */
int hala_rt_set_adaptive_sampling(hala_rt_renderer* r, const hala_adaptive_params* p);
/* W*H uint32, row-major: the samples folded into each pixel (with the feature off: the frames rendered since the accumulation started) */
int hala_rt_read_sample_counts(hala_rt_renderer* r, uint32_t* dst);
/* active / total blocks, active in-frame pixels, n and s */
int hala_rt_get_adaptive_status(hala_rt_renderer* r, hala_adaptive_status* out);

/* ------------------------------------------------------------------------------------------------
 * Temporal reprojection (docs/RENDER_SPEC.md 16; no reference equivalent): carries the accumulated frame across a scene edit.
 * hala_rt_temporal_capture keeps the frame as the history before an edit; after hala_rt_refit and a few new samples,
 * hala_rt_temporal_resolve reprojects the history through the captured camera and instance transforms, validates each tap against ids and
 * position, and blends it with the new samples by sample count.  A frame-space pass beside the integrator: images 0-5, statistics and
 * the existing refusals are the same with the feature on or off, and nothing is allocated for a renderer that never enables it.
 *
 *   hala_rt_set_aovs(r, 3); hala_rt_set_temporal(r, &params);
 *   ... updates ...   hala_rt_temporal_capture(r);                       // before the edit
 *   hala_rt_update_node_transform(...); hala_rt_refit(r);                 // the accumulation restarts
 *   hala_rt_update_batch(r, 4); hala_rt_temporal_resolve(r, NULL);        // 4 new samples + the reprojected history
 *   hala_rt_read_temporal(r, 0, dst);  or  hala_rt_denoise_temporal(r, &dp, NULL);
 * ---------------------------------------------------------------------------------------------- */
typedef struct hala_temporal_params {
  float max_history;    /* the history length (in samples) a pixel may carry over, in [1, 2^20]: bounds the lag of indirect light */
  float tol;            /* a tap is kept when its stored position lies within tol * (view depth) of the reprojected point, in [1e-6, 1] */
  float min_weight;     /* the least bilinear weight the valid taps must add up to, in (0, 1] */
  uint32_t reserved[5]; /* must be zero */
} hala_temporal_params; /* 32 B */
/* the defaults of RENDER_SPEC 16 (DESIGN.md "Temporal reprojection" records what stands behind them) */
void hala_temporal_default_params(hala_temporal_params* out);
/* RENDER_SPEC 16: p enables the feature with these parameters (a second call only replaces them and keeps the history); NULL turns it
 * off and frees its buffers.  Does not restart the accumulation.  Refused, with the renderer left as it was: invalid parameters (checked
 * before the handle is looked at), a sharded renderer (world > 1), several views, adaptive sampling on.  While the feature is on,
 * hala_rt_set_views with several views, hala_rt_set_adaptive_sampling with parameters and hala_rt_set_tile_shard with world > 1 are
 * refused in turn. */
int hala_rt_set_temporal(hala_rt_renderer* r, const hala_temporal_params* p);
/* RENDER_SPEC 16 "Vertex motion": enable != 0 lets the history follow vertex edits (hala_rt_update_vertices, posed deformers) on a
 * one-level tree.  From then on every capture also keeps the triangles in id order as they stand (one device-to-device copy of 48 B per
 * triangle on the renderer's stream, allocated by the first such capture), and a resolve carries a pixel of an edited primitive by the
 * barycentrics of its mean hit point on its triangle, placed on the same triangle of the capture.  On a two-level tree, with a history
 * captured before the call, or with enable = 0 (which frees the kept triangles) such a primitive starts without history as it always
 * did.  Off by default and turned off by hala_rt_set_temporal(r, NULL).  Does not restart the accumulation.  Refused, with the renderer
 * left as it was, while temporal reprojection is off. */
int hala_rt_set_temporal_vertex_motion(hala_rt_renderer* r, int enable);
typedef struct hala_temporal_clamp_params {
  uint32_t radius;      /* the neighbourhood is (2 radius + 1)^2 pixels of the current accumulation, radius in {1, 2, 3} */
  float gamma;          /* the history may lie within gamma standard errors of the neighbourhood mean, finite, in (0, 1000] */
  uint32_t reserved[2]; /* must be zero */
} hala_temporal_clamp_params; /* 16 B */
/* the defaults of RENDER_SPEC 16 "History clamp" (DESIGN.md "History clamp" has the sweep behind them) */
void hala_temporal_clamp_default_params(hala_temporal_clamp_params* out);
/* RENDER_SPEC 16 "History clamp": p makes every resolve (and so every capture) clamp the reprojected history colour of a pixel, per
 * channel, to mean +- gamma standard errors of the current accumulation over the pixel's (2 radius + 1)^2 neighbourhood before it is
 * blended, so that light the edit changed does not lag by max_history samples; NULL turns the clamp off, and every output is then bit
 * for bit what it is without this call.  History length, sample counts, the motion image and pixels without history are the same
 * either way.  Off by default and turned off by hala_rt_set_temporal(r, NULL).  Does not restart the accumulation, does not drop the
 * history and allocates nothing.  Refused, with the renderer left as it was: invalid parameters (checked before the handle is looked
 * at), temporal reprojection off. */
int hala_rt_set_temporal_clamp(hala_rt_renderer* r, const hala_temporal_clamp_params* p);
/* RENDER_SPEC 16 "Capture": call it before editing the scene.  With samples folded since the last restart it resolves, then keeps the
 * resolved image, images 4 and 5, view 0's packed camera and every instance's world transform as the history (device-to-device copies on
 * the renderer's stream) and clears the edit marks; with none (two edits without a frame between) it succeeds and keeps the history it
 * has.  Refused: the feature is off, AOV bits 0 and 1 are not both on. */
int hala_rt_temporal_capture(hala_rt_renderer* r);
/* RENDER_SPEC 16 "Resolve": view 0's accumulation blended with the reprojected history into the temporal image, and the motion image.
 * Stream-ordered behind the updates enqueued so far; returns without waiting when gpu_ms is NULL, else times its launch with HIP events,
 * waits and stores the milliseconds.  Without a history every pixel is the accumulation with its sample count.  Writes none of images
 * 0-5.  Refused: the feature is off, AOV bits 0 and 1 are not both on, no sample folded since the accumulation restarted. */
int hala_rt_temporal_resolve(hala_rt_renderer* r, float* gpu_ms);
/* RENDER_SPEC 16 "Outputs": which = 0 the temporal image (rgb, history length + samples), 1 the motion image (dx, dy in pixels towards
 * the history, view depth in the captured camera, 1; all 0 where nothing was reprojected); W*H*4 floats, row 0 = top.  Refused before
 * the first resolve. */
int hala_rt_read_temporal(hala_rt_renderer* r, int which, float* dst_rgba32f);
/* RENDER_SPEC 16 "Outputs", zero-copy: the device address and byte size of the same images (valid until hala_rt_set_temporal(r, NULL)
 * or destroy); reads of it belong on the renderer's stream */
int hala_rt_get_temporal_buffer(hala_rt_renderer* r, int which, void** d_ptr, size_t* bytes);
/* RENDER_SPEC 16 "Denoising": the filter of hala_rt_denoise (RENDER_SPEC 10) with the temporal image of the last resolve as colour and the
 * current albedo / normal as guides; the result goes to the denoised image (hala_rt_read_denoised).  Refused before the first resolve. */
int hala_rt_denoise_temporal(hala_rt_renderer* r, const hala_denoise_params* p, float* gpu_ms);

/* ------------------------------------------------------------------------------------------------
 * Stand-alone pieces of the path (usable without a renderer)
 * ---------------------------------------------------------------------------------------------- */
/* EnvMap::build_distribution_maps (src/envmap.rs:239-388) on the GPU. pixels: RGBA32F host, W*H*4. */
int hala_envmap_build_distribution(int device_ordinal, const float* rgba32f, uint32_t width,
                                   uint32_t height, float* total_sum, float* marginal,
                                   float* conditional);
/* save_images' host tonemap (src/rt_renderer.rs:1256-1316) applied in place to RGBA32F pixels. */
void hala_tonemap_pixels(float* rgba32f, size_t pixel_count, int enable_tonemap, int enable_aces,
                         int use_simple_aces);
/* The decoder behind hala_rt_set_envmap_file (`image::open(path)` of src/envmap.rs:48-53 for the float formats): fills
 * width / height / channels (3 or 4); copies the row-0-is-top float pixels into dst when dst != NULL and capacity_floats
 * is large enough.  No GPU involved. */
int hala_load_float_image(const char* path, uint32_t* width, uint32_t* height, uint32_t* channels, float* dst,
                          size_t capacity_floats);
/* save_images' PFM writer (src/rt_renderer.rs:1318-1334). */
int hala_write_pfm(const char* path, const float* rgba32f, uint32_t width, uint32_t height);
/* Cryptomatte name hashing (docs/RENDER_SPEC.md 15), no GPU involved: raw = MurmurHash3_x86_32 of the bytes of `name`, seed 0; id = raw
 * with bit 23 flipped when its exponent bits are 0 or 255 (either output may be NULL). */
int hala_cryptomatte_hash(const char* name, uint32_t* raw, uint32_t* id);
/* The OpenEXR writer of hala_rt_save_cryptomatte, no GPU involved: single-part scanline OpenEXR 2.0, ZIP compression (16 lines per block;
 * a block that does not shrink is stored as it is), every channel FLOAT and written in ascending byte order of the names whatever the
 * order given; planes[c] holds channel c's W*H floats, row 0 = top.  attr_names / attr_values: string attributes.  Refused: no channel, a
 * null or empty name, duplicate names, a name longer than 255 bytes, a size of W or H outside 1..2^20, blocks of 2^31 bytes or more, an
 * attribute named like one of the header attributes the writer sets itself. */
int hala_write_exr(const char* path, uint32_t width, uint32_t height, uint32_t channel_count, const char* const* channel_names,
                   const float* const* planes, uint32_t attribute_count, const char* const* attr_names, const char* const* attr_values);

/* HalaRayTracingProgramDesc (src/raytracing_program.rs:25-55): parses the serde JSON field names and
 * defaults; returns the parsed counts (used by the host mirror of HalaRayTracingProgram::new). */
typedef struct hala_rtprog_desc_info {
  uint32_t raygen_count;
  uint32_t miss_count;
  uint32_t hit_count;
  uint32_t callable_count;
  uint32_t push_constant_size;
  uint32_t binding_count;
  uint32_t ray_recursion_depth;
} hala_rtprog_desc_info;
int hala_rtprog_parse_desc(const char* desc_json, hala_rtprog_desc_info* out);

/* HalaRayTracingProgram (src/raytracing_program.rs:70-341), one export per method: the generic "RT pass" object an application
 * builds beside the renderer.  The shader paths of the description are recorded (SPIR-V has no meaning for the HIP kernels), the
 * pipeline is the library's traversal kernel pair, bind() takes the device buffers of one ray batch where the reference takes
 * descriptor sets, and bytes 0..3 of the push-constant block select the hit group: 0 closest hit, 1 any hit.
 *   hala_rtprog_create              <- HalaRayTracingProgram::new (:85-252): desc_json = the serde form of HalaRayTracingProgramDesc
 *                                      (:33-55); the renderer supplies device + acceleration structure (logical_device and
 *                                      descriptor_set_layouts there); fails on a parse error or an empty raygen list
 *   hala_rtprog_bind                <- bind (:264-278)
 *   hala_rtprog_push_constants{,_f32} <- push_constants / push_constants_f32 (:285-322): offset + length must lie inside
 *                                      push_constant_size (at least 4 bytes are kept for the mode word)
 *   hala_rtprog_trace_rays          <- trace_rays(index, command_buffers, width, height, depth) (:330-332): width*height*depth rays of
 *                                      the bound batch; hip_stream as in hala_rt_trace_rays (the command buffer of the reference)
 *   hala_rtprog_trace_rays_indirect <- trace_rays_indirect (:338-340): device-resident {width, height, depth}
 * The program borrows the renderer: destroy it before the renderer. */
typedef struct hala_rtprog hala_rtprog;
int hala_rtprog_create(hala_rt_renderer* r, const char* desc_json, const char* debug_name, hala_rtprog** out);
void hala_rtprog_destroy(hala_rtprog* p);
int hala_rtprog_get_desc_info(const hala_rtprog* p, hala_rtprog_desc_info* out);
int hala_rtprog_bind(hala_rtprog* p, const hala_ray* d_rays, hala_hit* d_hits);
int hala_rtprog_push_constants(hala_rtprog* p, uint32_t offset, const void* data, size_t len);
int hala_rtprog_push_constants_f32(hala_rtprog* p, uint32_t offset, const float* data, size_t count);
int hala_rtprog_trace_rays(hala_rtprog* p, uint32_t width, uint32_t height, uint32_t depth, void* hip_stream);
int hala_rtprog_trace_rays_indirect(hala_rtprog* p, const uint32_t* d_indirect, void* hip_stream);
/* hala_rt_trace_rays_multi on the bound batch: width*height*depth rays, k records each (the bound hit buffer holds that many).  The
 * constant block is not consulted: word 0 keeps selecting the behaviour of hala_rtprog_trace_rays only. */
int hala_rtprog_trace_rays_multi(hala_rtprog* p, uint32_t width, uint32_t height, uint32_t depth, uint32_t k, uint32_t* d_counts, void* hip_stream);

const char* hala_version(void);

#ifdef __cplusplus
}
#endif
#endif /* HALART_H */
