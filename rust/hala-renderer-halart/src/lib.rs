//! `HalaRenderer` / `HalaRayTracingProgram` over libhalart.so — the same public names, argument meaning and error type
//! as hala-renderer's ray-tracing renderer (`src/rt_renderer.rs`, `src/raytracing_program.rs`, `src/error.rs`), so an
//! application written against the reference switches by changing one `use`.
//!
//! SOURCE ONLY — never compiled: the build container has no Rust toolchain.  Every `extern "C"`
//! declaration below is a line-for-line transcription of `include/halart.h`; the ctypes twin of this file
//! (`hala-renderer_amd/renderer.py`) is what the test-suite exercises against the same library.
#![allow(non_camel_case_types)]

use std::ffi::{CStr, CString};
use std::os::raw::{c_char, c_int, c_void};
use std::path::Path;

pub mod sys {
  use super::*;

  #[repr(C)] pub struct hala_rt_renderer { _private: [u8; 0] }

  /// src/scene/vertex.rs:2-9 (44 B)
  #[repr(C)] #[derive(Clone, Copy)]
  pub struct hala_vertex { pub position: [f32; 3], pub normal: [f32; 3], pub tangent: [f32; 3], pub tex_coord: [f32; 2] }

  #[repr(C)] pub struct hala_node_desc {
    pub name: *const c_char, pub parent: i32, pub local_transform: [f32; 16],
    pub mesh_index: u32, pub camera_index: u32, pub light_index: u32,
  }
  #[repr(C)] pub struct hala_primitive_desc {
    pub indices: *const u32, pub index_count: u32, pub vertices: *const hala_vertex, pub vertex_count: u32, pub material_index: u32,
  }
  #[repr(C)] pub struct hala_mesh_desc { pub primitives: *const hala_primitive_desc, pub primitive_count: u32 }
  #[repr(C)] pub struct hala_material_desc {
    pub type_: u32, pub base_color: [f32; 3], pub opacity: f32, pub emission: [f32; 3], pub anisotropic: f32, pub metallic: f32,
    pub roughness: f32, pub subsurface: f32, pub specular_tint: f32, pub sheen: f32, pub sheen_tint: f32, pub clearcoat: f32,
    pub clearcoat_roughness: f32, pub clearcoat_tint: [f32; 3], pub specular_transmission: f32, pub ior: f32,
    pub medium_type: u32, pub medium_color: [f32; 3], pub medium_density: f32, pub medium_anisotropy: f32,
    pub base_color_map_index: u32, pub emission_map_index: u32, pub normal_map_index: u32, pub metallic_roughness_map_index: u32,
  }
  #[repr(C)] pub struct hala_light_desc { pub color: [f32; 3], pub intensity: f32, pub light_type: u32, pub param0: f32, pub param1: f32 }
  #[repr(C)] pub struct hala_camera_desc {
    pub type_: u32, pub aspect: f32, pub yfov: f32, pub znear: f32, pub zfar: f32, pub focal_distance: f32, pub aperture: f32, pub xmag: f32, pub ymag: f32,
  }
  /// docs/RENDER_SPEC.md 14 (32 B): packed light / material / environment -> light group
  #[repr(C)] pub struct hala_light_groups {
    pub group_count: u32, pub environment_group: u32, pub light_count: u32, pub material_count: u32,
    pub light_group: *const u32, pub material_group: *const u32,
  }
  /// docs/RENDER_SPEC.md 15 (24 B): layer_mask bit 0 object, bit 1 material, bit 2 asset
  #[repr(C)] pub struct hala_cryptomatte_desc {
    pub layer_mask: u32, pub material_name_count: u32, pub material_names: *const *const c_char, pub reserved: [u32; 2],
  }
  #[repr(C)] pub struct hala_image_desc { pub format: u32, pub width: u32, pub height: u32, pub data: *const c_void, pub num_of_bytes: usize }
  #[repr(C)] pub struct hala_index_pair { pub key: u32, pub value: u32 }
  #[repr(C)] pub struct hala_scene_desc {
    pub nodes: *const hala_node_desc, pub node_count: u32,
    pub meshes: *const hala_mesh_desc, pub mesh_count: u32,
    pub materials: *const hala_material_desc, pub material_count: u32,
    pub lights: *const hala_light_desc, pub light_count: u32,
    pub cameras: *const hala_camera_desc, pub camera_count: u32,
    pub texture2image_mapping: *const hala_index_pair, pub texture_count: u32,
    pub image2data_mapping: *const hala_index_pair, pub image_count: u32,
    pub image_data: *const hala_image_desc, pub image_data_count: u32,
  }
  #[repr(C)] #[derive(Clone, Copy)] pub struct hala_ray { pub origin: [f32; 3], pub tmin: f32, pub direction: [f32; 3], pub tmax: f32 }
  #[repr(C)] #[derive(Clone, Copy)] pub struct hala_hit { pub t: f32, pub u: f32, pub v: f32, pub prim: u32 }
  /// hala_point_query (16 B) / hala_closest_point (32 B): closest-point query batches (include/halart.h, docs/RENDER_SPEC.md 4.8)
  #[repr(C)] #[derive(Clone, Copy)] pub struct hala_point_query { pub point: [f32; 3], pub radius: f32 }
  #[repr(C)] #[derive(Clone, Copy)] pub struct hala_closest_point { pub distance: f32, pub u: f32, pub v: f32, pub prim: u32, pub point: [f32; 3], pub region: u32 }
  /// hala_distance_grid_desc (36 B): signed distance grids (include/halart.h, docs/RENDER_SPEC.md 4.9); flags: bit 0 signed, bits 1-2 method
  #[repr(C)] #[derive(Clone, Copy)] pub struct hala_distance_grid_desc { pub origin: [f32; 3], pub spacing: f32, pub dims: [u32; 3], pub band: f32, pub flags: u32 }
  /// hala_occlusion_sample (32 B) / hala_occlusion (16 B): occlusion batches (include/halart.h, docs/RENDER_SPEC.md 4.10)
  #[repr(C)] #[derive(Clone, Copy)] pub struct hala_occlusion_sample { pub point: [f32; 3], pub bias: f32, pub normal: [f32; 3], pub reach: f32 }
  #[repr(C)] #[derive(Clone, Copy)] pub struct hala_occlusion { pub visibility: f32, pub bent: [f32; 3] }
  /// hala_bake_desc (28 B) / hala_bake_texel (16 B): bake maps (include/halart.h, docs/RENDER_SPEC.md 4.11); flags: HALA_BAKE_*
  #[repr(C)] #[derive(Clone, Copy)] pub struct hala_bake_desc { pub instance: u32, pub width: u32, pub height: u32, pub flags: u32, pub bias: f32, pub reach: f32, pub margin: u32 }
  #[repr(C)] #[derive(Clone, Copy)] pub struct hala_bake_texel { pub u: f32, pub v: f32, pub prim: u32, pub source: u32 }
  /// hala_bake_chart (24 B) / hala_bake_atlas_desc (24 B): bake atlases (include/halart.h, docs/RENDER_SPEC.md 4.12); flags: HALA_BAKE_*, per chart
  #[repr(C)] #[derive(Clone, Copy)] pub struct hala_bake_chart { pub instance: u32, pub flags: u32, pub scale: [f32; 2], pub offset: [f32; 2] }
  #[repr(C)] #[derive(Clone, Copy)] pub struct hala_bake_atlas_desc { pub width: u32, pub height: u32, pub bias: f32, pub reach: f32, pub margin: u32, pub chart_count: u32 }
  /// hala_bake_transfer_desc (16 B) / hala_bake_transfer_hit (32 B): transfer bakes (include/halart.h, docs/RENDER_SPEC.md 4.13); flags: 0
  #[repr(C)] #[derive(Clone, Copy)] pub struct hala_bake_transfer_desc { pub front: f32, pub back: f32, pub flags: u32, pub target_count: u32 }
  #[repr(C)] #[derive(Clone, Copy)] pub struct hala_bake_transfer_hit { pub t: f32, pub u: f32, pub v: f32, pub prim: u32, pub normal: [f32; 3], pub height: f32 }
  #[repr(C)] #[derive(Default)] pub struct hala_rt_info { pub width: u32, pub height: u32 }

  /// hala_rt_build_options (include/halart.h): every field 0 = the default
  #[repr(C)] #[derive(Default, Clone, Copy)]
  pub struct hala_rt_build_options { pub builder: u32, pub ploc_tail: u32, pub ploc_look_every: u32, pub collapse_look_every: u32, pub instancing: u32, pub texture_bundles: u32, pub instance_levels: u32, pub reserved: [u32; 1] }
  /// hala_temporal_params (include/halart.h, docs/RENDER_SPEC.md 16; 32 B): fill it with hala_temporal_default_params
  #[repr(C)] #[derive(Default, Clone, Copy)]
  pub struct hala_temporal_params { pub max_history: f32, pub tol: f32, pub min_weight: f32, pub reserved: [u32; 5] }
  /// hala_temporal_clamp_params (include/halart.h, docs/RENDER_SPEC.md 16 "History clamp"; 16 B): fill it with hala_temporal_clamp_default_params
  #[repr(C)] #[derive(Default, Clone, Copy)]
  pub struct hala_temporal_clamp_params { pub radius: u32, pub gamma: f32, pub reserved: [u32; 2] }
  /// hala_shutter_params / hala_shutter_status (include/halart.h "Shutter", docs/RENDER_SPEC.md 18; 32 B each)
  #[repr(C)] #[derive(Default, Clone, Copy)]
  pub struct hala_shutter_params { pub shutter_open: f32, pub shutter_close: f32, pub time_stride: u32, pub reserved: [u32; 5] }
  #[repr(C)] #[derive(Default, Clone, Copy)]
  pub struct hala_shutter_status { pub enabled: u32, pub time_stride: u32, pub step: u32, pub time: f32, pub steps: u64, pub reserved: [u32; 2] }
  /// hala_node_refit_status, 40 B (include/halart.h "Node batches", docs/RENDER_SPEC.md 20)
  #[repr(C)] #[derive(Default, Clone, Copy)]
  pub struct hala_node_refit_status { pub bound_nodes: u32, pub affected_nodes: u32, pub affected_instances: u32, pub levels: u32, pub last_path: u32, pub last_reason: u32, pub device_refits: u64, pub host_refits: u64 }
  /// hala_refit_policy (16 B) / hala_tree_quality (48 B): include/halart.h "Tree quality and the refit policy", docs/RENDER_SPEC.md 4.6
  #[repr(C)] #[derive(Default, Clone, Copy)]
  pub struct hala_refit_policy { pub mode: u32, pub max_inflation: f32, pub reserved: [u32; 2] }
  #[repr(C)] #[derive(Default, Clone, Copy)]
  pub struct hala_tree_quality { pub first_node: u32, pub node_count: u32, pub valid: u32, pub rebuilt_last_refit: u32, pub node_q_built: u64, pub tri_q_built: u64, pub node_q_now: u64, pub tri_q_now: u64 }
  /// hala_deformer_normals_info, 24 B (RENDER_SPEC 17 "Recomputed normals")
  #[repr(C)] #[derive(Default, Clone, Copy)]
  pub struct hala_deformer_normals_info { pub mode: u32, pub class_count: u32, pub entry_count: u32, pub reserved: u32, pub launches: u64 }
  pub const HALA_DEFORM_NORMALS_AS_POSED: u32 = 0;
  pub const HALA_DEFORM_NORMALS_RECOMPUTED: u32 = 1;
  /// the largest capacity of a multi-hit batch (RENDER_SPEC 4.7)
  pub const HALA_MAX_MULTI_HITS: u32 = 16;
  /// the largest number of rays per sample of an occlusion batch (RENDER_SPEC 4.10)
  pub const HALA_MAX_OCCLUSION_RAYS: u32 = 256;
  /// the largest side of a bake map, the largest dilation margin and the flag bits of hala_bake_desc (RENDER_SPEC 4.11)
  pub const HALA_MAX_BAKE_DIM: u32 = 4096;
  pub const HALA_MAX_BAKE_MARGIN: u32 = 16;
  pub const HALA_BAKE_SHADING_NORMAL: u32 = 1;
  pub const HALA_BAKE_FLIP_NORMAL: u32 = 2;
  #[repr(C)] pub struct hala_scene { _private: [u8; 0] }
  #[repr(C)] pub struct hala_rtprog { _private: [u8; 0] }
  extern "C" {
    pub fn hala_last_error_message() -> *const c_char;
    pub fn hala_rt_create(name: *const c_char, width: u32, height: u32, device_ordinal: c_int, max_depth: u32, rr_depth: u32,
                          enable_tonemap: c_int, enable_aces: c_int, use_simple_aces: c_int, max_frames: u64, out: *mut *mut hala_rt_renderer) -> c_int;
    pub fn hala_rt_destroy(r: *mut hala_rt_renderer);
    pub fn hala_rt_push_general_shader(r: *mut hala_rt_renderer, code: *const c_void, code_size: usize, stage: c_int, debug_name: *const c_char) -> c_int;
    pub fn hala_rt_push_general_shader_with_file(r: *mut hala_rt_renderer, file_path: *const c_char, stage: c_int, debug_name: *const c_char) -> c_int;
    pub fn hala_rt_push_hit_shaders_with_file(r: *mut hala_rt_renderer, closest: *const c_char, any: *const c_char, isect: *const c_char, debug_name: *const c_char) -> c_int;
    pub fn hala_rt_load_blue_noise_pixels(r: *mut hala_rt_renderer, rgba8: *const u8, width: u32, height: u32) -> c_int;
    pub fn hala_rt_set_scene(r: *mut hala_rt_renderer, scene: *const hala_scene_desc) -> c_int;
    pub fn hala_rt_set_envmap_file(r: *mut hala_rt_renderer, path: *const c_char, rotation_degrees: f32) -> c_int;
    pub fn hala_rt_set_envmap_pixels(r: *mut hala_rt_renderer, pixels: *const f32, channels: u32, width: u32, height: u32, rotation_degrees: f32) -> c_int;
    pub fn hala_rt_set_ground_color(r: *mut hala_rt_renderer, rgba: *const f32);
    pub fn hala_rt_set_sky_color(r: *mut hala_rt_renderer, rgba: *const f32);
    pub fn hala_rt_set_env_intensity(r: *mut hala_rt_renderer, intensity: f32);
    pub fn hala_rt_set_exposure_value(r: *mut hala_rt_renderer, exposure_value: f32);
    pub fn hala_rt_commit(r: *mut hala_rt_renderer) -> c_int;
    pub fn hala_rt_update(r: *mut hala_rt_renderer, delta_time: f64, width: u32, height: u32) -> c_int;
    pub fn hala_rt_update_batch(r: *mut hala_rt_renderer, frames: u32) -> c_int;
    pub fn hala_rt_render(r: *mut hala_rt_renderer) -> c_int;
    pub fn hala_rt_wait_idle(r: *mut hala_rt_renderer) -> c_int;
    pub fn hala_rt_save_images(r: *mut hala_rt_renderer, path: *const c_char) -> c_int;
    pub fn hala_rt_get_info(r: *mut hala_rt_renderer, out: *mut hala_rt_info) -> c_int;
    pub fn hala_rt_trace_rays(r: *mut hala_rt_renderer, d_rays: *const hala_ray, d_hits: *mut hala_hit, count: u32, mode: c_int,
                              d_counters: *mut u64, hip_stream: *mut c_void) -> c_int;
    pub fn hala_rt_trace_rays_indirect(r: *mut hala_rt_renderer, d_rays: *const hala_ray, d_hits: *mut hala_hit, d_indirect: *const u32,
                                       mode: c_int, hip_stream: *mut c_void) -> c_int;
    pub fn hala_rt_trace_rays_multi(r: *mut hala_rt_renderer, d_rays: *const hala_ray, d_hits: *mut hala_hit, d_counts: *mut u32, count: u32, k: u32,
                                    hip_stream: *mut c_void) -> c_int;
    pub fn hala_rt_trace_rays_multi_host(r: *mut hala_rt_renderer, rays: *const hala_ray, hits: *mut hala_hit, counts: *mut u32, count: u32, k: u32) -> c_int;
    pub fn hala_rt_closest_points(r: *mut hala_rt_renderer, d_queries: *const hala_point_query, d_out: *mut hala_closest_point, count: u32,
                                  hip_stream: *mut c_void) -> c_int;
    pub fn hala_rt_closest_points_host(r: *mut hala_rt_renderer, queries: *const hala_point_query, out: *mut hala_closest_point, count: u32) -> c_int;
    pub fn hala_rt_closest_points_counted(r: *mut hala_rt_renderer, d_queries: *const hala_point_query, d_out: *mut hala_closest_point, count: u32,
                                          d_counters: *mut u64, hip_stream: *mut c_void) -> c_int;
    pub fn hala_rt_distance_grid(r: *mut hala_rt_renderer, desc: *const hala_distance_grid_desc, d_distance: *mut f32, d_prim: *mut u32,
                                 hip_stream: *mut c_void) -> c_int;
    pub fn hala_rt_distance_grid_host(r: *mut hala_rt_renderer, desc: *const hala_distance_grid_desc, distance: *mut f32, prim: *mut u32) -> c_int;
    pub fn hala_rt_distance_grid_counted(r: *mut hala_rt_renderer, desc: *const hala_distance_grid_desc, d_distance: *mut f32, d_prim: *mut u32,
                                         d_counters: *mut u64, hip_stream: *mut c_void) -> c_int;
    pub fn hala_rt_occlusion(r: *mut hala_rt_renderer, d_samples: *const hala_occlusion_sample, d_out: *mut hala_occlusion, d_masks: *mut u32, count: u32,
                             rays: u32, seed: u32, hip_stream: *mut c_void) -> c_int;
    pub fn hala_rt_occlusion_host(r: *mut hala_rt_renderer, samples: *const hala_occlusion_sample, out: *mut hala_occlusion, masks: *mut u32, count: u32,
                                  rays: u32, seed: u32) -> c_int;
    pub fn hala_rt_bake_samples(r: *mut hala_rt_renderer, desc: *const hala_bake_desc, d_samples: *mut hala_occlusion_sample, d_texels: *mut hala_bake_texel,
                                hip_stream: *mut c_void) -> c_int;
    pub fn hala_rt_bake_samples_host(r: *mut hala_rt_renderer, desc: *const hala_bake_desc, samples: *mut hala_occlusion_sample,
                                     texels: *mut hala_bake_texel) -> c_int;
    pub fn hala_rt_bake_occlusion(r: *mut hala_rt_renderer, desc: *const hala_bake_desc, rays: u32, seed: u32, d_out: *mut hala_occlusion,
                                  d_texels: *mut hala_bake_texel, hip_stream: *mut c_void) -> c_int;
    pub fn hala_rt_bake_occlusion_host(r: *mut hala_rt_renderer, desc: *const hala_bake_desc, rays: u32, seed: u32, out: *mut hala_occlusion,
                                       texels: *mut hala_bake_texel) -> c_int;
    pub fn hala_rt_bake_atlas_samples(r: *mut hala_rt_renderer, desc: *const hala_bake_atlas_desc, charts: *const hala_bake_chart,
                                      d_samples: *mut hala_occlusion_sample, d_texels: *mut hala_bake_texel, hip_stream: *mut c_void) -> c_int;
    pub fn hala_rt_bake_atlas_samples_host(r: *mut hala_rt_renderer, desc: *const hala_bake_atlas_desc, charts: *const hala_bake_chart,
                                           samples: *mut hala_occlusion_sample, texels: *mut hala_bake_texel) -> c_int;
    pub fn hala_rt_bake_atlas_occlusion(r: *mut hala_rt_renderer, desc: *const hala_bake_atlas_desc, charts: *const hala_bake_chart, rays: u32, seed: u32,
                                        d_out: *mut hala_occlusion, d_texels: *mut hala_bake_texel, hip_stream: *mut c_void) -> c_int;
    pub fn hala_rt_bake_atlas_occlusion_host(r: *mut hala_rt_renderer, desc: *const hala_bake_atlas_desc, charts: *const hala_bake_chart, rays: u32, seed: u32,
                                             out: *mut hala_occlusion, texels: *mut hala_bake_texel) -> c_int;
    pub fn hala_rt_bake_transfer(r: *mut hala_rt_renderer, desc: *const hala_bake_desc, transfer: *const hala_bake_transfer_desc, targets: *const u32,
                                 d_out: *mut hala_bake_transfer_hit, d_texels: *mut hala_bake_texel, hip_stream: *mut c_void) -> c_int;
    pub fn hala_rt_bake_transfer_host(r: *mut hala_rt_renderer, desc: *const hala_bake_desc, transfer: *const hala_bake_transfer_desc, targets: *const u32,
                                      out: *mut hala_bake_transfer_hit, texels: *mut hala_bake_texel) -> c_int;
    pub fn hala_rt_update_node_transform(r: *mut hala_rt_renderer, node_index: u32, local_transform: *const f32) -> c_int;
    pub fn hala_rt_update_material(r: *mut hala_rt_renderer, material_index: u32, material: *const hala_material_desc) -> c_int;
    pub fn hala_rt_update_vertices(r: *mut hala_rt_renderer, mesh_index: u32, primitive_index: u32, vertices: *const hala_vertex, vertex_count: u32) -> c_int;
    pub fn hala_rt_refit(r: *mut hala_rt_renderer) -> c_int;
    // node batches (RENDER_SPEC 20): a bound node set posed from one array of column-major locals; where 0 = host memory, 1 = device memory
    pub fn hala_rt_bind_nodes(r: *mut hala_rt_renderer, node_indices: *const u32, count: u32) -> c_int;
    pub fn hala_rt_refit_nodes(r: *mut hala_rt_renderer, locals: *const f32, where_: c_int) -> c_int;
    pub fn hala_rt_get_node_refit_status(r: *mut hala_rt_renderer, out: *mut hala_node_refit_status) -> c_int;
    // tree quality (RENDER_SPEC 4.6): mode 0 off | 1 rebuild above max_inflation | 2 rebuild at every refit | 3 measure only
    pub fn hala_rt_set_refit_policy(r: *mut hala_rt_renderer, policy: *const hala_refit_policy) -> c_int;
    pub fn hala_rt_get_tree_quality(r: *mut hala_rt_renderer, dst: *mut hala_tree_quality, capacity: u32, tree_count: *mut u32,
                                    refits_measured: *mut u64, trees_rebuilt_by_policy: *mut u64) -> c_int;
    pub fn hala_rt_load_blue_noise_texture(r: *mut hala_rt_renderer, path: *const c_char) -> c_int;
    pub fn hala_rt_set_tile_shard(r: *mut hala_rt_renderer, rank: u32, world: u32, tile_size: u32) -> c_int;
    // the exchange step (RCCL all-gather + de-interleave) inside the library
    pub fn hala_rt_comm_unique_id(out_128_bytes: *mut u8) -> c_int;
    pub fn hala_rt_comm_init_rank(r: *mut hala_rt_renderer, unique_id_128_bytes: *const u8, rank: u32, world: u32) -> c_int;
    pub fn hala_rt_comm_attach(r: *mut hala_rt_renderer, nccl_comm: *mut c_void) -> c_int;
    pub fn hala_rt_comm_destroy(r: *mut hala_rt_renderer) -> c_int;
    pub fn hala_rt_tile_allgather(r: *mut hala_rt_renderer, aov_mask: u32) -> c_int;
    pub fn hala_rt_tile_allgather_begin(r: *mut hala_rt_renderer, aov_mask: u32) -> c_int;
    pub fn hala_rt_tile_allgather_finish(r: *mut hala_rt_renderer) -> c_int;
    // HalaRayTracingProgram as a C object
    pub fn hala_rtprog_create(r: *mut hala_rt_renderer, desc_json: *const c_char, debug_name: *const c_char, out: *mut *mut hala_rtprog) -> c_int;
    pub fn hala_rtprog_destroy(p: *mut hala_rtprog);
    pub fn hala_rtprog_bind(p: *mut hala_rtprog, d_rays: *const hala_ray, d_hits: *mut hala_hit) -> c_int;
    pub fn hala_rtprog_push_constants(p: *mut hala_rtprog, offset: u32, data: *const c_void, len: usize) -> c_int;
    pub fn hala_rtprog_push_constants_f32(p: *mut hala_rtprog, offset: u32, data: *const f32, count: usize) -> c_int;
    pub fn hala_rtprog_trace_rays(p: *mut hala_rtprog, width: u32, height: u32, depth: u32, hip_stream: *mut c_void) -> c_int;
    pub fn hala_rtprog_trace_rays_indirect(p: *mut hala_rtprog, d_indirect: *const u32, hip_stream: *mut c_void) -> c_int;
    pub fn hala_rtprog_trace_rays_multi(p: *mut hala_rtprog, width: u32, height: u32, depth: u32, k: u32, d_counts: *mut u32, hip_stream: *mut c_void) -> c_int;
    pub fn hala_rt_tile_buffer(r: *mut hala_rt_renderer, which: c_int, d_ptr: *mut *mut c_void, bytes: *mut usize) -> c_int;
    pub fn hala_rt_scatter_gathered_tiles(r: *mut hala_rt_renderer, which: c_int, d_gathered: *const c_void, bytes: usize) -> c_int;
    pub fn hala_rt_scatter_gathered_tiles_on_stream(r: *mut hala_rt_renderer, which: c_int, d_gathered: *const c_void, bytes: usize, hip_stream: *mut c_void) -> c_int;
    pub fn hala_rt_get_stream(r: *mut hala_rt_renderer, hip_stream: *mut *mut c_void) -> c_int;
    pub fn hala_rt_set_launch_timing_period(r: *mut hala_rt_renderer, period: u32) -> c_int;
    pub fn hala_rt_set_pass_fusion(r: *mut hala_rt_renderer, mode: u32) -> c_int;
    pub fn hala_rt_variant_ledger(family: u32, launched: *mut u64, built: *mut u64, reset: c_int) -> c_int;
    pub fn hala_rt_selftest_math(which: c_int, first: u32, count: u64, mismatches: *mut u64, first_bad: *mut u32) -> c_int;
    pub fn hala_rt_selftest_math_values(which: c_int, patterns: *const u32, count: u32, helper_bits: *mut u32, reference_bits: *mut u32,
                                        mismatches: *mut u64, first_bad: *mut u32) -> c_int;
    pub fn hala_rt_selftest_collapse(leaves: u32, leaf_max: u32, left: *const u32, right: *const u32, node_parent: *const u32,
                                     leaf_parent: *const u32, first: *const u32, last: *const u32, node_boxes: *const f32,
                                     leaf_boxes: *const f32, costs: *mut f32, choices: *mut u32, keep: *mut u32, refs4: *mut u32,
                                     node_count: *mut u32, levels: *mut u32) -> c_int;
    // one hierarchy builder (1 SAH, 2 PLOC, 3 LBVH) on `count` boxes [count][6] from host memory; out: the binary tree in the arrays
    // hala_rt_selftest_collapse takes, sorted_ids [count] and node_boxes [count - 1][6] widened by pad (include/halart.h)
    pub fn hala_rt_selftest_hierarchy(count: u32, boxes: *const f32, pad: f32, builder: u32, ploc_tail: u32, ploc_look_every: u32,
                                      sorted_ids: *mut u32, left: *mut u32, right: *mut u32, first: *mut u32, last: *mut u32,
                                      node_parent: *mut u32, leaf_parent: *mut u32, node_boxes: *mut f32) -> c_int;
    pub fn hala_rt_set_frames_in_flight(r: *mut hala_rt_renderer, n: u32) -> c_int;
    pub fn hala_rt_frames_in_flight_info(r: *mut hala_rt_renderer, second_slot_updates: *mut u64, second_buffers: *mut u32) -> c_int;
    pub fn hala_rt_set_build_options(r: *mut hala_rt_renderer, options: *const hala_rt_build_options) -> c_int;
    pub fn hala_rt_tile_allgather_begin_external(r: *mut hala_rt_renderer, aov_mask: u32) -> c_int;
    pub fn hala_rt_get_exchange_buffers(r: *mut hala_rt_renderer, which: c_int, d_staged: *mut *mut c_void, staged_bytes: *mut usize,
                                        d_receive: *mut *mut c_void, receive_bytes: *mut usize, hip_stream: *mut *mut c_void) -> c_int;
    // first-hit AOVs (docs/RENDER_SPEC.md 13): mask bit 0 = image 4 position, bit 1 = image 5 ids
    pub fn hala_rt_set_aovs(r: *mut hala_rt_renderer, mask: u32) -> c_int;
    pub fn hala_temporal_default_params(out: *mut hala_temporal_params);
    pub fn hala_rt_set_temporal(r: *mut hala_rt_renderer, p: *const hala_temporal_params) -> c_int;
    pub fn hala_rt_set_temporal_vertex_motion(r: *mut hala_rt_renderer, enable: c_int) -> c_int;
    pub fn hala_temporal_clamp_default_params(out: *mut hala_temporal_clamp_params);
    pub fn hala_rt_set_temporal_clamp(r: *mut hala_rt_renderer, p: *const hala_temporal_clamp_params) -> c_int;
    // shutter motion blur (RENDER_SPEC 18): every setter is an edit, applied by hala_rt_refit; a NULL pair of keys clears them
    pub fn hala_shutter_default_params(out: *mut hala_shutter_params);
    pub fn hala_rt_set_shutter(r: *mut hala_rt_renderer, p: *const hala_shutter_params) -> c_int;
    pub fn hala_rt_get_shutter_status(r: *mut hala_rt_renderer, out: *mut hala_shutter_status) -> c_int;
    pub fn hala_rt_set_node_keys(r: *mut hala_rt_renderer, node_index: u32, open: *const f32, close: *const f32) -> c_int;
    pub fn hala_rt_set_deformer_keys(r: *mut hala_rt_renderer, mesh_index: u32, primitive_index: u32, weights_open: *const f32, weights_close: *const f32,
                                     weight_count: u32, palette_open: *const f32, palette_close: *const f32, joint_count: u32) -> c_int;
    // recomputed normals of a deformer (RENDER_SPEC 17): an edit like the others, applied by hala_rt_refit
    pub fn hala_rt_set_deformer_normals(r: *mut hala_rt_renderer, mesh_index: u32, primitive_index: u32, mode: u32) -> c_int;
    pub fn hala_rt_get_deformer_normals(r: *mut hala_rt_renderer, mesh_index: u32, primitive_index: u32, out: *mut hala_deformer_normals_info) -> c_int;
    pub fn hala_rt_set_vertex_keys(r: *mut hala_rt_renderer, mesh_index: u32, primitive_index: u32, open: *const c_void, close: *const c_void,
                                   vertex_count: u32) -> c_int;
    pub fn hala_rt_temporal_capture(r: *mut hala_rt_renderer) -> c_int;
    pub fn hala_rt_temporal_resolve(r: *mut hala_rt_renderer, gpu_ms: *mut f32) -> c_int;
    pub fn hala_rt_read_temporal(r: *mut hala_rt_renderer, which: c_int, dst_rgba32f: *mut f32) -> c_int;
    // light groups (docs/RENDER_SPEC.md 14): g = NULL turns them off; relight which 0 = linear, 1 = tonemapped
    pub fn hala_rt_set_light_groups(r: *mut hala_rt_renderer, g: *const hala_light_groups) -> c_int;
    pub fn hala_rt_read_light_group(r: *mut hala_rt_renderer, view: u32, group: u32, dst_rgba32f: *mut f32) -> c_int;
    pub fn hala_rt_relight(r: *mut hala_rt_renderer, view: u32, rgb_scales: *const f32, group_count: u32) -> c_int;
    pub fn hala_rt_read_relit(r: *mut hala_rt_renderer, which: c_int, dst_rgba32f: *mut f32) -> c_int;
    pub fn hala_rt_get_relit_buffer(r: *mut hala_rt_renderer, which: c_int, d_ptr: *mut *mut c_void, bytes: *mut usize) -> c_int;
    // Cryptomatte (docs/RENDER_SPEC.md 15): d = NULL turns it off; layer 0 object, 1 material, 2 asset
    pub fn hala_rt_set_cryptomatte(r: *mut hala_rt_renderer, d: *const hala_cryptomatte_desc) -> c_int;
    pub fn hala_rt_read_cryptomatte(r: *mut hala_rt_renderer, view: u32, layer: u32, dst: *mut f32) -> c_int;
    pub fn hala_rt_read_cryptomatte_records(r: *mut hala_rt_renderer, view: u32, layer: u32, dst: *mut u32) -> c_int;
    pub fn hala_rt_get_cryptomatte_manifest(r: *mut hala_rt_renderer, layer: u32, dst: *mut c_char, capacity: usize, length: *mut usize) -> c_int;
    pub fn hala_rt_save_cryptomatte(r: *mut hala_rt_renderer, view: u32, path: *const c_char) -> c_int;
    pub fn hala_cryptomatte_hash(name: *const c_char, raw: *mut u32, id: *mut u32) -> c_int;
    pub fn hala_write_exr(path: *const c_char, width: u32, height: u32, channel_count: u32, channel_names: *const *const c_char,
                          planes: *const *const f32, attribute_count: u32, attr_names: *const *const c_char, attr_values: *const *const c_char) -> c_int;
    // cpu::HalaScene::new inside the library (for hosts without the Rust `src/scene` module)
    pub fn hala_scene_load_gltf(path: *const c_char, out: *mut *mut hala_scene) -> c_int;
    pub fn hala_scene_get_desc(scene: *const hala_scene) -> *const hala_scene_desc;
    pub fn hala_scene_free(scene: *mut hala_scene);
    pub fn hala_load_float_image(path: *const c_char, width: *mut u32, height: *mut u32, channels: *mut u32, dst: *mut f32, capacity_floats: usize) -> c_int;
  }
}

/// src/error.rs:5-22
#[derive(thiserror::Error, Debug)]
#[error("{msg}")]
pub struct HalaRendererError { msg: String }
impl HalaRendererError {
  pub fn new(msg: &str) -> Self { Self { msg: msg.to_string() } }
  pub fn message(&self) -> &str { &self.msg }
}
fn check(rc: c_int) -> Result<(), HalaRendererError> {
  if rc == 0 { return Ok(()); }
  let msg = unsafe { CStr::from_ptr(sys::hala_last_error_message()) }.to_string_lossy().into_owned();
  Err(HalaRendererError { msg })
}
fn cpath<P: AsRef<Path>>(p: P) -> CString { CString::new(p.as_ref().to_string_lossy().as_bytes()).unwrap() }

/// CPU scene model the application already owns (`hala_renderer::scene::cpu`); only the parts read here are listed.
pub mod cpu {
  pub struct HalaNode { pub name: String, pub parent: Option<u32>, pub local_transform: glam::Mat4, pub mesh_index: u32, pub camera_index: u32, pub light_index: u32 }
  pub struct HalaPrimitive { pub indices: Vec<u32>, pub vertices: Vec<super::sys::hala_vertex>, pub material_index: u32 }
  pub struct HalaMesh { pub primitives: Vec<HalaPrimitive> }
  pub struct HalaScene {
    pub nodes: Vec<HalaNode>, pub meshes: Vec<HalaMesh>, pub materials: Vec<super::sys::hala_material_desc>,
    pub lights: Vec<super::sys::hala_light_desc>, pub cameras: Vec<super::sys::hala_camera_desc>,
    pub texture2image_mapping: std::collections::BTreeMap<u32, u32>, pub image2data_mapping: std::collections::BTreeMap<u32, u32>,
    pub image_data: Vec<(u32, u32, u32, Vec<u8>)>,  // (format, width, height, bytes)
  }
}

/// src/renderer.rs:11-15
pub struct HalaRendererInfo { pub name: String, pub width: u32, pub height: u32 }

/// src/rt_renderer.rs:568-617 — same constructor arguments minus the window (headless).
pub struct HalaRenderer { h: *mut sys::hala_rt_renderer, info: HalaRendererInfo }

impl HalaRenderer {
  /// src/rt_renderer.rs:650-813
  #[allow(clippy::too_many_arguments)]
  pub fn new(name: &str, width: u32, height: u32, device_ordinal: i32, max_depth: u32, rr_depth: u32, enable_tonemap: bool,
             enable_aces: bool, use_simple_aces: bool, max_frames: u64) -> Result<Self, HalaRendererError> {
    let mut h = std::ptr::null_mut();
    let cname = CString::new(name).unwrap();
    check(unsafe { sys::hala_rt_create(cname.as_ptr(), width, height, device_ordinal, max_depth, rr_depth, enable_tonemap as c_int,
                                       enable_aces as c_int, use_simple_aces as c_int, max_frames, &mut h) })?;
    Ok(Self { h, info: HalaRendererInfo { name: name.to_string(), width, height } })
  }
  pub fn info(&self) -> &HalaRendererInfo { &self.info }

  /// src/rt_renderer.rs:965-995 (accepted, recorded, ignored: the integrator is compiled into the library)
  pub fn push_general_shader_with_file(&mut self, file_path: &str, stage: i32, debug_name: &str) -> Result<(), HalaRendererError> {
    let (p, n) = (CString::new(file_path).unwrap(), CString::new(debug_name).unwrap());
    check(unsafe { sys::hala_rt_push_general_shader_with_file(self.h, p.as_ptr(), stage, n.as_ptr()) })
  }
  /// src/rt_renderer.rs:1161-1178 — the scene is borrowed for the call only
  pub fn set_scene(&mut self, scene: &mut cpu::HalaScene) -> Result<(), HalaRendererError> {
    let names: Vec<CString> = scene.nodes.iter().map(|n| CString::new(n.name.as_str()).unwrap()).collect();
    let nodes: Vec<sys::hala_node_desc> = scene.nodes.iter().zip(&names).map(|(n, name)| sys::hala_node_desc {
      name: name.as_ptr(), parent: n.parent.map_or(-1, |p| p as i32), local_transform: n.local_transform.to_cols_array(),
      mesh_index: n.mesh_index, camera_index: n.camera_index, light_index: n.light_index }).collect();
    let prims: Vec<Vec<sys::hala_primitive_desc>> = scene.meshes.iter().map(|m| m.primitives.iter().map(|p| sys::hala_primitive_desc {
      indices: p.indices.as_ptr(), index_count: p.indices.len() as u32, vertices: p.vertices.as_ptr(), vertex_count: p.vertices.len() as u32,
      material_index: p.material_index }).collect()).collect();
    let meshes: Vec<sys::hala_mesh_desc> = prims.iter().map(|p| sys::hala_mesh_desc { primitives: p.as_ptr(), primitive_count: p.len() as u32 }).collect();
    let t2i: Vec<sys::hala_index_pair> = scene.texture2image_mapping.iter().map(|(k, v)| sys::hala_index_pair { key: *k, value: *v }).collect();
    let i2d: Vec<sys::hala_index_pair> = scene.image2data_mapping.iter().map(|(k, v)| sys::hala_index_pair { key: *k, value: *v }).collect();
    let images: Vec<sys::hala_image_desc> = scene.image_data.iter().map(|(f, w, h, d)| sys::hala_image_desc {
      format: *f, width: *w, height: *h, data: d.as_ptr() as *const c_void, num_of_bytes: d.len() }).collect();
    let desc = sys::hala_scene_desc {
      nodes: nodes.as_ptr(), node_count: nodes.len() as u32, meshes: meshes.as_ptr(), mesh_count: meshes.len() as u32,
      materials: scene.materials.as_ptr(), material_count: scene.materials.len() as u32, lights: scene.lights.as_ptr(), light_count: scene.lights.len() as u32,
      cameras: scene.cameras.as_ptr(), camera_count: scene.cameras.len() as u32, texture2image_mapping: t2i.as_ptr(), texture_count: t2i.len() as u32,
      image2data_mapping: i2d.as_ptr(), image_count: i2d.len() as u32, image_data: images.as_ptr(), image_data_count: images.len() as u32 };
    check(unsafe { sys::hala_rt_set_scene(self.h, &desc) })
  }
  /// src/rt_renderer.rs:1117-1156
  pub fn load_blue_noise_texture<P: AsRef<Path>>(&mut self, path: P) -> Result<(), HalaRendererError> {
    check(unsafe { sys::hala_rt_load_blue_noise_texture(self.h, cpath(path).as_ptr()) })
  }
  /// src/rt_renderer.rs:1184-1195
  pub fn set_envmap<P: AsRef<Path>>(&mut self, path: P, rotation: f32) -> Result<(), HalaRendererError> {
    check(unsafe { sys::hala_rt_set_envmap_file(self.h, cpath(path).as_ptr(), rotation) })
  }
  /// src/rt_renderer.rs:1199-1219
  pub fn set_ground_color(&mut self, color: glam::Vec4) { unsafe { sys::hala_rt_set_ground_color(self.h, color.to_array().as_ptr()) } }
  pub fn set_sky_color(&mut self, color: glam::Vec4) { unsafe { sys::hala_rt_set_sky_color(self.h, color.to_array().as_ptr()) } }
  pub fn set_env_intensity(&mut self, intensity: f32) { unsafe { sys::hala_rt_set_env_intensity(self.h, intensity) } }
  pub fn set_exposure_value(&mut self, exposure_value: f32) { unsafe { sys::hala_rt_set_exposure_value(self.h, exposure_value) } }
  /// src/rt_renderer.rs:1224-1352
  pub fn save_images<P: AsRef<Path>>(&self, path: P) -> Result<(), HalaRendererError> { check(unsafe { sys::hala_rt_save_images(self.h, cpath(path).as_ptr()) }) }

  // HalaRendererTrait (src/renderer.rs:210-324)
  pub fn commit(&mut self) -> Result<(), HalaRendererError> { check(unsafe { sys::hala_rt_commit(self.h) }) }
  pub fn update(&mut self, delta_time: f64, width: u32, height: u32) -> Result<(), HalaRendererError> { check(unsafe { sys::hala_rt_update(self.h, delta_time, width, height) }) }
  pub fn update_batch(&mut self, frames: u32) -> Result<(), HalaRendererError> { check(unsafe { sys::hala_rt_update_batch(self.h, frames) }) }
  pub fn render(&mut self) -> Result<(), HalaRendererError> { check(unsafe { sys::hala_rt_render(self.h) }) }
  pub fn wait_idle(&self) -> Result<(), HalaRendererError> { check(unsafe { sys::hala_rt_wait_idle(self.h) }) }

  // beyond the reference: refit + tile sharding (BASELINE.json north_star)
  pub fn update_node_transform(&mut self, node_index: u32, local: glam::Mat4) -> Result<(), HalaRendererError> {
    check(unsafe { sys::hala_rt_update_node_transform(self.h, node_index, local.to_cols_array().as_ptr()) })
  }
  pub fn update_vertices(&mut self, mesh_index: u32, primitive_index: u32, vertices: &[sys::hala_vertex]) -> Result<(), HalaRendererError> {
    check(unsafe { sys::hala_rt_update_vertices(self.h, mesh_index, primitive_index, vertices.as_ptr(), vertices.len() as u32) })
  }
  pub fn refit(&mut self) -> Result<(), HalaRendererError> { check(unsafe { sys::hala_rt_refit(self.h) }) }
  /// closest-point queries (RENDER_SPEC 4.8) from host memory: the nearest surface point within each query's radius; a miss has distance < 0
  pub fn closest_points(&self, queries: &[sys::hala_point_query]) -> Result<Vec<sys::hala_closest_point>, HalaRendererError> {
    let miss = sys::hala_closest_point { distance: -1.0, u: 0.0, v: 0.0, prim: u32::MAX, point: [0.0; 3], region: 0 };
    let mut out = vec![miss; queries.len()];
    check(unsafe { sys::hala_rt_closest_points_host(self.h, queries.as_ptr(), out.as_mut_ptr(), queries.len() as u32) })?;
    Ok(out)
  }
  /// the device-pointer form, on the renderer's stream
  /// RENDER_SPEC 4.9: the distance field on a grid, [nz][ny][nx] with x fastest (host memory, synchronous)
  pub fn distance_grid(&self, desc: &sys::hala_distance_grid_desc) -> Result<Vec<f32>, HalaRendererError> {
    let mut out = vec![0.0f32; desc.dims[0] as usize * desc.dims[1] as usize * desc.dims[2] as usize];
    check(unsafe { sys::hala_rt_distance_grid_host(self.h, desc, out.as_mut_ptr(), std::ptr::null_mut()) })?;
    Ok(out)
  }
  pub fn closest_points_device(&self, d_queries: *const sys::hala_point_query, d_out: *mut sys::hala_closest_point, count: u32) -> Result<(), HalaRendererError> {
    check(unsafe { sys::hala_rt_closest_points(self.h, d_queries, d_out, count, std::ptr::null_mut()) })
  }
  /// occlusion batches (RENDER_SPEC 4.10) from host memory: `rays` (1..=256) any-hit rays over each sample's hemisphere; visibility < 0 marks
  /// an invalid sample
  pub fn occlusion(&self, samples: &[sys::hala_occlusion_sample], rays: u32, seed: u32) -> Result<Vec<sys::hala_occlusion>, HalaRendererError> {
    let mut out = vec![sys::hala_occlusion { visibility: -1.0, bent: [0.0; 3] }; samples.len()];
    check(unsafe { sys::hala_rt_occlusion_host(self.h, samples.as_ptr(), out.as_mut_ptr(), std::ptr::null_mut(), samples.len() as u32, rays, seed) })?;
    Ok(out)
  }
  /// the device-pointer form, on the renderer's stream; d_masks (count * ceil(rays / 32) words) may be null
  pub fn occlusion_device(&self, d_samples: *const sys::hala_occlusion_sample, d_out: *mut sys::hala_occlusion, d_masks: *mut u32, count: u32, rays: u32,
                          seed: u32) -> Result<(), HalaRendererError> {
    check(unsafe { sys::hala_rt_occlusion(self.h, d_samples, d_out, d_masks, count, rays, seed, std::ptr::null_mut()) })
  }
  /// bake maps (RENDER_SPEC 4.11) to host memory: the occlusion samples and texel records of the desc.width x desc.height map of an
  /// instance's texture space, row-major from the row of the smallest v; a texel nothing covers has prim 0xffffffff and the all-zero sample
  pub fn bake_samples(&self, desc: &sys::hala_bake_desc) -> Result<(Vec<sys::hala_occlusion_sample>, Vec<sys::hala_bake_texel>), HalaRendererError> {
    let n = desc.width as usize * desc.height as usize;
    let mut samples = vec![sys::hala_occlusion_sample { point: [0.0; 3], bias: 0.0, normal: [0.0; 3], reach: 0.0 }; n];
    let mut texels = vec![sys::hala_bake_texel { u: 0.0, v: 0.0, prim: u32::MAX, source: u32::MAX }; n];
    check(unsafe { sys::hala_rt_bake_samples_host(self.h, desc, samples.as_mut_ptr(), texels.as_mut_ptr()) })?;
    Ok((samples, texels))
  }
  /// the baked occlusion map: `rays` (1..=256) any-hit rays per covered texel, then the gutters filled within desc.margin texels; visibility < 0
  /// marks a texel that neither has a sample nor was filled, texels[i].source the texel a record came from
  pub fn bake_occlusion(&self, desc: &sys::hala_bake_desc, rays: u32, seed: u32) -> Result<(Vec<sys::hala_occlusion>, Vec<sys::hala_bake_texel>), HalaRendererError> {
    let n = desc.width as usize * desc.height as usize;
    let mut out = vec![sys::hala_occlusion { visibility: -1.0, bent: [0.0; 3] }; n];
    let mut texels = vec![sys::hala_bake_texel { u: 0.0, v: 0.0, prim: u32::MAX, source: u32::MAX }; n];
    check(unsafe { sys::hala_rt_bake_occlusion_host(self.h, desc, rays, seed, out.as_mut_ptr(), texels.as_mut_ptr()) })?;
    Ok((out, texels))
  }
  /// the device-pointer forms, on the renderer's stream; d_texels (width * height records) may be null
  pub fn bake_samples_device(&self, desc: &sys::hala_bake_desc, d_samples: *mut sys::hala_occlusion_sample, d_texels: *mut sys::hala_bake_texel) -> Result<(), HalaRendererError> {
    check(unsafe { sys::hala_rt_bake_samples(self.h, desc, d_samples, d_texels, std::ptr::null_mut()) })
  }
  pub fn bake_occlusion_device(&self, desc: &sys::hala_bake_desc, rays: u32, seed: u32, d_out: *mut sys::hala_occlusion, d_texels: *mut sys::hala_bake_texel)
                               -> Result<(), HalaRendererError> {
    check(unsafe { sys::hala_rt_bake_occlusion(self.h, desc, rays, seed, d_out, d_texels, std::ptr::null_mut()) })
  }
  /// bake atlases (RENDER_SPEC 4.12) to host memory: the instances of `charts`, each through its scale and offset, in one map; `desc.chart_count`
  /// is taken from the slice.  Only texels that a chart covers are traced by the occlusion form.
  pub fn bake_atlas_samples(&self, desc: &sys::hala_bake_atlas_desc, charts: &[sys::hala_bake_chart])
                            -> Result<(Vec<sys::hala_occlusion_sample>, Vec<sys::hala_bake_texel>), HalaRendererError> {
    let d = sys::hala_bake_atlas_desc { chart_count: charts.len() as u32, ..*desc };
    let n = d.width as usize * d.height as usize;
    let mut samples = vec![sys::hala_occlusion_sample { point: [0.0; 3], bias: 0.0, normal: [0.0; 3], reach: 0.0 }; n];
    let mut texels = vec![sys::hala_bake_texel { u: 0.0, v: 0.0, prim: u32::MAX, source: u32::MAX }; n];
    check(unsafe { sys::hala_rt_bake_atlas_samples_host(self.h, &d, charts.as_ptr(), samples.as_mut_ptr(), texels.as_mut_ptr()) })?;
    Ok((samples, texels))
  }
  pub fn bake_atlas_occlusion(&self, desc: &sys::hala_bake_atlas_desc, charts: &[sys::hala_bake_chart], rays: u32, seed: u32)
                              -> Result<(Vec<sys::hala_occlusion>, Vec<sys::hala_bake_texel>), HalaRendererError> {
    let d = sys::hala_bake_atlas_desc { chart_count: charts.len() as u32, ..*desc };
    let n = d.width as usize * d.height as usize;
    let mut out = vec![sys::hala_occlusion { visibility: -1.0, bent: [0.0; 3] }; n];
    let mut texels = vec![sys::hala_bake_texel { u: 0.0, v: 0.0, prim: u32::MAX, source: u32::MAX }; n];
    check(unsafe { sys::hala_rt_bake_atlas_occlusion_host(self.h, &d, charts.as_ptr(), rays, seed, out.as_mut_ptr(), texels.as_mut_ptr()) })?;
    Ok((out, texels))
  }
  /// the device-pointer forms, on the renderer's stream; the chart table is read before they return; d_texels may be null
  pub fn bake_atlas_samples_device(&self, desc: &sys::hala_bake_atlas_desc, charts: &[sys::hala_bake_chart], d_samples: *mut sys::hala_occlusion_sample,
                                   d_texels: *mut sys::hala_bake_texel) -> Result<(), HalaRendererError> {
    let d = sys::hala_bake_atlas_desc { chart_count: charts.len() as u32, ..*desc };
    check(unsafe { sys::hala_rt_bake_atlas_samples(self.h, &d, charts.as_ptr(), d_samples, d_texels, std::ptr::null_mut()) })
  }
  pub fn bake_atlas_occlusion_device(&self, desc: &sys::hala_bake_atlas_desc, charts: &[sys::hala_bake_chart], rays: u32, seed: u32,
                                     d_out: *mut sys::hala_occlusion, d_texels: *mut sys::hala_bake_texel) -> Result<(), HalaRendererError> {
    let d = sys::hala_bake_atlas_desc { chart_count: charts.len() as u32, ..*desc };
    check(unsafe { sys::hala_rt_bake_atlas_occlusion(self.h, &d, charts.as_ptr(), rays, seed, d_out, d_texels, std::ptr::null_mut()) })
  }
  /// transfer bakes (RENDER_SPEC 4.13) to host memory: every texel of `desc.instance`'s map projected from `front` ahead of its surface to `back`
  /// behind it onto the instances of `targets` (empty: every other instance); `transfer.target_count` is taken from the slice
  pub fn bake_transfer(&self, desc: &sys::hala_bake_desc, transfer: &sys::hala_bake_transfer_desc, targets: &[u32])
                       -> Result<(Vec<sys::hala_bake_transfer_hit>, Vec<sys::hala_bake_texel>), HalaRendererError> {
    let t = sys::hala_bake_transfer_desc { target_count: targets.len() as u32, ..*transfer };
    let n = desc.width as usize * desc.height as usize;
    let mut out = vec![sys::hala_bake_transfer_hit { t: -1.0, u: 0.0, v: 0.0, prim: u32::MAX, normal: [0.0; 3], height: 0.0 }; n];
    let mut texels = vec![sys::hala_bake_texel { u: 0.0, v: 0.0, prim: u32::MAX, source: u32::MAX }; n];
    let list = if targets.is_empty() { std::ptr::null() } else { targets.as_ptr() };
    check(unsafe { sys::hala_rt_bake_transfer_host(self.h, desc, &t, list, out.as_mut_ptr(), texels.as_mut_ptr()) })?;
    Ok((out, texels))
  }
  /// the device-pointer form, on the renderer's stream; the target list is read before it returns; d_texels may be null
  pub fn bake_transfer_device(&self, desc: &sys::hala_bake_desc, transfer: &sys::hala_bake_transfer_desc, targets: &[u32],
                              d_out: *mut sys::hala_bake_transfer_hit, d_texels: *mut sys::hala_bake_texel) -> Result<(), HalaRendererError> {
    let t = sys::hala_bake_transfer_desc { target_count: targets.len() as u32, ..*transfer };
    let list = if targets.is_empty() { std::ptr::null() } else { targets.as_ptr() };
    check(unsafe { sys::hala_rt_bake_transfer(self.h, desc, &t, list, d_out, d_texels, std::ptr::null_mut()) })
  }
  /// binds an ordered node set (empty: unbinds); refit_nodes then takes one local transform per bound node, in that order
  pub fn bind_nodes(&mut self, node_indices: &[u32]) -> Result<(), HalaRendererError> {
    check(unsafe { sys::hala_rt_bind_nodes(self.h, node_indices.as_ptr(), node_indices.len() as u32) })
  }
  /// update_node_transform for every bound node + refit, with the per-node and per-instance work on the device where it can be
  pub fn refit_nodes(&mut self, locals: &[glam::Mat4]) -> Result<(), HalaRendererError> {
    let flat: Vec<f32> = locals.iter().flat_map(|m| m.to_cols_array()).collect();
    check(unsafe { sys::hala_rt_refit_nodes(self.h, flat.as_ptr(), 0) })
  }
  /// the same from device memory of the renderer's device (16 floats per bound node, column-major), read on the renderer's stream
  pub unsafe fn refit_nodes_device(&mut self, d_locals: *const f32) -> Result<(), HalaRendererError> { check(sys::hala_rt_refit_nodes(self.h, d_locals, 1)) }
  pub fn node_refit_status(&self) -> Result<sys::hala_node_refit_status, HalaRendererError> {
    let mut s = sys::hala_node_refit_status::default();
    check(unsafe { sys::hala_rt_get_node_refit_status(self.h, &mut s) })?;
    Ok(s)
  }
  /// the refit policy (RENDER_SPEC 4.6): mode 0 off, 1 rebuild when a refitted tree's cost exceeds max_inflation times its cost when built,
  /// 2 rebuild at every refit, 3 measure only; max_inflation is 0 unless mode is 1
  pub fn set_refit_policy(&mut self, mode: u32, max_inflation: f32) -> Result<(), HalaRendererError> {
    let p = sys::hala_refit_policy { mode, max_inflation, reserved: [0; 2] };
    check(unsafe { sys::hala_rt_set_refit_policy(self.h, &p) })
  }
  /// (trees, refits_measured, trees_rebuilt_by_policy)
  pub fn tree_quality(&self) -> Result<(Vec<sys::hala_tree_quality>, u64, u64), HalaRendererError> {
    let (mut n, mut measured, mut rebuilt) = (0u32, 0u64, 0u64);
    check(unsafe { sys::hala_rt_get_tree_quality(self.h, std::ptr::null_mut(), 0, &mut n, &mut measured, &mut rebuilt) })?;
    let mut trees = vec![sys::hala_tree_quality::default(); n as usize];
    check(unsafe { sys::hala_rt_get_tree_quality(self.h, trees.as_mut_ptr(), n, &mut n, &mut measured, &mut rebuilt) })?;
    trees.truncate(n as usize);
    Ok((trees, measured, rebuilt))
  }
  /// the hipStream_t of this renderer, for stream-ordered hand-overs of the tile buffer (multi-GPU gather)
  pub fn stream(&self) -> Result<*mut c_void, HalaRendererError> {
    let mut s: *mut c_void = std::ptr::null_mut();
    check(unsafe { sys::hala_rt_get_stream(self.h, &mut s) })?;
    Ok(s)
  }
  /// per-launch timing events on every `period`-th update (1: all, 0: none)
  pub fn set_launch_timing_period(&mut self, period: u32) -> Result<(), HalaRendererError> { check(unsafe { sys::hala_rt_set_launch_timing_period(self.h, period) }) }
  /// 2 (default): updates without per-launch timing alternate between two frame slots and overlap; 1: strictly serial
  pub fn set_frames_in_flight(&mut self, n: u32) -> Result<(), HalaRendererError> { check(unsafe { sys::hala_rt_set_frames_in_flight(self.h, n) }) }
  /// 0: one launch per pass, 1 (default): fused launches except in timed updates, 2: always
  pub fn set_pass_fusion(&mut self, mode: u32) -> Result<(), HalaRendererError> { check(unsafe { sys::hala_rt_set_pass_fusion(self.h, mode) }) }
  /// How the next commit() builds the acceleration structure: builder 0 auto | 1 SAH | 2 PLOC | 3 LBVH; instancing 0 auto | 1 flattened |
  /// 2 two-level (the BLAS / TLAS split of gpu_uploader.rs:782-815, :937-959)
  pub fn set_build_options(&mut self, builder: u32, instancing: u32) -> Result<(), HalaRendererError> {
    let o = sys::hala_rt_build_options { builder, instancing, ..Default::default() };
    check(unsafe { sys::hala_rt_set_build_options(self.h, &o) })
  }
  pub fn set_tile_shard(&mut self, rank: u32, world: u32, tile_size: u32) -> Result<(), HalaRendererError> { check(unsafe { sys::hala_rt_set_tile_shard(self.h, rank, world, tile_size) }) }

  // temporal reprojection across scene edits (docs/RENDER_SPEC.md 16); needs AOV bits 0 and 1 (sys::hala_rt_set_aovs(h, 3))
  /// the library's default parameters when `enable`, else the feature off and its buffers freed
  pub fn set_temporal(&mut self, enable: bool) -> Result<(), HalaRendererError> {
    if !enable { return check(unsafe { sys::hala_rt_set_temporal(self.h, std::ptr::null()) }); }
    let mut p = sys::hala_temporal_params::default();
    unsafe { sys::hala_temporal_default_params(&mut p) };
    check(unsafe { sys::hala_rt_set_temporal(self.h, &p) })
  }
  /// RENDER_SPEC 16 "Vertex motion": the history follows vertex edits and posed deformers on a one-level tree
  pub fn set_temporal_vertex_motion(&mut self, enable: bool) -> Result<(), HalaRendererError> {
    check(unsafe { sys::hala_rt_set_temporal_vertex_motion(self.h, enable as c_int) })
  }
  /// RENDER_SPEC 16 "History clamp": the library's default radius and gamma when `enable`, else the clamp off
  pub fn set_temporal_clamp(&mut self, enable: bool) -> Result<(), HalaRendererError> {
    if !enable { return check(unsafe { sys::hala_rt_set_temporal_clamp(self.h, std::ptr::null()) }); }
    let mut p = sys::hala_temporal_clamp_params::default();
    unsafe { sys::hala_temporal_clamp_default_params(&mut p) };
    check(unsafe { sys::hala_rt_set_temporal_clamp(self.h, &p) })
  }
  /// before an edit: keep the frame as the history
  pub fn temporal_capture(&mut self) -> Result<(), HalaRendererError> { check(unsafe { sys::hala_rt_temporal_capture(self.h) }) }
  /// after the edit, refit and a few updates: blend the reprojected history with the new samples (read with sys::hala_rt_read_temporal)
  pub fn temporal_resolve(&mut self) -> Result<(), HalaRendererError> { check(unsafe { sys::hala_rt_temporal_resolve(self.h, std::ptr::null_mut()) }) }
}
impl Drop for HalaRenderer { fn drop(&mut self) { unsafe { sys::hala_rt_destroy(self.h) } } }

/// A scene loaded by the library's own glTF reader (csrc/gltf_loader.cpp): what `cpu::HalaScene::new(path)` returns in the
/// reference (src/scene/cpu/scene.rs:40-55), kept on the C side and handed to `set_scene` by reference.
pub struct HalaNativeScene { h: *mut sys::hala_scene }
impl HalaNativeScene {
  pub fn new<P: AsRef<Path>>(path: P) -> Result<Self, HalaRendererError> {
    let mut h = std::ptr::null_mut();
    check(unsafe { sys::hala_scene_load_gltf(cpath(path).as_ptr(), &mut h) })?;
    Ok(Self { h })
  }
}
impl Drop for HalaNativeScene { fn drop(&mut self) { unsafe { sys::hala_scene_free(self.h) } } }
impl HalaRenderer {
  pub fn set_native_scene(&mut self, scene: &HalaNativeScene) -> Result<(), HalaRendererError> {
    check(unsafe { sys::hala_rt_set_scene(self.h, sys::hala_scene_get_desc(scene.h)) })
  }
}

/// src/raytracing_program.rs:70-341 — the generic "RT pass" object, over the library's `hala_rtprog_*` exports: a ray batch traced
/// against a committed renderer's acceleration structure.  `desc` is serialised with serde exactly as the reference's
/// HalaRayTracingProgramDesc (:33-47), so an application's existing JSON descriptions load unchanged.
pub struct HalaRayTracingProgram<'a> { h: *mut sys::hala_rtprog, _renderer: std::marker::PhantomData<&'a HalaRenderer> }
impl<'a> HalaRayTracingProgram<'a> {
  /// :85-252 — the renderer stands for logical_device + descriptor_set_layouts
  pub fn new(renderer: &'a HalaRenderer, desc_json: &str, debug_name: &str) -> Result<Self, HalaRendererError> {
    let (d, n) = (CString::new(desc_json).unwrap(), CString::new(debug_name).unwrap());
    let mut h = std::ptr::null_mut();
    check(unsafe { sys::hala_rtprog_create(renderer.h, d.as_ptr(), n.as_ptr(), &mut h) })?;
    Ok(Self { h, _renderer: std::marker::PhantomData })
  }
  /// :264-278 — device addresses of the batch stand in for descriptor sets
  pub fn bind(&mut self, d_rays: *const sys::hala_ray, d_hits: *mut sys::hala_hit) -> Result<(), HalaRendererError> {
    check(unsafe { sys::hala_rtprog_bind(self.h, d_rays, d_hits) })
  }
  /// :285-300 — bytes 0..3 select the hit group: 0 closest hit, 1 any hit
  pub fn push_constants(&mut self, offset: u32, data: &[u8]) -> Result<(), HalaRendererError> {
    check(unsafe { sys::hala_rtprog_push_constants(self.h, offset, data.as_ptr() as *const c_void, data.len()) })
  }
  /// :307-322
  pub fn push_constants_f32(&mut self, offset: u32, data: &[f32]) -> Result<(), HalaRendererError> {
    check(unsafe { sys::hala_rtprog_push_constants_f32(self.h, offset, data.as_ptr(), data.len()) })
  }
  /// :330-332
  pub fn trace_rays(&self, width: u32, height: u32, depth: u32) -> Result<(), HalaRendererError> {
    check(unsafe { sys::hala_rtprog_trace_rays(self.h, width, height, depth, std::ptr::null_mut()) })
  }
  /// :338-340
  pub fn trace_rays_indirect(&self, indirect_device_address: u64) -> Result<(), HalaRendererError> {
    check(unsafe { sys::hala_rtprog_trace_rays_indirect(self.h, indirect_device_address as *const u32, std::ptr::null_mut()) })
  }
  /// RENDER_SPEC 4.7: the k nearest hits of every ray of the bound batch (its hit buffer holds width * height * depth * k records);
  /// `d_counts`: a device array of one word per ray, or null
  pub fn trace_rays_multi(&self, width: u32, height: u32, depth: u32, k: u32, d_counts: *mut u32) -> Result<(), HalaRendererError> {
    check(unsafe { sys::hala_rtprog_trace_rays_multi(self.h, width, height, depth, k, d_counts, std::ptr::null_mut()) })
  }
}
impl<'a> Drop for HalaRayTracingProgram<'a> { fn drop(&mut self) { unsafe { sys::hala_rtprog_destroy(self.h) } } }

/// multi-GPU: one process (or thread) per GPU; rank 0 makes the id, the application hands it to the other ranks
impl HalaRenderer {
  pub fn comm_unique_id() -> Result<[u8; 128], HalaRendererError> {
    let mut id = [0u8; 128];
    check(unsafe { sys::hala_rt_comm_unique_id(id.as_mut_ptr()) })?;
    Ok(id)
  }
  pub fn comm_init_rank(&mut self, id: &[u8; 128], rank: u32, world: u32) -> Result<(), HalaRendererError> { check(unsafe { sys::hala_rt_comm_init_rank(self.h, id.as_ptr(), rank, world) }) }
  /// aov_mask bit k = AOV k (0 accum, 1 albedo, 2 normal, 3 final): RCCL all-gather of the rank's tiles + de-interleave, stream-ordered
  pub fn tile_allgather(&mut self, aov_mask: u32) -> Result<(), HalaRendererError> { check(unsafe { sys::hala_rt_tile_allgather(self.h, aov_mask) }) }
  pub fn tile_allgather_begin(&mut self, aov_mask: u32) -> Result<(), HalaRendererError> { check(unsafe { sys::hala_rt_tile_allgather_begin(self.h, aov_mask) }) }
  pub fn tile_allgather_finish(&mut self) -> Result<(), HalaRendererError> { check(unsafe { sys::hala_rt_tile_allgather_finish(self.h) }) }
}
