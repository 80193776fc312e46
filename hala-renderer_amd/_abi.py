"""ctypes mirror of include/halart.h (the C-ABI boundary of libhalart.so).

Every Structure here is checked against the byte sizes of the reference's #[repr(C)] records
 in tests/test_layouts.py.  Nothing in this module touches the GPU.
"""
import ctypes as C

INVALID_INDEX = 0xFFFFFFFF  # u32::MAX, reference: src/scene/cpu/node.rs:23-25
MAX_CAMERA_COUNT = 8        # reference: src/scene/loader/gpu_uploader.rs:39
MAX_LIGHT_COUNT = 32        # reference: src/scene/loader/gpu_uploader.rs:40
MAX_MORPH_TARGETS = 64      # HALA_MAX_MORPH_TARGETS (docs/RENDER_SPEC.md 17)
MAX_JOINTS = 256            # HALA_MAX_JOINTS


class Vertex(C.Structure):  # src/scene/vertex.rs:2-9, 44 B
    _fields_ = [("position", C.c_float * 3), ("normal", C.c_float * 3),
                ("tangent", C.c_float * 3), ("tex_coord", C.c_float * 2)]


class GpuCamera(C.Structure):  # src/scene/gpu/camera.rs:10-20, 80 B
    _fields_ = [("position", C.c_float * 3), ("_pad0", C.c_float),
                ("right", C.c_float * 3), ("_pad1", C.c_float),
                ("up", C.c_float * 3), ("_pad2", C.c_float),
                ("forward", C.c_float * 3), ("yfov", C.c_float),
                ("focal_distance_or_xmag", C.c_float), ("aperture_or_ymag", C.c_float),
                ("type", C.c_uint32), ("_pad3", C.c_uint32)]


class GpuLight(C.Structure):  # src/scene/gpu/light.rs:7-32, 80 B
    _fields_ = [("intensity", C.c_float * 3), ("_pad0", C.c_float),
                ("position", C.c_float * 3), ("_pad1", C.c_float),
                ("u", C.c_float * 3), ("_pad2", C.c_float),
                ("v", C.c_float * 3), ("radius", C.c_float), ("area", C.c_float),
                ("type", C.c_uint32), ("_pad3", C.c_uint32 * 2)]


class Aabb(C.Structure):  # HalaAABB, gpu_uploader.rs:169-180, 24 B
    _fields_ = [("min", C.c_float * 3), ("max", C.c_float * 3)]


class GpuMaterial(C.Structure):  # src/scene/gpu/material.rs:6-48, 144 B
    _fields_ = [("medium_color", C.c_float * 3), ("medium_density", C.c_float),
                ("medium_anisotropy", C.c_float), ("medium_type", C.c_uint32),
                ("_medium_padding", C.c_float * 2),
                ("base_color", C.c_float * 3), ("opacity", C.c_float),
                ("emission", C.c_float * 3), ("anisotropic", C.c_float),
                ("metallic", C.c_float), ("roughness", C.c_float),
                ("subsurface", C.c_float), ("specular_tint", C.c_float),
                ("sheen", C.c_float), ("sheen_tint", C.c_float),
                ("clearcoat", C.c_float), ("clearcoat_roughness", C.c_float),
                ("clearcoat_tint", C.c_float * 3), ("specular_transmission", C.c_float),
                ("ior", C.c_float), ("ax", C.c_float), ("ay", C.c_float),
                ("base_color_map_index", C.c_uint32), ("normal_map_index", C.c_uint32),
                ("metallic_roughness_map_index", C.c_uint32), ("emission_map_index", C.c_uint32),
                ("type", C.c_uint32)]


class GpuMeshData(C.Structure):  # src/scene/gpu/mesh.rs:32-39, 96 B
    _fields_ = [("transform", C.c_float * 16), ("material_index", C.c_uint32), ("_pad0", C.c_uint32),
                ("vertices", C.c_uint64), ("indices", C.c_uint64), ("_pad1", C.c_uint64)]


class GlobalUniform(C.Structure):  # src/rt_renderer.rs:44-65, 112 B
    _fields_ = [("ground_color", C.c_float * 4), ("sky_color", C.c_float * 4),
                ("resolution", C.c_float * 2), ("max_depth", C.c_uint32), ("rr_depth", C.c_uint32),
                ("frame_index", C.c_uint32), ("camera_index", C.c_uint32), ("env_type", C.c_uint32),
                ("env_map_width", C.c_uint32), ("env_map_height", C.c_uint32),
                ("env_total_sum", C.c_float), ("env_rotation", C.c_float), ("env_intensity", C.c_float),
                ("exposure_value", C.c_float), ("enable_tonemap", C.c_uint32), ("enable_aces", C.c_uint32),
                ("use_simple_aces", C.c_uint32), ("num_of_lights", C.c_uint32), ("_pad", C.c_uint32 * 3)]


class NodeDesc(C.Structure):  # src/scene/cpu/node.rs:2-12
    _fields_ = [("name", C.c_char_p), ("parent", C.c_int32), ("local_transform", C.c_float * 16),
                ("mesh_index", C.c_uint32), ("camera_index", C.c_uint32), ("light_index", C.c_uint32)]


class PrimitiveDesc(C.Structure):  # src/scene/cpu/mesh.rs:6-13
    _fields_ = [("indices", C.POINTER(C.c_uint32)), ("index_count", C.c_uint32),
                ("vertices", C.POINTER(Vertex)), ("vertex_count", C.c_uint32),
                ("material_index", C.c_uint32)]


class MeshDesc(C.Structure):
    _fields_ = [("primitives", C.POINTER(PrimitiveDesc)), ("primitive_count", C.c_uint32)]


class MaterialDesc(C.Structure):  # src/scene/cpu/material.rs:24-50, :75-80
    _fields_ = [("type", C.c_uint32), ("base_color", C.c_float * 3), ("opacity", C.c_float),
                ("emission", C.c_float * 3), ("anisotropic", C.c_float), ("metallic", C.c_float),
                ("roughness", C.c_float), ("subsurface", C.c_float), ("specular_tint", C.c_float),
                ("sheen", C.c_float), ("sheen_tint", C.c_float), ("clearcoat", C.c_float),
                ("clearcoat_roughness", C.c_float), ("clearcoat_tint", C.c_float * 3),
                ("specular_transmission", C.c_float), ("ior", C.c_float),
                ("medium_type", C.c_uint32), ("medium_color", C.c_float * 3),
                ("medium_density", C.c_float), ("medium_anisotropy", C.c_float),
                ("base_color_map_index", C.c_uint32), ("emission_map_index", C.c_uint32),
                ("normal_map_index", C.c_uint32), ("metallic_roughness_map_index", C.c_uint32)]


class LightDesc(C.Structure):  # src/scene/cpu/light.rs:30-39
    _fields_ = [("color", C.c_float * 3), ("intensity", C.c_float), ("light_type", C.c_uint32),
                ("param0", C.c_float), ("param1", C.c_float)]


class CameraDesc(C.Structure):  # src/scene/cpu/camera.rs:4-29
    _fields_ = [("type", C.c_uint32), ("aspect", C.c_float), ("yfov", C.c_float), ("znear", C.c_float),
                ("zfar", C.c_float), ("focal_distance", C.c_float), ("aperture", C.c_float),
                ("xmag", C.c_float), ("ymag", C.c_float)]


class ImageDesc(C.Structure):  # src/scene/cpu/image_data.rs:14-20
    _fields_ = [("format", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32),
                ("data", C.c_void_p), ("num_of_bytes", C.c_size_t)]


class IndexPair(C.Structure):
    _fields_ = [("key", C.c_uint32), ("value", C.c_uint32)]


class SceneDesc(C.Structure):  # src/scene/cpu/scene.rs:17-26
    _fields_ = [("nodes", C.POINTER(NodeDesc)), ("node_count", C.c_uint32),
                ("meshes", C.POINTER(MeshDesc)), ("mesh_count", C.c_uint32),
                ("materials", C.POINTER(MaterialDesc)), ("material_count", C.c_uint32),
                ("lights", C.POINTER(LightDesc)), ("light_count", C.c_uint32),
                ("cameras", C.POINTER(CameraDesc)), ("camera_count", C.c_uint32),
                ("texture2image_mapping", C.POINTER(IndexPair)), ("texture_count", C.c_uint32),
                ("image2data_mapping", C.POINTER(IndexPair)), ("image_count", C.c_uint32),
                ("image_data", C.POINTER(ImageDesc)), ("image_data_count", C.c_uint32)]


class Ray(C.Structure):  # 32 B
    _fields_ = [("origin", C.c_float * 3), ("tmin", C.c_float), ("direction", C.c_float * 3), ("tmax", C.c_float)]


class Hit(C.Structure):  # 16 B
    _fields_ = [("t", C.c_float), ("u", C.c_float), ("v", C.c_float), ("prim", C.c_uint32)]


class PointQuery(C.Structure):  # hala_point_query, 16 B (RENDER_SPEC 4.8)
    _fields_ = [("point", C.c_float * 3), ("radius", C.c_float)]


class ClosestPoint(C.Structure):  # hala_closest_point, 32 B
    _fields_ = [("distance", C.c_float), ("u", C.c_float), ("v", C.c_float), ("prim", C.c_uint32), ("point", C.c_float * 3), ("region", C.c_uint32)]


class DistanceGridDesc(C.Structure):  # hala_distance_grid_desc, 36 B (RENDER_SPEC 4.9)
    _fields_ = [("origin", C.c_float * 3), ("spacing", C.c_float), ("dims", C.c_uint32 * 3), ("band", C.c_float), ("flags", C.c_uint32)]


class OcclusionSample(C.Structure):  # hala_occlusion_sample, 32 B (RENDER_SPEC 4.10)
    _fields_ = [("point", C.c_float * 3), ("bias", C.c_float), ("normal", C.c_float * 3), ("reach", C.c_float)]


class Occlusion(C.Structure):  # hala_occlusion, 16 B
    _fields_ = [("visibility", C.c_float), ("bent", C.c_float * 3)]


class BakeDesc(C.Structure):  # hala_bake_desc, 28 B (RENDER_SPEC 4.11)
    _fields_ = [("instance", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("flags", C.c_uint32), ("bias", C.c_float), ("reach", C.c_float),
                ("margin", C.c_uint32)]


class BakeTexel(C.Structure):  # hala_bake_texel, 16 B
    _fields_ = [("u", C.c_float), ("v", C.c_float), ("prim", C.c_uint32), ("source", C.c_uint32)]


class BakeChart(C.Structure):  # hala_bake_chart, 24 B (RENDER_SPEC 4.12)
    _fields_ = [("instance", C.c_uint32), ("flags", C.c_uint32), ("scale", C.c_float * 2), ("offset", C.c_float * 2)]


class BakeAtlasDesc(C.Structure):  # hala_bake_atlas_desc, 24 B
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("bias", C.c_float), ("reach", C.c_float), ("margin", C.c_uint32), ("chart_count", C.c_uint32)]


class BakeTransferDesc(C.Structure):  # hala_bake_transfer_desc, 16 B (RENDER_SPEC 4.13)
    _fields_ = [("front", C.c_float), ("back", C.c_float), ("flags", C.c_uint32), ("target_count", C.c_uint32)]


class BakeTransferHit(C.Structure):  # hala_bake_transfer_hit, 32 B
    _fields_ = [("t", C.c_float), ("u", C.c_float), ("v", C.c_float), ("prim", C.c_uint32), ("normal", C.c_float * 3), ("height", C.c_float)]


class RtInfo(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32)]


class RtStatistics(C.Structure):
    _fields_ = [("total_frames", C.c_uint64), ("last_gpu_ms", C.c_double), ("rays_last_update", C.c_uint64),
                ("rays_total", C.c_uint64), ("traverse_ms_last_update", C.c_double),
                ("gpu_ms_total", C.c_double), ("traverse_closest_ms_total", C.c_double),
                ("traverse_shadow_ms_total", C.c_double), ("traverse_closest_launches", C.c_uint64),
                ("traverse_shadow_launches", C.c_uint64), ("updates_rendered", C.c_uint64),
                ("rays_closest_total", C.c_uint64), ("rays_shadow_total", C.c_uint64),
                ("nodes_closest_total", C.c_uint64), ("tris_closest_total", C.c_uint64),
                ("nodes_shadow_total", C.c_uint64), ("tris_shadow_total", C.c_uint64),
                ("rays_closest_counted", C.c_uint64), ("rays_shadow_counted", C.c_uint64),
                ("wave_steps_closest_total", C.c_uint64), ("leaf_passes_closest_total", C.c_uint64), ("leaf_lanes_closest_total", C.c_uint64),
                ("wave_steps_shadow_total", C.c_uint64), ("leaf_passes_shadow_total", C.c_uint64), ("leaf_lanes_shadow_total", C.c_uint64),
                ("traverse_primary_ms_total", C.c_double), ("traverse_primary_launches", C.c_uint64),
                ("nodes_primary_total", C.c_uint64), ("tris_primary_total", C.c_uint64), ("rays_primary_counted", C.c_uint64),
                ("rays_primary_total", C.c_uint64),
                ("rays_closest_timed", C.c_uint64), ("rays_primary_timed", C.c_uint64), ("rays_shadow_timed", C.c_uint64),
                ("shade_ms_total", C.c_double), ("shade_launches", C.c_uint64),
                ("traverse_fused_ms_total", C.c_double), ("traverse_fused_launches", C.c_uint64),
                ("rays_fused_closest_timed", C.c_uint64), ("rays_fused_shadow_timed", C.c_uint64)]


class BuildOptions(C.Structure):  # hala_rt_build_options
    _fields_ = [("builder", C.c_uint32), ("ploc_tail", C.c_uint32), ("ploc_look_every", C.c_uint32),
                ("collapse_look_every", C.c_uint32), ("instancing", C.c_uint32), ("texture_bundles", C.c_uint32), ("instance_levels", C.c_uint32),
                ("reserved", C.c_uint32 * 1)]


class TextureBundleInfo(C.Structure):  # hala_texture_bundle_info, 24 B
    _fields_ = [("bundle_count", C.c_uint32), ("bundled_materials", C.c_uint32), ("unbundled_textured_materials", C.c_uint32),
                ("reserved", C.c_uint32), ("bundle_bytes", C.c_uint64)]


class BvhInfo(C.Structure):
    _fields_ = [("node_count", C.c_uint32), ("triangle_count", C.c_uint32), ("max_depth", C.c_uint32),
                ("lds_node_count", C.c_uint32), ("scene_min", C.c_float * 3), ("scene_max", C.c_float * 3),
                ("node_width", C.c_uint32), ("stored_triangle_count", C.c_uint32), ("instance_node_count", C.c_uint32),
                ("instance_ref_count", C.c_uint32), ("tree_bytes", C.c_uint64)]


class RtProgDescInfo(C.Structure):
    _fields_ = [("raygen_count", C.c_uint32), ("miss_count", C.c_uint32), ("hit_count", C.c_uint32),
                ("callable_count", C.c_uint32), ("push_constant_size", C.c_uint32),
                ("binding_count", C.c_uint32), ("ray_recursion_depth", C.c_uint32)]


class DenoiseParams(C.Structure):  # hala_denoise_params, 32 B (docs/RENDER_SPEC.md 10)
    _fields_ = [("iterations", C.c_uint32), ("sigma_color", C.c_float), ("sigma_albedo", C.c_float),
                ("normal_power", C.c_uint32), ("demodulate", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class AdaptiveParams(C.Structure):  # hala_adaptive_params, 32 B (docs/RENDER_SPEC.md 11)
    _fields_ = [("threshold", C.c_float), ("min_samples", C.c_uint32), ("interval", C.c_uint32), ("reserved", C.c_uint32 * 5)]


class AdaptiveStatus(C.Structure):  # hala_adaptive_status, 32 B
    _fields_ = [("enabled", C.c_uint32), ("active_blocks", C.c_uint32), ("total_blocks", C.c_uint32), ("active_pixels", C.c_uint32),
                ("samples", C.c_uint32), ("last_snapshot", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class LightGroups(C.Structure):  # hala_light_groups, 32 B (docs/RENDER_SPEC.md 14)
    _fields_ = [("group_count", C.c_uint32), ("environment_group", C.c_uint32), ("light_count", C.c_uint32),
                ("material_count", C.c_uint32), ("light_group", C.POINTER(C.c_uint32)), ("material_group", C.POINTER(C.c_uint32))]


class CryptomatteDesc(C.Structure):  # hala_cryptomatte_desc, 24 B (docs/RENDER_SPEC.md 15)
    _fields_ = [("layer_mask", C.c_uint32), ("material_name_count", C.c_uint32), ("material_names", C.POINTER(C.c_char_p)),
                ("reserved", C.c_uint32 * 2)]


class TemporalParams(C.Structure):  # hala_temporal_params, 32 B (docs/RENDER_SPEC.md 16)
    _fields_ = [("max_history", C.c_float), ("tol", C.c_float), ("min_weight", C.c_float), ("reserved", C.c_uint32 * 5)]


class TemporalClampParams(C.Structure):  # hala_temporal_clamp_params, 16 B (docs/RENDER_SPEC.md 16 "History clamp")
    _fields_ = [("radius", C.c_uint32), ("gamma", C.c_float), ("reserved", C.c_uint32 * 2)]


class DeformerDesc(C.Structure):  # hala_deformer_desc, 64 B (docs/RENDER_SPEC.md 17)
    _fields_ = [("mesh_index", C.c_uint32), ("primitive_index", C.c_uint32), ("target_count", C.c_uint32),
                ("target_position_deltas", C.POINTER(C.c_float)), ("target_normal_deltas", C.POINTER(C.c_float)),
                ("target_tangent_deltas", C.POINTER(C.c_float)), ("joint_count", C.c_uint32),
                ("joints", C.POINTER(C.c_uint16)), ("weights", C.POINTER(C.c_float))]


class ShutterParams(C.Structure):  # hala_shutter_params, 32 B (docs/RENDER_SPEC.md 18)
    _fields_ = [("shutter_open", C.c_float), ("shutter_close", C.c_float), ("time_stride", C.c_uint32), ("reserved", C.c_uint32 * 5)]


class ShutterStatus(C.Structure):  # hala_shutter_status, 32 B
    _fields_ = [("enabled", C.c_uint32), ("time_stride", C.c_uint32), ("step", C.c_uint32), ("time", C.c_float), ("steps", C.c_uint64),
                ("reserved", C.c_uint32 * 2)]


class NodeRefitStatus(C.Structure):  # hala_node_refit_status, 40 B (docs/RENDER_SPEC.md 20)
    _fields_ = [("bound_nodes", C.c_uint32), ("affected_nodes", C.c_uint32), ("affected_instances", C.c_uint32), ("levels", C.c_uint32),
                ("last_path", C.c_uint32), ("last_reason", C.c_uint32), ("device_refits", C.c_uint64), ("host_refits", C.c_uint64)]


NODE_REFIT_PATH_NONE, NODE_REFIT_PATH_DEVICE, NODE_REFIT_PATH_HOST = 0, 1, 2
NODE_REFIT_PENDING_EDIT, NODE_REFIT_SHUTTER_KEYS, NODE_REFIT_CAMERA_OR_LIGHT, NODE_REFIT_HOST_LEVELS, NODE_REFIT_CLASSIFICATION = 1, 2, 3, 4, 5
NODE_REFIT_POLICY_REBUILD = 6


class RefitPolicy(C.Structure):  # hala_refit_policy, 16 B (docs/RENDER_SPEC.md 4.6)
    _fields_ = [("mode", C.c_uint32), ("max_inflation", C.c_float), ("reserved", C.c_uint32 * 2)]


class TreeQuality(C.Structure):  # hala_tree_quality, 48 B
    _fields_ = [("first_node", C.c_uint32), ("node_count", C.c_uint32), ("valid", C.c_uint32), ("rebuilt_last_refit", C.c_uint32),
                ("node_q_built", C.c_uint64), ("tri_q_built", C.c_uint64), ("node_q_now", C.c_uint64), ("tri_q_now", C.c_uint64)]


REFIT_POLICY_OFF, REFIT_POLICY_THRESHOLD, REFIT_POLICY_ALWAYS, REFIT_POLICY_MEASURE = 0, 1, 2, 3

# the rig of a glTF file (docs/RENDER_SPEC.md 19; include/halart.h "The rig of a glTF file")
RIG_STEP, RIG_LINEAR, RIG_CUBICSPLINE = 0, 1, 2
RIG_TRANSLATION, RIG_ROTATION, RIG_SCALE, RIG_WEIGHTS = 0, 1, 2, 3


class RigNode(C.Structure):  # hala_rig_node, 112 B
    _fields_ = [("parent", C.c_int32), ("is_matrix", C.c_uint32), ("local_transform", C.c_float * 16), ("translation", C.c_float * 3),
                ("rotation", C.c_float * 4), ("scale", C.c_float * 3)]


class RigSkin(C.Structure):  # hala_rig_skin, 24 B
    _fields_ = [("joint_count", C.c_uint32), ("reserved", C.c_uint32), ("joints", C.POINTER(C.c_uint32)), ("inverse_bind_matrices", C.POINTER(C.c_float))]


class RigBinding(C.Structure):  # hala_rig_binding, 88 B
    _fields_ = [("mesh_index", C.c_uint32), ("primitive_index", C.c_uint32), ("node", C.c_uint32), ("node_count", C.c_uint32), ("skin", C.c_uint32),
                ("vertex_count", C.c_uint32), ("influence_sets", C.c_uint32), ("target_count", C.c_uint32), ("joints", C.POINTER(C.c_uint16)),
                ("weights", C.POINTER(C.c_float)), ("target_position_deltas", C.POINTER(C.c_float)), ("target_normal_deltas", C.POINTER(C.c_float)),
                ("target_tangent_deltas", C.POINTER(C.c_float)), ("default_weights", C.POINTER(C.c_float)), ("weight_first", C.c_uint32),
                ("palette_first", C.c_uint32)]


class RigSampler(C.Structure):  # hala_rig_sampler, 32 B
    _fields_ = [("times", C.POINTER(C.c_float)), ("values", C.POINTER(C.c_float)), ("key_count", C.c_uint32), ("interpolation", C.c_uint32),
                ("width", C.c_uint32), ("reserved", C.c_uint32)]


class RigChannel(C.Structure):  # hala_rig_channel, 16 B
    _fields_ = [("sampler", C.c_uint32), ("node", C.c_uint32), ("path", C.c_uint32), ("reserved", C.c_uint32)]


class RigClip(C.Structure):  # hala_rig_clip, 40 B
    _fields_ = [("name", C.c_char_p), ("samplers", C.POINTER(RigSampler)), ("channels", C.POINTER(RigChannel)), ("sampler_count", C.c_uint32),
                ("channel_count", C.c_uint32), ("time_first", C.c_float), ("time_last", C.c_float)]


class RigDesc(C.Structure):  # hala_rig_desc, 72 B
    _fields_ = [("node_count", C.c_uint32), ("gltf_node_count", C.c_uint32), ("nodes", C.POINTER(RigNode)), ("node_of_gltf", C.POINTER(C.c_uint32)),
                ("skins", C.POINTER(RigSkin)), ("bindings", C.POINTER(RigBinding)), ("clips", C.POINTER(RigClip)), ("skin_count", C.c_uint32),
                ("binding_count", C.c_uint32), ("clip_count", C.c_uint32), ("weight_floats", C.c_uint32), ("palette_floats", C.c_uint32),
                ("reserved", C.c_uint32)]


class RigStatus(C.Structure):  # hala_rig_status, 32 B
    _fields_ = [("bindings", C.c_uint32), ("deformers", C.c_uint32), ("pose_launches", C.c_uint64), ("segments_posed", C.c_uint64),
                ("batch_launches", C.c_uint64)]


class DeformerNormalsInfo(C.Structure):  # hala_deformer_normals_info, 24 B (docs/RENDER_SPEC.md 17 "Recomputed normals")
    _fields_ = [("mode", C.c_uint32), ("class_count", C.c_uint32), ("entry_count", C.c_uint32), ("reserved", C.c_uint32), ("launches", C.c_uint64)]


DEFORM_NORMALS_AS_POSED, DEFORM_NORMALS_RECOMPUTED = 0, 1

# argtypes / restype of the denoise, adaptive sampling, view and AOV entry points (load_library installs them)
PROTOTYPES = {
    "hala_rt_trace_rays_multi": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p], C.c_int),
    "hala_rt_trace_rays_multi_host": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32], C.c_int),
    "hala_rt_closest_points": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p], C.c_int),
    "hala_rt_closest_points_host": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32], C.c_int),
    "hala_rt_closest_points_counted": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p], C.c_int),
    "hala_rt_distance_grid": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "hala_rt_distance_grid_host": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "hala_rt_distance_grid_counted": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    # renderer, samples, out, masks | count, rays, seed (, stream)
    "hala_rt_occlusion": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p], C.c_int),
    "hala_rt_occlusion_host": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32], C.c_int),
    # renderer, desc, samples | out, texels (, stream); the occlusion forms take rays, seed behind desc
    "hala_rt_bake_samples": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "hala_rt_bake_samples_host": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "hala_rt_bake_occlusion": ([C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "hala_rt_bake_occlusion_host": ([C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p], C.c_int),
    # the atlas forms (RENDER_SPEC 4.12): the chart table follows the description
    "hala_rt_bake_atlas_samples": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "hala_rt_bake_atlas_samples_host": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "hala_rt_bake_atlas_occlusion": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "hala_rt_bake_atlas_occlusion_host": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p], C.c_int),
    "hala_rt_bake_transfer": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "hala_rt_bake_transfer_host": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "hala_rtprog_trace_rays_multi": ([C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p], C.c_int),
    "hala_denoise_default_params": ([C.POINTER(DenoiseParams)], None),
    "hala_rt_denoise": ([C.c_void_p, C.POINTER(DenoiseParams), C.POINTER(C.c_float)], C.c_int),
    "hala_rt_read_denoised": ([C.c_void_p, C.POINTER(C.c_float)], C.c_int),
    "hala_rt_get_denoised_buffer": ([C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)], C.c_int),
    "hala_rt_save_denoised": ([C.c_void_p, C.c_char_p], C.c_int),
    "hala_denoise_images": ([C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint32, C.c_uint32,
                             C.POINTER(DenoiseParams), C.POINTER(C.c_float)], C.c_int),
    "hala_adaptive_default_params": ([C.POINTER(AdaptiveParams)], None),
    "hala_rt_set_adaptive_sampling": ([C.c_void_p, C.POINTER(AdaptiveParams)], C.c_int),
    "hala_rt_read_sample_counts": ([C.c_void_p, C.POINTER(C.c_uint32)], C.c_int),
    "hala_rt_get_adaptive_status": ([C.c_void_p, C.POINTER(AdaptiveStatus)], C.c_int),
    "hala_rt_set_views": ([C.c_void_p, C.POINTER(C.c_uint32), C.c_uint32], C.c_int),
    "hala_rt_read_view_image": ([C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_float)], C.c_int),
    "hala_rt_set_aovs": ([C.c_void_p, C.c_uint32], C.c_int),
    "hala_rt_set_light_groups": ([C.c_void_p, C.POINTER(LightGroups)], C.c_int),
    "hala_rt_read_light_group": ([C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)], C.c_int),
    "hala_rt_relight": ([C.c_void_p, C.c_uint32, C.POINTER(C.c_float), C.c_uint32], C.c_int),
    "hala_rt_read_relit": ([C.c_void_p, C.c_int, C.POINTER(C.c_float)], C.c_int),
    "hala_rt_get_relit_buffer": ([C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)], C.c_int),
    "hala_rt_set_cryptomatte": ([C.c_void_p, C.POINTER(CryptomatteDesc)], C.c_int),
    "hala_rt_read_cryptomatte": ([C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)], C.c_int),
    "hala_rt_read_cryptomatte_records": ([C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)], C.c_int),
    "hala_rt_get_cryptomatte_manifest": ([C.c_void_p, C.c_uint32, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)], C.c_int),
    "hala_rt_save_cryptomatte": ([C.c_void_p, C.c_uint32, C.c_char_p], C.c_int),
    "hala_cryptomatte_hash": ([C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)], C.c_int),
    "hala_write_exr": ([C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(C.POINTER(C.c_float)), C.c_uint32,
                        C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)], C.c_int),
    "hala_rt_texture_bundle_info": ([C.c_void_p, C.POINTER(TextureBundleInfo)], C.c_int),
    "hala_temporal_default_params": ([C.POINTER(TemporalParams)], None),
    "hala_rt_set_temporal": ([C.c_void_p, C.POINTER(TemporalParams)], C.c_int),
    "hala_rt_set_temporal_vertex_motion": ([C.c_void_p, C.c_int], C.c_int),
    "hala_temporal_clamp_default_params": ([C.POINTER(TemporalClampParams)], None),
    "hala_rt_set_temporal_clamp": ([C.c_void_p, C.POINTER(TemporalClampParams)], C.c_int),
    "hala_rt_temporal_capture": ([C.c_void_p], C.c_int),
    "hala_rt_temporal_resolve": ([C.c_void_p, C.POINTER(C.c_float)], C.c_int),
    "hala_rt_read_temporal": ([C.c_void_p, C.c_int, C.POINTER(C.c_float)], C.c_int),
    "hala_rt_get_temporal_buffer": ([C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)], C.c_int),
    "hala_rt_denoise_temporal": ([C.c_void_p, C.POINTER(DenoiseParams), C.POINTER(C.c_float)], C.c_int),
    "hala_rt_set_deformer": ([C.c_void_p, C.POINTER(DeformerDesc)], C.c_int),
    "hala_rt_update_deformer": ([C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_float), C.c_uint32], C.c_int),
    "hala_rt_clear_deformer": ([C.c_void_p, C.c_uint32, C.c_uint32], C.c_int),
    "hala_rt_read_vertices": ([C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)], C.c_int),
    "hala_rt_set_deformer_normals": ([C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32], C.c_int),
    "hala_rt_get_deformer_normals": ([C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(DeformerNormalsInfo)], C.c_int),
    "hala_shutter_default_params": ([C.POINTER(ShutterParams)], None),
    "hala_rt_set_shutter": ([C.c_void_p, C.POINTER(ShutterParams)], C.c_int),
    "hala_rt_get_shutter_status": ([C.c_void_p, C.POINTER(ShutterStatus)], C.c_int),
    "hala_rt_set_node_keys": ([C.c_void_p, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float)], C.c_int),
    "hala_rt_set_deformer_keys": ([C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint32,
                                   C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint32], C.c_int),
    "hala_rt_set_vertex_keys": ([C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32], C.c_int),
    "hala_scene_get_rig": ([C.c_void_p], C.POINTER(RigDesc)),
    "hala_rig_sample_clip": ([C.POINTER(RigDesc), C.c_uint32, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)], C.c_int),
    "hala_rt_set_rig": ([C.c_void_p, C.POINTER(RigDesc)], C.c_int),
    "hala_rt_pose_rig": ([C.c_void_p, C.c_uint32, C.c_float], C.c_int),
    "hala_rt_key_rig": ([C.c_void_p, C.c_uint32, C.c_float, C.c_float], C.c_int),
    "hala_rt_get_rig_pose": ([C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float),
                              C.POINTER(C.c_float)], C.c_int),
    "hala_rt_get_rig_status": ([C.c_void_p, C.POINTER(RigStatus)], C.c_int),
    "hala_rt_bind_nodes": ([C.c_void_p, C.POINTER(C.c_uint32), C.c_uint32], C.c_int),
    "hala_rt_refit_nodes": ([C.c_void_p, C.c_void_p, C.c_int], C.c_int),
    "hala_rt_get_node_refit_status": ([C.c_void_p, C.POINTER(NodeRefitStatus)], C.c_int),
    "hala_rt_set_refit_policy": ([C.c_void_p, C.POINTER(RefitPolicy)], C.c_int),
    "hala_rt_get_tree_quality": ([C.c_void_p, C.POINTER(TreeQuality), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                  C.POINTER(C.c_uint64)], C.c_int),
    "hala_rt_variant_ledger": ([C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_int], C.c_int),
    "hala_rt_selftest_math": ([C.c_int, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)], C.c_int),
    "hala_rt_selftest_math_values": ([C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)], C.c_int),
    "hala_rt_selftest_collapse": ([C.c_uint32, C.c_uint32] + [C.c_void_p] * 12 + [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)], C.c_int),
    # count, boxes, pad, builder, ploc_tail, ploc_look_every | sorted_ids, left, right, first, last, node_parent, leaf_parent, node_boxes
    "hala_rt_selftest_hierarchy": ([C.c_uint32, C.c_void_p, C.c_float, C.c_uint32, C.c_uint32, C.c_uint32] + [C.c_void_p] * 8, C.c_int),
}

# hala_rt_variant_ledger: the kernel families in the order of its `family`, each with its flags, first flag = bit 0 of a combination's index
VARIANT_FAMILIES = [
    ("k_trace_primary", ("COUNT", "STAGED", "INST", "VIEWS", "FAR")),
    ("k_trace_batch", ("ANY", "COUNT", "ALPHA", "STAGED", "INST")),
    ("k_trace_shadow", ("COUNT", "ALPHA", "STAGED", "INST", "GROUPS")),
    ("k_trace_shadow_then_batch", ("ALPHA", "STAGED", "INST", "GROUPS")),
    ("k_shade", ("PRIMARY", "SIMPLE", "SCATTER", "AOV", "GROUPS")),
    ("k_resolve", ("AOV", "GROUPS")),
]


# numpy dtypes of the batch records
import numpy as _np

RAY_DTYPE = _np.dtype([("origin", "<f4", 3), ("tmin", "<f4"), ("direction", "<f4", 3), ("tmax", "<f4")])
HIT_DTYPE = _np.dtype([("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("prim", "<u4")])
# RENDER_SPEC 4.8: hala_point_query (16 B), hala_closest_point (32 B)
POINT_QUERY_DTYPE = _np.dtype([("point", "<f4", 3), ("radius", "<f4")])
CLOSEST_POINT_DTYPE = _np.dtype([("distance", "<f4"), ("u", "<f4"), ("v", "<f4"), ("prim", "<u4"), ("point", "<f4", 3), ("region", "<u4")])
# RENDER_SPEC 4.10: hala_occlusion_sample (32 B), hala_occlusion (16 B)
OCCLUSION_SAMPLE_DTYPE = _np.dtype([("point", "<f4", 3), ("bias", "<f4"), ("normal", "<f4", 3), ("reach", "<f4")])
OCCLUSION_DTYPE = _np.dtype([("visibility", "<f4"), ("bent", "<f4", 3)])
# RENDER_SPEC 4.11: hala_bake_texel (16 B)
BAKE_TEXEL_DTYPE = _np.dtype([("u", "<f4"), ("v", "<f4"), ("prim", "<u4"), ("source", "<u4")])
# RENDER_SPEC 4.12: hala_bake_chart (24 B)
BAKE_CHART_DTYPE = _np.dtype([("instance", "<u4"), ("flags", "<u4"), ("scale", "<f4", 2), ("offset", "<f4", 2)])
# RENDER_SPEC 4.13: hala_bake_transfer_hit (32 B)
BAKE_TRANSFER_HIT_DTYPE = _np.dtype([("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("prim", "<u4"), ("normal", "<f4", 3), ("height", "<f4")])
VERTEX_DTYPE = _np.dtype([("position", "<f4", 3), ("normal", "<f4", 3), ("tangent", "<f4", 3), ("tex_coord", "<f4", 2)])

# every symbol include/halart.h declares (tests/test_abi.py checks the .so exports all of them)
EXPORTS = [
    "hala_last_error_message", "hala_rt_create", "hala_rt_destroy",
    "hala_rt_push_general_shader", "hala_rt_push_general_shader_with_file",
    "hala_rt_push_hit_shaders", "hala_rt_push_hit_shaders_with_file",
    "hala_rt_load_blue_noise_texture", "hala_rt_load_blue_noise_pixels", "hala_rt_set_scene", "hala_rt_set_envmap_pixels",
    "hala_rt_set_envmap_file", "hala_rt_set_ground_color", "hala_rt_set_sky_color",
    "hala_rt_set_env_intensity", "hala_rt_set_exposure_value", "hala_rt_commit", "hala_rt_set_build_options", "hala_rt_update", "hala_rt_update_batch",
    "hala_rt_render", "hala_rt_wait_idle", "hala_rt_save_images", "hala_rt_read_image",
    "hala_rt_get_info", "hala_rt_get_statistics", "hala_rt_set_counting", "hala_rt_set_launch_timing_period", "hala_rt_set_pass_fusion", "hala_rt_set_frames_in_flight", "hala_rt_frames_in_flight_info", "hala_rt_reset_accumulation", "hala_rt_get_global_uniform",
    "hala_rt_get_packed_cameras", "hala_rt_get_packed_lights", "hala_rt_get_packed_materials",
    "hala_rt_get_packed_primitives", "hala_rt_get_env_distribution", "hala_rt_get_texture_info",
    "hala_rt_read_texture_level", "hala_rt_sample_texture_host", "hala_rt_set_tile_shard",
    "hala_rt_tile_buffer", "hala_rt_get_stream", "hala_rt_scatter_gathered_tiles", "hala_rt_scatter_gathered_tiles_on_stream", "hala_rt_trace_rays",
    "hala_rt_trace_rays_host", "hala_rt_trace_rays_indirect", "hala_rt_get_bvh_info", "hala_rt_download_bvh", "hala_rt_download_instance_refs",
    "hala_rt_update_node_transform", "hala_rt_update_vertices", "hala_rt_update_material", "hala_rt_refit", "hala_envmap_build_distribution",
    "hala_tonemap_pixels", "hala_write_pfm", "hala_rtprog_parse_desc", "hala_version",
    "hala_scene_load_gltf", "hala_scene_get_desc", "hala_scene_free", "hala_load_float_image",
    "hala_rtprog_create", "hala_rtprog_destroy", "hala_rtprog_get_desc_info", "hala_rtprog_bind", "hala_rtprog_push_constants",
    "hala_rtprog_push_constants_f32", "hala_rtprog_trace_rays", "hala_rtprog_trace_rays_indirect",
    "hala_rt_comm_unique_id", "hala_rt_comm_init_rank", "hala_rt_comm_attach", "hala_rt_comm_destroy",
    "hala_rt_tile_allgather", "hala_rt_tile_allgather_begin", "hala_rt_tile_allgather_finish", "hala_rt_get_gathered_buffer",
    "hala_rt_tile_allgather_begin_external", "hala_rt_get_exchange_buffers",
    "hala_denoise_default_params", "hala_rt_denoise", "hala_rt_read_denoised", "hala_rt_get_denoised_buffer", "hala_rt_save_denoised",
    "hala_denoise_images",
    "hala_adaptive_default_params", "hala_rt_set_adaptive_sampling", "hala_rt_read_sample_counts", "hala_rt_get_adaptive_status",
    "hala_rt_set_views", "hala_rt_read_view_image", "hala_rt_set_aovs",
    "hala_rt_set_light_groups", "hala_rt_read_light_group", "hala_rt_relight", "hala_rt_read_relit", "hala_rt_get_relit_buffer",
    "hala_rt_set_cryptomatte", "hala_rt_read_cryptomatte", "hala_rt_read_cryptomatte_records", "hala_rt_get_cryptomatte_manifest",
    "hala_rt_save_cryptomatte", "hala_cryptomatte_hash", "hala_write_exr",
    "hala_temporal_default_params", "hala_rt_set_temporal", "hala_rt_temporal_capture", "hala_rt_temporal_resolve", "hala_rt_read_temporal",
    "hala_rt_get_temporal_buffer", "hala_rt_denoise_temporal", "hala_rt_set_temporal_vertex_motion",
    "hala_temporal_clamp_default_params", "hala_rt_set_temporal_clamp",
    "hala_rt_texture_bundle_info",
    "hala_rt_set_deformer", "hala_rt_update_deformer", "hala_rt_clear_deformer", "hala_rt_read_vertices",
    "hala_rt_set_deformer_normals", "hala_rt_get_deformer_normals",
    "hala_shutter_default_params", "hala_rt_set_shutter", "hala_rt_get_shutter_status", "hala_rt_set_node_keys", "hala_rt_set_deformer_keys",
    "hala_rt_set_vertex_keys",
    "hala_scene_get_rig", "hala_rig_sample_clip", "hala_rt_set_rig", "hala_rt_pose_rig", "hala_rt_key_rig", "hala_rt_get_rig_pose",
    "hala_rt_get_rig_status",
    "hala_rt_bind_nodes", "hala_rt_refit_nodes", "hala_rt_get_node_refit_status",
    "hala_rt_set_refit_policy", "hala_rt_get_tree_quality",
    "hala_rt_variant_ledger",
    "hala_rt_selftest_math", "hala_rt_selftest_math_values", "hala_rt_selftest_collapse", "hala_rt_selftest_hierarchy",
    "hala_rt_trace_rays_multi", "hala_rt_trace_rays_multi_host", "hala_rtprog_trace_rays_multi",
    "hala_rt_closest_points", "hala_rt_closest_points_host", "hala_rt_closest_points_counted",
    "hala_rt_distance_grid", "hala_rt_distance_grid_host", "hala_rt_distance_grid_counted",
    "hala_rt_occlusion", "hala_rt_occlusion_host",
    "hala_rt_bake_samples", "hala_rt_bake_samples_host", "hala_rt_bake_occlusion", "hala_rt_bake_occlusion_host",
    "hala_rt_bake_atlas_samples", "hala_rt_bake_atlas_samples_host", "hala_rt_bake_atlas_occlusion", "hala_rt_bake_atlas_occlusion_host",
    "hala_rt_bake_transfer", "hala_rt_bake_transfer_host",
]
MAX_MULTI_HITS = 16  # HALA_MAX_MULTI_HITS (RENDER_SPEC 4.7)
MAX_OCCLUSION_RAYS = 256  # HALA_MAX_OCCLUSION_RAYS (RENDER_SPEC 4.10)
MAX_BAKE_DIM, MAX_BAKE_MARGIN, BAKE_SHADING_NORMAL, BAKE_FLIP_NORMAL = 4096, 16, 1, 2  # HALA_MAX_BAKE_*, HALA_BAKE_* (RENDER_SPEC 4.11)
GRID_SIGNED, GRID_METHOD_SHIFT, MAX_GRID_DIM = 1, 1, 1024  # HALA_GRID_* (RENDER_SPEC 4.9)
