"""HalaRenderer — host mirror of the reference's ray-tracing renderer (src/rt_renderer.rs:568-1353) over the
C ABI of libhalart.so.  Method names, argument meaning, call order and error behaviour follow the reference;
every method cites the lines it mirrors.  All compute happens in the HIP library.
"""
import ctypes as C
import os

import numpy as np

from . import _abi as A


class HalaRenderer:
    """reference: `pub struct HalaRenderer` src/rt_renderer.rs:568-617."""

    RAYGEN, MISS, CALLABLE = 0, 1, 2  # shader stages accepted by push_general_shader

    def __init__(self, name, width, height, max_depth, rr_depth, enable_tonemap, enable_aces, use_simple_aces,
                 max_frames, device_ordinal=0):
        """HalaRenderer::new (src/rt_renderer.rs:650-813). `width`/`height` stand for gpu_req.{width,height}
        (:661-662); the winit window is replaced by `device_ordinal` (headless)."""
        from . import check, load_library
        self._lib = load_library()
        self._check = check
        self._device_ordinal = int(device_ordinal)
        self._h = C.c_void_p()
        check(self._lib.hala_rt_create(name.encode(), C.c_uint32(width), C.c_uint32(height), C.c_int(device_ordinal),
                                       C.c_uint32(max_depth), C.c_uint32(rr_depth), C.c_int(bool(enable_tonemap)),
                                       C.c_int(bool(enable_aces)), C.c_int(bool(use_simple_aces)),
                                       C.c_uint64(max_frames), C.byref(self._h)))
        self.width, self.height = width, height

    # -- lifetime ---------------------------------------------------------------------------------------
    def close(self):
        """Drop order of src/rt_renderer.rs:620-633."""
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.hala_rt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- shaders (accepted, validated, recorded; SPIR-V has no meaning for the HIP integrator) -----------
    def push_general_shader(self, code: bytes, stage, group_type=None, debug_name=""):
        """src/rt_renderer.rs:925-957"""
        self._check(self._lib.hala_rt_push_general_shader(self._h, code, C.c_size_t(len(code)), C.c_int(stage), debug_name.encode()))

    def push_general_shader_with_file(self, file_path, stage, group_type=None, debug_name=""):
        """src/rt_renderer.rs:965-995"""
        self._check(self._lib.hala_rt_push_general_shader_with_file(self._h, os.fsencode(file_path), C.c_int(stage), debug_name.encode()))

    def push_hit_shaders(self, closest_code=None, any_hit_code=None, intersection_code=None, debug_name=""):
        """src/rt_renderer.rs:1003-1046"""
        def arg(b):
            return (b, C.c_size_t(len(b))) if b else (None, C.c_size_t(0))
        c, a, i = arg(closest_code), arg(any_hit_code), arg(intersection_code)
        self._check(self._lib.hala_rt_push_hit_shaders(self._h, c[0], c[1], a[0], a[1], i[0], i[1], debug_name.encode()))

    def push_hit_shaders_with_file(self, closest_hit_path=None, any_hit_path=None, intersection_path=None, debug_name=""):
        """src/rt_renderer.rs:1056-1112"""
        enc = lambda p: os.fsencode(p) if p else None  # noqa: E731
        self._check(self._lib.hala_rt_push_hit_shaders_with_file(self._h, enc(closest_hit_path), enc(any_hit_path), enc(intersection_path), debug_name.encode()))

    def load_blue_noise_texture(self, path_or_rgba8):
        """src/rt_renderer.rs:1117-1156: a PNG / JPEG path like the reference, or decoded RGBA8 pixels [H,W,4]; optional in this integrator"""
        if isinstance(path_or_rgba8, (str, bytes, os.PathLike)):
            self._check(self._lib.hala_rt_load_blue_noise_texture(self._h, os.fsencode(path_or_rgba8)))
            return
        px = np.ascontiguousarray(path_or_rgba8, dtype=np.uint8)
        self._check(self._lib.hala_rt_load_blue_noise_pixels(self._h, px.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_uint32(px.shape[1]), C.c_uint32(px.shape[0])))

    # -- scene / environment ------------------------------------------------------------------------------
    def set_scene(self, scene_in_cpu):
        """src/rt_renderer.rs:1161-1178"""
        if hasattr(scene_in_cpu, "desc_ptr"):  # a scene the library loaded itself (NativeScene: hala_scene_load_gltf)
            self._check(self._lib.hala_rt_set_scene(self._h, scene_in_cpu.desc_ptr()))
            return
        holder = scene_in_cpu.to_desc()
        self._check(self._lib.hala_rt_set_scene(self._h, holder.ptr()))
        self._scene = scene_in_cpu  # set_light_groups resolves light node names through it

    def set_envmap(self, path_or_pixels, rotation=0.0):
        """src/rt_renderer.rs:1184-1195. A str/PathLike goes through the library's decoder (.hdr / .pfm);
        an ndarray [H,W,3|4] float32 is the already decoded image."""
        if isinstance(path_or_pixels, (str, bytes, os.PathLike)):
            self._check(self._lib.hala_rt_set_envmap_file(self._h, os.fsencode(path_or_pixels), C.c_float(rotation)))
            return
        px = np.ascontiguousarray(path_or_pixels, dtype=np.float32)
        h, w, ch = px.shape
        self._check(self._lib.hala_rt_set_envmap_pixels(self._h, px.ctypes.data_as(C.POINTER(C.c_float)), C.c_uint32(ch), C.c_uint32(w), C.c_uint32(h), C.c_float(rotation)))

    def set_ground_color(self, color):
        """src/rt_renderer.rs:1199-1201"""
        self._lib.hala_rt_set_ground_color(self._h, (C.c_float * 4)(*color))

    def set_sky_color(self, color):
        """src/rt_renderer.rs:1205-1207"""
        self._lib.hala_rt_set_sky_color(self._h, (C.c_float * 4)(*color))

    def set_env_intensity(self, intensity):
        """src/rt_renderer.rs:1211-1213"""
        self._lib.hala_rt_set_env_intensity(self._h, C.c_float(intensity))

    def set_exposure_value(self, exposure_value):
        """src/rt_renderer.rs:1217-1219"""
        self._lib.hala_rt_set_exposure_value(self._h, C.c_float(exposure_value))

    # -- HalaRendererTrait (src/renderer.rs:210-324) ------------------------------------------------------------
    def commit(self):
        """src/rt_renderer.rs:136-379"""
        self._check(self._lib.hala_rt_commit(self._h))

    BUILDERS = {None: 0, "auto": 0, "sah": 1, "ploc": 2, "lbvh": 3}
    INSTANCE_LEVELS = {None: 0, "host": 0, "gpu": 1}

    def set_build_options(self, builder=None, ploc_tail=0, ploc_look_every=0, collapse_look_every=0, instancing=None, texture_bundles=None,
                          instance_levels=None):
        """how the next commit() builds the acceleration structure (hala_rt_set_build_options): builder = None | "sah" | "ploc" | "lbvh";
        instancing = True: two-level tree (RENDER_SPEC 4.5: primitives referenced by several instances are stored once), False: every
        instance flattened to world space (one tree), None: automatic (flattened up to 2^26 triangles); the other fields only change how the
        host drives the build rounds (same tree); texture_bundles = None / True: the co-sized 8-bit maps of a material are also stored
        interleaved and fetched together (same images, faster shading), False: off; instance_levels = None | "host" | "gpu": where the
        instance levels of a two-level tree are built at commit and rebuilt by every refit and shutter step (same images)"""
        o = A.BuildOptions(builder=self.BUILDERS[builder], ploc_tail=ploc_tail, ploc_look_every=ploc_look_every, collapse_look_every=collapse_look_every,
                           instancing=0 if instancing is None else (2 if instancing else 1),
                           texture_bundles=0 if texture_bundles is None or texture_bundles else 1,
                           instance_levels=self.INSTANCE_LEVELS[instance_levels])
        self._check(self._lib.hala_rt_set_build_options(self._h, C.byref(o)))

    def update(self, delta_time=0.0, width=None, height=None, ui_fn=None):
        """src/rt_renderer.rs:387-471 — one sample per pixel; `ui_fn` is dropped."""
        self._check(self._lib.hala_rt_update(self._h, C.c_double(delta_time), C.c_uint32(width or self.width), C.c_uint32(height or self.height)))

    def update_batch(self, frames: int):
        """`frames` update()s as one wavefront pass (bit-identical result; fewer, larger launches)"""
        self._check(self._lib.hala_rt_update_batch(self._h, C.c_uint32(frames)))

    def render(self):
        """src/rt_renderer.rs:475-502: nothing to present; bounds the updates in flight to two (it does not flush: read_image,
        save_images, statistics and wait_idle wait for the stream themselves)"""
        self._check(self._lib.hala_rt_render(self._h))

    def wait_idle(self):
        """src/renderer.rs:251-256"""
        self._check(self._lib.hala_rt_wait_idle(self._h))

    def save_images(self, path):
        """src/rt_renderer.rs:1224-1352"""
        self._check(self._lib.hala_rt_save_images(self._h, os.fsencode(path)))

    def info(self):
        """src/renderer.rs:212"""
        i = A.RtInfo()
        self._check(self._lib.hala_rt_get_info(self._h, C.byref(i)))
        return i

    def statistics(self):
        """src/renderer.rs:218, :135-207"""
        s = A.RtStatistics()
        self._check(self._lib.hala_rt_get_statistics(self._h, C.byref(s)))
        return s

    def reset_accumulation(self):
        """HalaRendererStatistics::reset (src/renderer.rs:168-174): the next update() renders frame_index 0"""
        self._check(self._lib.hala_rt_reset_accumulation(self._h))

    def set_counting(self, enable: bool):
        """count BVH nodes visited / triangles tested in update() (inputs of the algorithmic-bytes figure)"""
        self._check(self._lib.hala_rt_set_counting(self._h, C.c_int(bool(enable))))

    def set_pass_fusion(self, mode):
        """0: one launch per pass; 1 (default): fused launches except in timed updates; 2: always (timed updates fill traverse_fused_*)"""
        self._check(self._lib.hala_rt_set_pass_fusion(self._h, C.c_uint32(mode)))

    def set_frames_in_flight(self, n):
        """2 (default): untimed updates alternate between two frame slots and overlap; 1: strictly serial — see include/halart.h"""
        self._check(self._lib.hala_rt_set_frames_in_flight(self._h, C.c_uint32(n)))

    def frames_in_flight_info(self):
        """-> (updates that ran on the second frame slot, the second set of wavefront buffers is allocated)"""
        n, b = C.c_ulonglong(0), C.c_uint32(0)
        self._check(self._lib.hala_rt_frames_in_flight_info(self._h, C.byref(n), C.byref(b)))
        return n.value, bool(b.value)

    def set_launch_timing_period(self, period):
        """per-launch HIP events on every `period`-th update (1: all, the default; 0: none) — see include/halart.h"""
        self._check(self._lib.hala_rt_set_launch_timing_period(self._h, C.c_uint32(period)))

    # -- read-back used by tests and bench (what save_images downloads, :1239-1254) -------------------------------
    ACCUM, ALBEDO, NORMAL, FINAL, POSITION, IDS = 0, 1, 2, 3, 4, 5
    IMAGE_NAMES = ("accum", "albedo", "normal", "final", "position", "ids")

    def read_image(self, which=0, view=0) -> np.ndarray:
        """one of the images of `view` (an index into the list set_views gave; 0: the only view by default); `which` is an index or a
        name of IMAGE_NAMES.  4 / 5 only while set_aovs turned them on (5 comes back as float32 bits: read_ids)"""
        if isinstance(which, str):
            which = self.IMAGE_NAMES.index(which)
        out = np.empty((self.height, self.width, 4), dtype=np.float32)
        dst = out.ctypes.data_as(C.POINTER(C.c_float))
        if view == 0:
            self._check(self._lib.hala_rt_read_image(self._h, C.c_int(which), dst))
        else:
            self._check(self._lib.hala_rt_read_view_image(self._h, C.c_uint32(view), C.c_int(which), dst))
        return out

    # -- views (docs/RENDER_SPEC.md 12; include/halart.h "hala_rt_set_views") ---------------------------------------
    def set_views(self, cameras):
        """render every camera index in `cameras` (1..8 entries, each < 8; duplicates allowed) in each update; view v of read_image
        is cameras[v].  [0] is the default.  Restarts the accumulation."""
        idx = [int(c) for c in cameras]
        arr = (C.c_uint32 * max(len(idx), 1))(*idx)
        self._check(self._lib.hala_rt_set_views(self._h, arr, C.c_uint32(len(idx))))

    # -- first-hit AOVs (docs/RENDER_SPEC.md 13; include/halart.h "hala_rt_set_aovs") -------------------------------------------
    def set_aovs(self, position=False, ids=False):
        """turn the first-hit position (image 4) and id (image 5) AOVs on or off.  Restarts the accumulation."""
        self._check(self._lib.hala_rt_set_aovs(self._h, C.c_uint32((1 if position else 0) | (2 if ids else 0))))

    def read_ids(self, view=0) -> np.ndarray:
        """[H, W, 4] uint32: (node, instance, material, triangle id) of the first hit of frame 0's sample; lights: (node, ~0, ~0,
        0x80000000 | light index); misses: all ~0"""
        return self.read_image(self.IDS, view=view).view(np.uint32)

    # -- light groups (docs/RENDER_SPEC.md 14; include/halart.h "hala_rt_set_light_groups") --------------------------------------
    def set_light_groups(self, lights=None, environment=0, materials=None, group_count=None):
        """split the beauty image by emitter.  lights: a list of groups indexed by packed light (the order of packed_lights()), or a dict
        {light node name: group} (every other light: group 0); environment: the environment's group; materials: one group for every
        material (an int), a list indexed by material, or None — then all materials share one group of their own, one past the largest
        group the lights and the environment use.  group_count: None = one past the largest group used.  set_light_groups(None) or no
        arguments at all turns the feature off.  Restarts the accumulation."""
        if lights is None and materials is None and group_count is None and environment == 0:
            self._check(self._lib.hala_rt_set_light_groups(self._h, None))
            self.light_group_count = 0
            return
        n_lights = len(self.packed_lights()[0])
        if isinstance(lights, dict):
            scene = getattr(self, "_scene", None)
            if scene is None or not hasattr(scene, "nodes"):
                raise ValueError("set_light_groups: a dict of light node names needs the HalaScene given to set_scene")
            from .scene import INVALID
            names = [nd.name for nd in scene.nodes if nd.light_index != INVALID]  # packed light order (RENDER_SPEC 7.2)
            unknown = set(lights) - set(names)
            if unknown:
                raise ValueError(f"set_light_groups: no light node named {sorted(unknown)}")
            lg = [int(lights.get(nm, 0)) for nm in names[:n_lights]]
        else:
            lg = [int(x) for x in (lights if lights is not None else [0] * n_lights)]
        used = max(lg + [int(environment)]) + 1
        if materials is None or isinstance(materials, (int, np.integer)):
            n_mat = len(self.packed_materials())
            mg = [used if materials is None else int(materials)] * n_mat
        else:
            mg = [int(x) for x in materials]
        g = A.LightGroups()
        g.group_count = int(group_count) if group_count is not None else max(lg + mg + [int(environment)]) + 1
        g.environment_group = int(environment)
        la, ma = (C.c_uint32 * max(len(lg), 1))(*lg), (C.c_uint32 * max(len(mg), 1))(*mg)
        g.light_count, g.material_count = len(lg), len(mg)
        g.light_group = C.cast(la, C.POINTER(C.c_uint32))
        g.material_group = C.cast(ma, C.POINTER(C.c_uint32))
        self._check(self._lib.hala_rt_set_light_groups(self._h, C.byref(g)))
        self.light_group_count = g.group_count

    def read_light_group(self, group, view=0) -> np.ndarray:
        """[H, W, 4] float32: the running mean of light group `group`'s share of the beauty image (alpha 1)"""
        out = np.empty((self.height, self.width, 4), dtype=np.float32)
        self._check(self._lib.hala_rt_read_light_group(self._h, C.c_uint32(view), C.c_uint32(group), out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def relight(self, scales, view=0):
        """-> (linear, tonemapped) [H, W, 4] float32: sum over the groups of scales[g] * read_light_group(g) on the GPU; scales: one
        RGB triple (or one float) per group, finite, negative values allowed; tonemapped = the renderer's operators on linear * exposure"""
        sc = np.array([np.broadcast_to(np.asarray(s, np.float32), (3,)) for s in scales], dtype=np.float32).reshape(-1)
        self._check(self._lib.hala_rt_relight(self._h, C.c_uint32(view), sc.ctypes.data_as(C.POINTER(C.c_float)), C.c_uint32(len(scales))))
        out = []
        for which in (0, 1):
            img = np.empty((self.height, self.width, 4), dtype=np.float32)
            self._check(self._lib.hala_rt_read_relit(self._h, C.c_int(which), img.ctypes.data_as(C.POINTER(C.c_float))))
            out.append(img)
        return tuple(out)

    def relit_buffer(self, which=0):
        """-> (device address, bytes) of the last relit image (0 linear, 1 tonemapped; zero-copy, on the renderer's stream)"""
        p = C.c_void_p(); n = C.c_size_t()
        self._check(self._lib.hala_rt_get_relit_buffer(self._h, C.c_int(which), C.byref(p), C.byref(n)))
        return p.value, n.value

    # -- Cryptomatte (docs/RENDER_SPEC.md 15; include/halart.h "hala_rt_set_cryptomatte") ------------------------------------------------
    CRYPTO_LAYERS = ("object", "material", "asset")

    def _crypto_layer(self, layer):
        return self.CRYPTO_LAYERS.index(layer) if isinstance(layer, str) else int(layer)

    def set_cryptomatte(self, layers=("object", "material", "asset"), material_names=None):
        """Cryptomatte ID mattes of the layers named ("object", "material", "asset"; None turns the feature off); material_names: a list
        indexed by material (None or "" entries: material<m>).  Restarts the accumulation."""
        if layers is None:
            self._check(self._lib.hala_rt_set_cryptomatte(self._h, None))
            return
        mask = 0
        for layer in layers:
            mask |= 1 << self._crypto_layer(layer)
        names = [None if n is None else str(n).encode("utf-8") for n in (material_names or [])]
        arr = (C.c_char_p * max(len(names), 1))(*names)
        d = A.CryptomatteDesc(layer_mask=mask, material_name_count=len(names), material_names=C.cast(arr, C.POINTER(C.c_char_p)))
        self._check(self._lib.hala_rt_set_cryptomatte(self._h, C.byref(d)))

    def read_cryptomatte(self, layer, view=0):
        """-> (ids float32 [H, W, 6], coverage float32 [H, W, 6]) of ranks 0..5 (an id is the float whose bits are the uint32 id)"""
        out = np.empty((3, self.height, self.width, 4), dtype=np.float32)
        self._check(self._lib.hala_rt_read_cryptomatte(self._h, C.c_uint32(view), C.c_uint32(self._crypto_layer(layer)),
                                                        out.ctypes.data_as(C.POINTER(C.c_float))))
        ids = np.stack([out[r // 2][..., 2 * (r % 2)] for r in range(6)], axis=-1)
        cov = np.stack([out[r // 2][..., 2 * (r % 2) + 1] for r in range(6)], axis=-1)
        return ids, cov

    def read_cryptomatte_records(self, layer, view=0) -> np.ndarray:
        """[H, W, 16] uint32: n, other, (id, count) x 7 of every pixel"""
        out = np.empty((self.height, self.width, 16), dtype=np.uint32)
        self._check(self._lib.hala_rt_read_cryptomatte_records(self._h, C.c_uint32(view), C.c_uint32(self._crypto_layer(layer)),
                                                                out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def cryptomatte_manifest(self, layer) -> dict:
        """{name: 8 lowercase hex digits of the id} of every name the committed scene can produce in the layer"""
        import json
        n = C.c_size_t(0)
        lay = C.c_uint32(self._crypto_layer(layer))
        self._check(self._lib.hala_rt_get_cryptomatte_manifest(self._h, lay, None, C.c_size_t(0), C.byref(n)))
        buf = C.create_string_buffer(n.value + 1)
        self._check(self._lib.hala_rt_get_cryptomatte_manifest(self._h, lay, buf, C.c_size_t(n.value + 1), C.byref(n)))
        return json.loads(buf.raw[:n.value].decode("utf-8"))

    def save_cryptomatte(self, path, view=0):
        """single-part scanline OpenEXR (ZIP): R, G, B, A = the view's accum and three sublayers per enabled layer, with the manifests"""
        self._check(self._lib.hala_rt_save_cryptomatte(self._h, C.c_uint32(view), os.fsencode(path)))

    # -- denoising (docs/RENDER_SPEC.md 10; include/halart.h "hala_rt_denoise") -----------------------------------
    def denoise(self, iterations=None, sigma_color=None, sigma_albedo=None, normal_power=None, demodulate=True, timed=False):
        """filter accum / albedo / normal into the denoised image (stream-ordered; None: the library's default).  timed: wait and
        return the GPU milliseconds of the filter's launches"""
        p = denoise_default_params(iterations=iterations, sigma_color=sigma_color, sigma_albedo=sigma_albedo,
                                   normal_power=normal_power, demodulate=demodulate)
        ms = C.c_float(0.0)
        self._check(self._lib.hala_rt_denoise(self._h, C.byref(p), C.byref(ms) if timed else None))
        return ms.value if timed else None

    def read_denoised(self) -> np.ndarray:
        out = np.empty((self.height, self.width, 4), dtype=np.float32)
        self._check(self._lib.hala_rt_read_denoised(self._h, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def denoised_buffer(self):
        """-> (device address, bytes) of the denoised RGBA32F image (zero-copy; wrap it on the renderer's stream)"""
        p = C.c_void_p(); n = C.c_size_t()
        self._check(self._lib.hala_rt_get_denoised_buffer(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def save_denoised(self, path):
        """<stem>_denoised.pfm, tonemapped on the host like save_images' <stem>_color.pfm"""
        self._check(self._lib.hala_rt_save_denoised(self._h, os.fsencode(path)))

    # -- temporal reprojection (docs/RENDER_SPEC.md 16; include/halart.h "hala_rt_set_temporal") ---------------------------------------
    def set_temporal(self, enable=True, max_history=None, tol=None, min_weight=None):
        """carry the accumulated frame across scene edits (needs set_aovs(position=True, ids=True)); None: the library's default;
        enable=False turns the feature off and frees its buffers.  Does not restart the accumulation."""
        if not enable:
            self._check(self._lib.hala_rt_set_temporal(self._h, None))
            return
        p = temporal_default_params(max_history=max_history, tol=tol, min_weight=min_weight)
        self._check(self._lib.hala_rt_set_temporal(self._h, C.byref(p)))

    def set_temporal_vertex_motion(self, enable=True):
        """let the history follow vertex edits (update_vertices, posed deformers) on a one-level tree: every capture from now on also
        keeps the triangles as they stand (RENDER_SPEC 16 "Vertex motion").  Refused while set_temporal() is off"""
        self._check(self._lib.hala_rt_set_temporal_vertex_motion(self._h, C.c_int(1 if enable else 0)))

    def set_temporal_clamp(self, radius=None, gamma=None, enable=True):
        """clamp the reprojected history of every resolve and capture to gamma standard errors around the mean of the current
        accumulation over the (2 radius + 1)^2 neighbourhood (RENDER_SPEC 16 "History clamp"), so that light an edit changed does not
        lag; None: the library's default; enable=False turns it off.  Refused while set_temporal() is off"""
        if not enable:
            self._check(self._lib.hala_rt_set_temporal_clamp(self._h, None))
            return
        p = temporal_clamp_default_params(radius=radius, gamma=gamma)
        self._check(self._lib.hala_rt_set_temporal_clamp(self._h, C.byref(p)))

    def temporal_capture(self):
        """keep the frame as it stands as the history; call it before update_node_transform / update_vertices / update_material"""
        self._check(self._lib.hala_rt_temporal_capture(self._h))

    def temporal_resolve(self, timed=False):
        """blend the accumulation with the reprojected history (stream-ordered).  timed: wait and return the GPU milliseconds"""
        ms = C.c_float(0.0)
        self._check(self._lib.hala_rt_temporal_resolve(self._h, C.byref(ms) if timed else None))
        return ms.value if timed else None

    def read_temporal(self, which=0) -> np.ndarray:
        """[H, W, 4] float32 of the last resolve: 0 / "temporal" = (rgb, history length + samples), 1 / "motion" = (dx, dy, view depth, 1)"""
        if isinstance(which, str):
            which = ("temporal", "motion").index(which)
        out = np.empty((self.height, self.width, 4), dtype=np.float32)
        self._check(self._lib.hala_rt_read_temporal(self._h, C.c_int(which), out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def temporal_buffer(self, which=0):
        """-> (device address, bytes) of the temporal (0) or motion (1) image (zero-copy, on the renderer's stream)"""
        p = C.c_void_p(); n = C.c_size_t()
        self._check(self._lib.hala_rt_get_temporal_buffer(self._h, C.c_int(which), C.byref(p), C.byref(n)))
        return p.value, n.value

    def denoise_temporal(self, iterations=None, sigma_color=None, sigma_albedo=None, normal_power=None, demodulate=True, timed=False):
        """denoise() with the temporal image of the last resolve as colour; the result is read with read_denoised()"""
        p = denoise_default_params(iterations=iterations, sigma_color=sigma_color, sigma_albedo=sigma_albedo,
                                   normal_power=normal_power, demodulate=demodulate)
        ms = C.c_float(0.0)
        self._check(self._lib.hala_rt_denoise_temporal(self._h, C.byref(p), C.byref(ms) if timed else None))
        return ms.value if timed else None

    # -- adaptive sampling (docs/RENDER_SPEC.md 11; include/halart.h "hala_rt_set_adaptive_sampling") -------------------------------
    def set_adaptive_sampling(self, threshold, min_samples=None, interval=None):
        """stop tracing the 8 x 8 pixel blocks whose error estimate fell below `threshold` (None: turn the feature off); None for
        min_samples / interval: the library's default.  Restarts the accumulation either way."""
        if threshold is None:
            self._check(self._lib.hala_rt_set_adaptive_sampling(self._h, None))
            return
        p = adaptive_default_params(threshold=threshold, min_samples=min_samples, interval=interval)
        self._check(self._lib.hala_rt_set_adaptive_sampling(self._h, C.byref(p)))

    def read_sample_counts(self) -> np.ndarray:
        """[H, W] uint32: the samples folded into each pixel"""
        out = np.empty((self.height, self.width), dtype=np.uint32)
        self._check(self._lib.hala_rt_read_sample_counts(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def adaptive_status(self) -> A.AdaptiveStatus:
        s = A.AdaptiveStatus()
        self._check(self._lib.hala_rt_get_adaptive_status(self._h, C.byref(s)))
        return s

    def global_uniform(self) -> A.GlobalUniform:
        u = A.GlobalUniform()
        self._check(self._lib.hala_rt_get_global_uniform(self._h, C.byref(u)))
        return u

    def packed_cameras(self):
        buf = (A.GpuCamera * A.MAX_CAMERA_COUNT)(); n = C.c_uint32()
        self._check(self._lib.hala_rt_get_packed_cameras(self._h, buf, C.c_uint32(A.MAX_CAMERA_COUNT), C.byref(n)))
        return list(buf[:n.value])

    def packed_lights(self):
        buf = (A.GpuLight * A.MAX_LIGHT_COUNT)(); bb = (A.Aabb * A.MAX_LIGHT_COUNT)(); n = C.c_uint32()
        self._check(self._lib.hala_rt_get_packed_lights(self._h, buf, bb, C.c_uint32(A.MAX_LIGHT_COUNT), C.byref(n)))
        return list(buf[:n.value]), list(bb[:n.value])

    def packed_materials(self, capacity=4096):
        buf = (A.GpuMaterial * capacity)(); n = C.c_uint32()
        self._check(self._lib.hala_rt_get_packed_materials(self._h, buf, C.c_uint32(capacity), C.byref(n)))
        return list(buf[:min(n.value, capacity)])

    def packed_primitives(self, capacity=65536):
        buf = (A.GpuMeshData * capacity)(); t = np.zeros((capacity, 12), dtype=np.float32); n = C.c_uint32()
        self._check(self._lib.hala_rt_get_packed_primitives(self._h, buf, t.ctypes.data_as(C.POINTER(C.c_float)), C.c_uint32(capacity), C.byref(n)))
        k = min(n.value, capacity)
        return list(buf[:k]), t[:k]

    def env_distribution(self, width, height):
        total = C.c_float(); marg = np.empty(height, dtype=np.float32); cond = np.empty((height, width), dtype=np.float32)
        self._check(self._lib.hala_rt_get_env_distribution(self._h, C.byref(total), marg.ctypes.data_as(C.POINTER(C.c_float)), cond.ctypes.data_as(C.POINTER(C.c_float))))
        return total.value, marg, cond

    # -- textures (set 2 binding 0) ---------------------------------------------------------------------------------------
    def texture_info(self, texture):
        w, h, m = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._check(self._lib.hala_rt_get_texture_info(self._h, C.c_uint32(texture), C.byref(w), C.byref(h), C.byref(m)))
        return w.value, h.value, m.value

    def texture_bundle_info(self):
        """texel bundles of the committed scene (hala_rt_texture_bundle_info): bundle_count, bundled_materials,
        unbundled_textured_materials, bundle_bytes"""
        i = A.TextureBundleInfo()
        self._check(self._lib.hala_rt_texture_bundle_info(self._h, C.byref(i)))
        return i

    def read_texture_level(self, texture, level):
        w, h, _ = self.texture_info(texture)
        lw, lh = max(1, w >> level), max(1, h >> level)
        out = np.empty((lh, lw, 4), dtype=np.float32)
        self._check(self._lib.hala_rt_read_texture_level(self._h, C.c_uint32(texture), C.c_uint32(level), out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def sample_texture(self, texture, uv_lod):
        q = np.ascontiguousarray(uv_lod, dtype=np.float32).reshape(-1, 3)
        out = np.empty((q.shape[0], 4), dtype=np.float32)
        self._check(self._lib.hala_rt_sample_texture_host(self._h, C.c_uint32(texture), q.ctypes.data_as(C.POINTER(C.c_float)), C.c_uint32(q.shape[0]),
                                                          out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    # -- ray-batch operator / BVH introspection ----------------------------------------------------------------------
    def trace_rays_host(self, rays: np.ndarray, mode=0, count_steps=False):
        rays = np.ascontiguousarray(rays, dtype=A.RAY_DTYPE)
        hits = np.empty(rays.shape[0], dtype=A.HIT_DTYPE)
        ctr = (C.c_uint64 * 2)(0, 0)
        self._check(self._lib.hala_rt_trace_rays_host(self._h, C.c_void_p(rays.ctypes.data), C.c_void_p(hits.ctypes.data), C.c_uint32(rays.shape[0]), C.c_int(mode), ctr if count_steps else None))
        return (hits, (ctr[0], ctr[1])) if count_steps else hits

    def trace_rays(self, d_rays: int, d_hits: int, count: int, mode=0, d_counters: int = 0, stream: int = 0):
        """device-pointer form: the vkCmdTraceRaysKHR analogue for one ray batch (src/rt_renderer.rs:458-464)"""
        self._check(self._lib.hala_rt_trace_rays(self._h, C.c_void_p(d_rays), C.c_void_p(d_hits), C.c_uint32(count), C.c_int(mode), C.c_void_p(d_counters), C.c_void_p(stream)))

    def trace_rays_multi_host(self, rays: np.ndarray, k: int, want_counts=True):
        """RENDER_SPEC 4.7: (hits[n, k], counts[n]) — the k nearest hits of every ray by (t, triangle id), padded with miss records;
        counts is None with want_counts=False (the library then gets a null counts pointer)"""
        rays = np.ascontiguousarray(rays, dtype=A.RAY_DTYPE)
        n = rays.shape[0]
        hits = np.empty((n, max(int(k), 0)), dtype=A.HIT_DTYPE)
        counts = np.zeros(n, dtype=np.uint32) if want_counts else None
        self._check(self._lib.hala_rt_trace_rays_multi_host(self._h, C.c_void_p(rays.ctypes.data), C.c_void_p(hits.ctypes.data),
                                                            C.c_void_p(counts.ctypes.data) if want_counts else None, C.c_uint32(n), C.c_uint32(k)))
        return hits, counts

    def trace_rays_multi(self, d_rays: int, d_hits: int, count: int, k: int, d_counts: int = 0, stream: int = 0):
        """device-pointer form of RENDER_SPEC 4.7: d_hits holds count * k records, d_counts (or 0) count words"""
        self._check(self._lib.hala_rt_trace_rays_multi(self._h, C.c_void_p(d_rays), C.c_void_p(d_hits), C.c_void_p(d_counts), C.c_uint32(count), C.c_uint32(k),
                                                       C.c_void_p(stream)))

    # -- what the device forms of the query batches share: a tensor or a pointer in, a checked output, a count -----------
    @staticmethod
    def _device_address(x):
        """the device address of a tensor, of a pointer, or 0 for None"""
        return x.data_ptr() if hasattr(x, "data_ptr") else int(x or 0)

    @staticmethod
    def _device_count(x, itemsize, count):
        """the records of a device batch: `count` where given, else what the tensor holds"""
        if count is not None:
            return count
        if not hasattr(x, "data_ptr"):
            raise ValueError("a device pointer needs `count`")
        return x.numel() * x.element_size() // itemsize

    @staticmethod
    def _device_out(x, nbytes, too_small):
        """the device address of an output tensor (or pointer, or None), a tensor checked against the bytes the call writes"""
        if hasattr(x, "data_ptr") and x.numel() * x.element_size() < nbytes:
            raise ValueError(too_small)
        return HalaRenderer._device_address(x)

    def closest_points(self, points, radius=np.inf, out=None, count=None, stream: int = 0, d_counters: int = 0):
        """RENDER_SPEC 4.8: the nearest surface point of every query point within `radius` (a scalar or one per point), as a structured
        array of A.CLOSEST_POINT_DTYPE (distance, u, v, prim, point, region; a miss has distance -1 and prim 0xffffffff).  `points` is
        an [n, 3] array or an array of A.POINT_QUERY_DTYPE (then `radius` is not used).
        Device form: `points` is a device tensor of 16-B queries (or a device pointer, with `count`) and `out` a device tensor (or
        pointer) of 32-B records; the batch is launched on `stream` and nothing is returned.  d_counters (device, 2 x uint64): node
        visits and triangle tests, through the counting variant of the kernel."""
        if out is not None or isinstance(points, int) or hasattr(points, "data_ptr"):
            if out is None:
                raise ValueError("the device form needs `out`")
            d_q = self._device_address(points)
            count = self._device_count(points, A.POINT_QUERY_DTYPE.itemsize, count)
            d_o = self._device_out(out, count * A.CLOSEST_POINT_DTYPE.itemsize, "`out` is too small for the batch")
            if d_counters:
                self._check(self._lib.hala_rt_closest_points_counted(self._h, C.c_void_p(d_q), C.c_void_p(d_o), C.c_uint32(count), C.c_void_p(d_counters),
                                                                     C.c_void_p(stream)))
            else:
                self._check(self._lib.hala_rt_closest_points(self._h, C.c_void_p(d_q), C.c_void_p(d_o), C.c_uint32(count), C.c_void_p(stream)))
            return None
        pts = np.asarray(points)
        if pts.dtype == A.POINT_QUERY_DTYPE:
            q = np.ascontiguousarray(pts).reshape(-1)
        else:
            pts = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3)
            q = np.empty(pts.shape[0], dtype=A.POINT_QUERY_DTYPE)
            q["point"] = pts
            q["radius"] = np.broadcast_to(np.asarray(radius, dtype=np.float32), (pts.shape[0],))
        res = np.empty(q.shape[0], dtype=A.CLOSEST_POINT_DTYPE)
        self._check(self._lib.hala_rt_closest_points_host(self._h, C.c_void_p(q.ctypes.data), C.c_void_p(res.ctypes.data), C.c_uint32(q.shape[0])))
        return res

    def distance_grid(self, origin, spacing, dims, band=np.inf, signed=True, method=None, want_prim=False, out=None, out_prim=None, stream: int = 0,
                      d_counters: int = 0):
        """RENDER_SPEC 4.9: the scene's distance field on the grid of dims = (nx, ny, nz) cubic voxels of size `spacing` whose voxel
        (0, 0, 0) is centred at `origin`, as a float32 array [nz, ny, nx]: the closest-point distance within `band`, or `band`;
        signed=True flips the sign bit of the voxels inside (crossing parity along +x).  method: None automatic, 1 a voxel per lane, 2
        a brick per wave — the result is the same.  want_prim=True returns (distance, prim), prim a uint32 array of triangle ids
        (0xffffffff where the band answered).
        Device form: `out` is a device tensor or pointer of nx * ny * nz floats (and `out_prim` one of as many uint32, or None); the
        grid is launched on `stream` and nothing is returned.  d_counters (device, 6 x uint64): the counting variants."""
        nx, ny, nz = (int(d) for d in dims)
        desc = A.DistanceGridDesc((C.c_float * 3)(*[float(x) for x in origin]), float(spacing), (C.c_uint32 * 3)(nx, ny, nz), float(band),
                                  (A.GRID_SIGNED if signed else 0) | (int(method or 0) << A.GRID_METHOD_SHIFT))
        if out is not None:
            d_o, d_p = (self._device_out(x, nx * ny * nz * 4, "the output is too small for the grid") for x in (out, out_prim))
            if d_counters:
                self._check(self._lib.hala_rt_distance_grid_counted(self._h, C.byref(desc), C.c_void_p(d_o), C.c_void_p(d_p), C.c_void_p(d_counters),
                                                                    C.c_void_p(stream)))
            else:
                self._check(self._lib.hala_rt_distance_grid(self._h, C.byref(desc), C.c_void_p(d_o), C.c_void_p(d_p), C.c_void_p(stream)))
            return None
        shape = tuple(max(d, 0) for d in (nz, ny, nx))
        distance = np.empty(shape, dtype=np.float32)
        prim = np.empty(shape, dtype=np.uint32) if want_prim else None
        self._check(self._lib.hala_rt_distance_grid_host(self._h, C.byref(desc), C.c_void_p(distance.ctypes.data),
                                                         C.c_void_p(prim.ctypes.data) if want_prim else None))
        return (distance, prim) if want_prim else distance

    def ray_eps(self) -> np.float32:
        """RENDER_SPEC 3: sqrt(dot(ext, ext)) * 1e-5 of the committed scene's box, in float32"""
        i = self.bvh_info()
        ext = np.array(i.scene_max[:], dtype=np.float32) - np.array(i.scene_min[:], dtype=np.float32)
        sq = np.float32(ext[0] * ext[0])
        for a in (1, 2):  # dot(): fma(z, z, fma(y, y, x * x)), each fma rounded once
            sq = np.float32(np.float64(ext[a]) * np.float64(ext[a]) + np.float64(sq))
        return np.float32(np.sqrt(sq) * np.float32(1e-5))

    def occlusion(self, points, normals=None, rays=64, reach=np.inf, bias=None, seed=0, want_masks=False, out=None, out_masks=None, count=None,
                  stream: int = 0):
        """RENDER_SPEC 4.10: ambient occlusion and the bent normal at surface points.  `rays` cosine-distributed any-hit rays of length
        `reach` leave each point's hemisphere around its normal; the answer is a structured array of A.OCCLUSION_DTYPE: `visibility`, the
        share of rays nothing blocks, and `bent`, the unit mean direction of those rays (0 when all are blocked).  A sample with a
        zero or non-finite normal, point or bias answers visibility -1.  `points` and `normals` are [n, 3] arrays (`reach` and `bias`
        scalars or one per point), or `points` is an array of A.OCCLUSION_SAMPLE_DTYPE and the rest is not used.  want_masks=True returns
        (records, masks): masks[i, j >> 5] bit j & 31 is set iff ray j of sample i is occluded.
        bias: how far along the normal the rays start; None is the scene's ray_eps (1e-5 of the scene box's diagonal).  With a bias of 0
        the origin lies in the plane of the triangle it was taken from, and of its neighbours: whether their hit distance rounds to
        t > 0 or not is then decided by the last bit of the arithmetic, so a surface occludes itself in a random pattern.
        Device form: `points` is a device tensor of 32-B samples (or a device pointer, with `count`), `out` a device tensor (or pointer)
        of 16-B records and `out_masks` one of count * ceil(rays / 32) words or None (the renderer then keeps the masks to itself);
        the batch is launched on `stream` and nothing is returned."""
        words = (int(rays) + 31) // 32
        if out is not None or isinstance(points, int) or hasattr(points, "data_ptr"):
            if out is None:
                raise ValueError("the device form needs `out`")
            d_s = self._device_address(points)
            count = self._device_count(points, A.OCCLUSION_SAMPLE_DTYPE.itemsize, count)
            d_o = self._device_out(out, count * A.OCCLUSION_DTYPE.itemsize, "`out` is too small for the batch")
            d_m = self._device_out(out_masks, count * words * 4, "`out_masks` is too small for the batch")
            self._check(self._lib.hala_rt_occlusion(self._h, C.c_void_p(d_s), C.c_void_p(d_o), C.c_void_p(d_m), C.c_uint32(count), C.c_uint32(rays),
                                                    C.c_uint32(seed), C.c_void_p(stream)))
            return None
        pts = np.asarray(points)
        if pts.dtype == A.OCCLUSION_SAMPLE_DTYPE:
            q = np.ascontiguousarray(pts).reshape(-1)
        else:
            pts = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3)
            n = pts.shape[0]
            q = np.empty(n, dtype=A.OCCLUSION_SAMPLE_DTYPE)
            q["point"] = pts
            q["normal"] = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
            q["bias"] = np.broadcast_to(np.asarray(self.ray_eps() if bias is None else bias, dtype=np.float32), (n,))
            q["reach"] = np.broadcast_to(np.asarray(reach, dtype=np.float32), (n,))
        res = np.empty(q.shape[0], dtype=A.OCCLUSION_DTYPE)
        masks = np.zeros((q.shape[0], max(words, 0)), dtype=np.uint32) if want_masks else None
        self._check(self._lib.hala_rt_occlusion_host(self._h, C.c_void_p(q.ctypes.data), C.c_void_p(res.ctypes.data),
                                                     C.c_void_p(masks.ctypes.data) if want_masks else None, C.c_uint32(q.shape[0]), C.c_uint32(rays),
                                                     C.c_uint32(seed)))
        return (res, masks) if want_masks else res

    def _bake_desc(self, instance, width, height, shading_normal, flip, bias, reach, margin):
        flags = (A.BAKE_SHADING_NORMAL if shading_normal else 0) | (A.BAKE_FLIP_NORMAL if flip else 0)
        return A.BakeDesc(int(instance), int(width), int(height), flags, float(self.ray_eps() if bias is None else bias), float(reach), int(margin))

    def _bake(self, fn, args, record_dtype, width, height, out, out_texels, stream):
        """What the four bake_* methods do once their description is made.  fn: the library's device form (its host form is fn +
        "_host"); args: what both take between the handle and the outputs; record_dtype: of the first output.  Host form: (records,
        texels) shaped (height, width); device form (out is not None): launched on `stream`, nothing returned."""
        count = int(width) * int(height)
        if out is not None:
            d_o = self._device_out(out, count * record_dtype.itemsize, "`out` is too small for the map")
            d_t = self._device_out(out_texels, count * A.BAKE_TEXEL_DTYPE.itemsize, "`out_texels` is too small for the map")
            self._check(getattr(self._lib, fn)(self._h, *args, C.c_void_p(d_o), C.c_void_p(d_t), C.c_void_p(stream)))
            return None
        rec = np.empty(max(count, 0), dtype=record_dtype)
        texels = np.empty(max(count, 0), dtype=A.BAKE_TEXEL_DTYPE)
        self._check(getattr(self._lib, fn + "_host")(self._h, *args, C.c_void_p(rec.ctypes.data), C.c_void_p(texels.ctypes.data)))
        return rec.reshape(int(height), int(width)), texels.reshape(int(height), int(width))

    def bake_samples(self, instance, width, height, *, shading_normal=False, flip=False, bias=None, reach=np.inf, out=None, out_texels=None,
                     stream: int = 0):
        """RENDER_SPEC 4.11: instance `instance` (instance order) rasterised into a width x height map of its texture space.  Returns
        (samples, texels), both shaped (height, width): A.OCCLUSION_SAMPLE_DTYPE, the surface point and normal under each texel centre
        (all zero where no triangle covers it), and A.BAKE_TEXEL_DTYPE, the barycentrics and the triangle found there (prim 0xffffffff:
        none).  The normal is cross(e1, e2) of the triangle, or with shading_normal=True the interpolated vertex normal in world space;
        flip=True negates it.  bias=None is the scene's ray_eps.  Row 0 is the row of the smallest v.
        Device form: `out` is a device tensor (or pointer) of width * height 32-B samples and `out_texels` one of 16-B records or None;
        the map is launched on `stream` and nothing is returned."""
        d = self._bake_desc(instance, width, height, shading_normal, flip, bias, reach, 0)
        return self._bake("hala_rt_bake_samples", (C.byref(d),), A.OCCLUSION_SAMPLE_DTYPE, width, height, out, out_texels, stream)

    def bake_occlusion(self, instance, width, height, rays, seed=0, *, margin=0, shading_normal=False, flip=False, bias=None, reach=np.inf, out=None,
                       out_texels=None, stream: int = 0):
        """RENDER_SPEC 4.11: the ambient-occlusion map of instance `instance`: what occlusion() answers, with `rays` and `seed`, for the
        samples of bake_samples(), texel i being sample i; then every texel without a sample takes the record of the nearest texel with
        one within `margin` texels (0..16) in x and in y.  Returns (records, texels), both shaped (height, width): A.OCCLUSION_DTYPE
        (visibility -1 where nothing was baked or copied) and A.BAKE_TEXEL_DTYPE, whose `source` names the texel a record came from.
        Device form: `out` is a device tensor (or pointer) of width * height 16-B records and `out_texels` one of 16-B texel records or
        None; the bake is launched on `stream`, nothing leaves the device and nothing is returned."""
        d = self._bake_desc(instance, width, height, shading_normal, flip, bias, reach, margin)
        return self._bake("hala_rt_bake_occlusion", (C.byref(d), C.c_uint32(rays), C.c_uint32(seed)), A.OCCLUSION_DTYPE, width, height, out, out_texels, stream)

    @staticmethod
    def _bake_charts(charts):
        """the chart table of an atlas as a contiguous array of A.BAKE_CHART_DTYPE: such an array as it is, or a sequence of
        (instance, scale, offset[, shading_normal[, flip]])"""
        if isinstance(charts, np.ndarray) and charts.dtype == A.BAKE_CHART_DTYPE:
            return np.ascontiguousarray(charts).reshape(-1)
        rows = list(charts)
        table = np.zeros(len(rows), dtype=A.BAKE_CHART_DTYPE)
        for k, row in enumerate(rows):
            instance, scale, offset = row[0], row[1], row[2]
            shading_normal, flip = (row[3] if len(row) > 3 else False), (row[4] if len(row) > 4 else False)
            table[k] = (int(instance), (A.BAKE_SHADING_NORMAL if shading_normal else 0) | (A.BAKE_FLIP_NORMAL if flip else 0), tuple(scale), tuple(offset))
        return table

    def _bake_atlas_desc(self, table, width, height, bias, reach, margin):
        return A.BakeAtlasDesc(int(width), int(height), float(self.ray_eps() if bias is None else bias), float(reach), int(margin), len(table))

    def bake_atlas_samples(self, charts, width, height, *, bias=None, reach=np.inf, out=None, out_texels=None, stream: int = 0):
        """RENDER_SPEC 4.12: several instances rasterised into one width x height map.  `charts` places them: an array of
        A.BAKE_CHART_DTYPE, or a sequence of (instance, scale, offset, shading_normal, flip) with scale and offset pairs applied to the
        instance's texture coordinates (uv * scale + offset, the map being [0, 1]^2) and the normal's choice per chart.  Where charts
        overlap, the lowest global triangle id owns the texel.  Returns (samples, texels) shaped (height, width) as bake_samples() does;
        the device form is bake_samples()'s."""
        table = self._bake_charts(charts)
        d = self._bake_atlas_desc(table, width, height, bias, reach, 0)
        return self._bake("hala_rt_bake_atlas_samples", (C.byref(d), C.c_void_p(table.ctypes.data)), A.OCCLUSION_SAMPLE_DTYPE, width, height, out, out_texels,
                          stream)

    def bake_atlas_occlusion(self, charts, width, height, rays, seed=0, *, margin=0, bias=None, reach=np.inf, out=None, out_texels=None, stream: int = 0):
        """RENDER_SPEC 4.12: the ambient-occlusion atlas of the charted instances: what occlusion() answers, with `rays` and `seed`, for
        the samples of bake_atlas_samples(), texel i being sample i, then the dilation of bake_occlusion() over the whole atlas.  Only
        the texels that have a sample are traced: a texel of the gutter costs next to nothing.  Returns (records, texels) shaped
        (height, width) as bake_occlusion() does; the device form is bake_occlusion()'s."""
        table = self._bake_charts(charts)
        d = self._bake_atlas_desc(table, width, height, bias, reach, margin)
        return self._bake("hala_rt_bake_atlas_occlusion", (C.byref(d), C.c_void_p(table.ctypes.data), C.c_uint32(rays), C.c_uint32(seed)), A.OCCLUSION_DTYPE,
                          width, height, out, out_texels, stream)

    def bake_transfer(self, instance, width, height, front, back=None, targets=None, *, margin=0, shading_normal=False, flip=False, out=None,
                      out_texels=None, stream: int = 0):
        """RENDER_SPEC 4.13: every texel of instance `instance`'s width x height bake map projected onto other instances.  The ray of a
        texel starts `front` ahead of its surface point along the unit normal (the triangle's, or with shading_normal=True the
        interpolated vertex normal; flip=True negates it) and runs against the normal for front + back (back=None: front; np.inf: no
        end); it sees only the triangles of `targets`, a sequence of instance indices (None or empty: every instance but `instance`).
        Returns (records, texels) shaped (height, width): A.BAKE_TRANSFER_HIT_DTYPE — the nearest target hit (t, u, v, prim), the
        target's world-space shading normal there and height = front - t, the displacement along the normal; t = -1 where there is no
        hit — and A.BAKE_TEXEL_DTYPE as bake_occlusion() gives it, with the same dilation by `margin`.
        Device form: `out` is a device tensor (or pointer) of width * height 32-B records and `out_texels` one of 16-B texel records or
        None; the bake is launched on `stream`, nothing leaves the device and nothing is returned."""
        d = self._bake_desc(instance, width, height, shading_normal, flip, 0.0, np.inf, margin)
        table = np.ascontiguousarray([] if targets is None else list(targets), dtype=np.uint32).reshape(-1)
        t = A.BakeTransferDesc(float(front), float(front if back is None else back), 0, len(table))
        return self._bake("hala_rt_bake_transfer", (C.byref(d), C.byref(t), C.c_void_p(table.ctypes.data) if len(table) else None), A.BAKE_TRANSFER_HIT_DTYPE,
                          width, height, out, out_texels, stream)

    def bvh_info(self) -> A.BvhInfo:
        i = A.BvhInfo()
        self._check(self._lib.hala_rt_get_bvh_info(self._h, C.byref(i)))
        return i

    def download_bvh(self):
        i = self.bvh_info()
        nodes = np.empty(i.node_count * 16, dtype=np.uint32)
        tris = np.empty(max(i.stored_triangle_count, 1) * 12, dtype=np.uint32)
        self._check(self._lib.hala_rt_download_bvh(self._h, C.c_void_p(nodes.ctypes.data), C.c_void_p(tris.ctypes.data)))
        return nodes, tris[: i.stored_triangle_count * 12]

    def download_instance_refs(self):
        """two-level trees: the 64-B records the instance leaves index ([n, 16] uint32: 12 floats world -> object, root node, global id
        of the first triangle, first shading record, instance index); empty for one-level trees"""
        n = C.c_uint32(0)
        self._check(self._lib.hala_rt_download_instance_refs(self._h, None, C.c_uint32(0), C.byref(n)))
        refs = np.empty((max(n.value, 1), 16), dtype=np.uint32)
        self._check(self._lib.hala_rt_download_instance_refs(self._h, C.c_void_p(refs.ctypes.data), C.c_uint32(n.value), C.byref(n)))
        return refs[: n.value]

    def update_node_transform(self, node_index, local_transform):
        m = np.asarray(local_transform, dtype=np.float32)
        self._check(self._lib.hala_rt_update_node_transform(self._h, C.c_uint32(node_index), (C.c_float * 16)(*m.T.reshape(-1).tolist())))

    def update_vertices(self, mesh_index, primitive_index, vertices):
        """deforming geometry: new vertices (VERTEX_DTYPE records, same count) for one primitive; applied by the next refit()"""
        v = np.ascontiguousarray(vertices, dtype=A.VERTEX_DTYPE)
        self._check(self._lib.hala_rt_update_vertices(self._h, C.c_uint32(mesh_index), C.c_uint32(primitive_index), C.c_void_p(v.ctypes.data), C.c_uint32(v.shape[0])))

    def update_material(self, material_index, material):
        """replace one cpu::HalaMaterial of the scene (interactive material edits); applied by the next refit()"""
        from .scene import fill_material_desc
        d = A.MaterialDesc()
        fill_material_desc(d, material)
        self._check(self._lib.hala_rt_update_material(self._h, C.c_uint32(material_index), C.byref(d)))

    def refit(self):
        self._check(self._lib.hala_rt_refit(self._h))

    # -- node batches (docs/RENDER_SPEC.md 20; include/halart.h "Node batches") --------------------------------------------------------
    def bind_nodes(self, indices):
        """binds an ordered set of nodes of the committed scene (None or empty: unbinds); refit_nodes() then poses them from one array"""
        idx = np.ascontiguousarray([] if indices is None else indices, dtype=np.uint32).reshape(-1)
        self._check(self._lib.hala_rt_bind_nodes(self._h, idx.ctypes.data_as(C.POINTER(C.c_uint32)) if idx.size else None, C.c_uint32(idx.size)))

    def refit_nodes(self, locals):
        """update_node_transform(indices[k], locals[k]) for every bound node + refit(), with the per-node and per-instance work on the
        device where that gives the same state (node_refit_status() tells).  locals: a numpy [n, 4, 4] float32 array, row-major as
        update_node_transform takes it, or a torch float32 tensor of n x 16 elements on the renderer's device holding the column-major
        floats (produced on the stream of get_stream(), or synchronised)"""
        n = self.node_refit_status().bound_nodes
        if hasattr(locals, "data_ptr"):  # a torch tensor: device input, read in place
            import torch
            if locals.dtype != torch.float32:
                raise TypeError(f"refit_nodes: the tensor must be float32, not {locals.dtype}")
            if locals.device.type != "cuda":
                raise ValueError("refit_nodes: a tensor must live on the renderer's device (pass a numpy array for host memory)")
            mine = getattr(self, "_device_ordinal", 0)
            if locals.device.index is not None and locals.device.index != mine:
                raise ValueError(f"refit_nodes: the tensor lives on device {locals.device.index}, the renderer on device {mine}")
            if locals.numel() != n * 16 or not locals.is_contiguous():
                raise ValueError(f"refit_nodes: expected a contiguous tensor of {n} x 16 floats, got shape {tuple(locals.shape)}")
            self._check(self._lib.hala_rt_refit_nodes(self._h, C.c_void_p(locals.data_ptr()), C.c_int(1)))
            return
        m = np.asarray(locals)
        if m.dtype != np.float32:
            raise TypeError(f"refit_nodes: the array must be float32, not {m.dtype}")
        if m.shape != (n, 4, 4):
            raise ValueError(f"refit_nodes: expected shape ({n}, 4, 4) for the bound nodes, got {m.shape}")
        cols = np.ascontiguousarray(m.transpose(0, 2, 1))  # column-major, as the C ABI takes it
        self._check(self._lib.hala_rt_refit_nodes(self._h, C.c_void_p(cols.ctypes.data), C.c_int(0)))

    def node_refit_status(self) -> A.NodeRefitStatus:
        """bound_nodes, affected_nodes, affected_instances, levels; last_path (0 none, 1 device, 2 host) and last_reason
        (A.NODE_REFIT_*) of the last refit_nodes(); device_refits, host_refits"""
        s = A.NodeRefitStatus()
        self._check(self._lib.hala_rt_get_node_refit_status(self._h, C.byref(s)))
        return s

    # -- tree quality and the refit policy (docs/RENDER_SPEC.md 4.6; include/halart.h "Tree quality and the refit policy") -------------
    def set_refit_policy(self, mode, max_inflation=0.0):
        """mode: A.REFIT_POLICY_OFF (0, the default: nothing is measured), _THRESHOLD (1: measure, rebuild the trees when a refitted
        tree's cost has grown beyond max_inflation times its cost when built; finite, >= 1), _ALWAYS (2: rebuild at every refit that
        refitted a tree), _MEASURE (3: measure only).  max_inflation must be 0 unless mode is 1"""
        p = A.RefitPolicy()
        p.mode = int(mode)
        p.max_inflation = float(max_inflation)
        self._check(self._lib.hala_rt_set_refit_policy(self._h, C.byref(p)))

    def tree_quality(self):
        """-> (trees, refits_measured, trees_rebuilt_by_policy): trees is a list of A.TreeQuality (first_node, node_count, valid,
        rebuilt_last_refit, node_q_built, tri_q_built, node_q_now, tri_q_now; the sums in units of 2^-32), empty with the policy off"""
        n, measured, rebuilt = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.hala_rt_get_tree_quality(self._h, None, C.c_uint32(0), C.byref(n), C.byref(measured), C.byref(rebuilt)))
        trees = (A.TreeQuality * max(1, n.value))()
        self._check(self._lib.hala_rt_get_tree_quality(self._h, trees, C.c_uint32(n.value), C.byref(n), C.byref(measured), C.byref(rebuilt)))
        return list(trees[:n.value]), measured.value, rebuilt.value

    # -- deformers (docs/RENDER_SPEC.md 17; include/halart.h "Deformers") ---------------------------------------------------------------
    def set_deformer(self, mesh, prim, targets=None, normal_targets=None, tangent_targets=None, joints=None, weights=None, joint_count=0):
        """register morph targets ([T, V, 3] position deltas, optionally normal / tangent deltas of the same shape) and / or a skin
        (joints [V, 4] uint16 below joint_count, weights [V, 4]) on one primitive of the committed scene; its current vertices become
        the rest pose.  Uploaded once; update_deformer() then poses it"""
        fp = C.POINTER(C.c_float)

        def deltas(a):
            if a is None:
                return None, None
            a = np.ascontiguousarray(a, dtype=np.float32)
            return a, a.ctypes.data_as(fp)

        d = A.DeformerDesc()
        d.mesh_index, d.primitive_index = mesh, prim
        t, d.target_position_deltas = deltas(targets)
        nt, d.target_normal_deltas = deltas(normal_targets)
        tt, d.target_tangent_deltas = deltas(tangent_targets)
        d.target_count = 0 if t is None else t.shape[0]
        for other in (nt, tt):
            if other is not None and (t is None or other.shape != t.shape):
                raise ValueError("normal and tangent deltas have the shape of the position deltas")
        d.joint_count = joint_count
        j = w = None
        if joint_count:
            if joints is None or weights is None:
                raise ValueError("a skin (joint_count > 0) needs joints and weights, both [V, 4]")
            j = np.ascontiguousarray(joints, dtype=np.uint16)
            w = np.ascontiguousarray(weights, dtype=np.float32)
            if j.ndim != 2 or j.shape[1] != 4 or w.shape != j.shape:
                raise ValueError("joints and weights are [V, 4]")
            d.joints, d.weights = j.ctypes.data_as(C.POINTER(C.c_uint16)), w.ctypes.data_as(fp)
        n = C.c_uint32(0)
        self._check(self._lib.hala_rt_read_vertices(self._h, C.c_uint32(mesh), C.c_uint32(prim), None, C.c_uint32(0), C.byref(n)))
        for a in (t, nt, tt):
            if a is not None and (a.ndim != 3 or a.shape[1:] != (n.value, 3)):
                raise ValueError(f"morph target deltas are [T, {n.value}, 3]")
        if j is not None and j.shape[0] != n.value:
            raise ValueError(f"joints and weights are [{n.value}, 4]")
        self._check(self._lib.hala_rt_set_deformer(self._h, C.byref(d)))

    def update_deformer(self, mesh, prim, morph_weights=None, joint_matrices=None):
        """this frame's pose: morph weights [T] and / or joint matrices [J, 3, 4] (row-major, in the primitive's object space); None
        keeps that part.  Recorded on the host only; applied by the next refit()"""
        fp = C.POINTER(C.c_float)
        w = None if morph_weights is None else np.ascontiguousarray(morph_weights, dtype=np.float32).reshape(-1)
        m = None if joint_matrices is None else np.ascontiguousarray(joint_matrices, dtype=np.float32).reshape(-1, 12)
        self._check(self._lib.hala_rt_update_deformer(self._h, C.c_uint32(mesh), C.c_uint32(prim),
                                                      None if w is None else w.ctypes.data_as(fp), C.c_uint32(0 if w is None else w.shape[0]),
                                                      None if m is None else m.ctypes.data_as(fp), C.c_uint32(0 if m is None else m.shape[0])))

    def clear_deformer(self, mesh, prim):
        """remove the primitive's deformer: the rest pose is back at the next refit()"""
        self._check(self._lib.hala_rt_clear_deformer(self._h, C.c_uint32(mesh), C.c_uint32(prim)))

    def set_deformer_normals(self, mesh, prim, mode):
        """mode 1 (A.DEFORM_NORMALS_RECOMPUTED): every pose of the primitive's deformer is followed on the device by the normals from the
        posed triangles and the tangent re-orthogonalised against them; mode 0: normal and tangent as k_deform poses them.  Takes effect
        at the next refit()"""
        self._check(self._lib.hala_rt_set_deformer_normals(self._h, C.c_uint32(mesh), C.c_uint32(prim), C.c_uint32(mode)))

    def get_deformer_normals(self, mesh, prim) -> A.DeformerNormalsInfo:
        """mode, classes and list entries of the deformer's adjacency tables, and the renderer's cumulative normals launches"""
        info = A.DeformerNormalsInfo()
        self._check(self._lib.hala_rt_get_deformer_normals(self._h, C.c_uint32(mesh), C.c_uint32(prim), C.byref(info)))
        return info

    def read_vertices(self, mesh, prim) -> np.ndarray:
        """a primitive's vertices as the device holds them (VERTEX_DTYPE records): the posed mesh of a deformed primitive"""
        n = C.c_uint32(0)
        self._check(self._lib.hala_rt_read_vertices(self._h, C.c_uint32(mesh), C.c_uint32(prim), None, C.c_uint32(0), C.byref(n)))
        out = np.empty(n.value, dtype=A.VERTEX_DTYPE)
        self._check(self._lib.hala_rt_read_vertices(self._h, C.c_uint32(mesh), C.c_uint32(prim), C.c_void_p(out.ctypes.data), C.c_uint32(n.value), C.byref(n)))
        return out

    # -- shutter motion blur (docs/RENDER_SPEC.md 18; include/halart.h "Shutter") -------------------------------------------------------
    def set_shutter(self, open=0.0, close=1.0, time_stride=1):
        """frame k of an accumulation renders the keyed holders at the time of step k // time_stride, a stratified sequence over
        [open, close); set_shutter(None) turns the shutter off.  Applied by the next refit()"""
        if open is None:
            self._check(self._lib.hala_rt_set_shutter(self._h, None))
            return
        p = A.ShutterParams()
        self._lib.hala_shutter_default_params(C.byref(p))
        p.shutter_open, p.shutter_close, p.time_stride = open, close, time_stride
        self._check(self._lib.hala_rt_set_shutter(self._h, C.byref(p)))

    def shutter_status(self) -> A.ShutterStatus:
        """enabled, time_stride, step (0xFFFFFFFF: none), time, steps: as the last refit() and the updates since left them"""
        s = A.ShutterStatus()
        self._check(self._lib.hala_rt_get_shutter_status(self._h, C.byref(s)))
        return s

    def set_node_keys(self, node_index, open=None, close=None):
        """the node's local transform ([4, 4], as update_node_transform takes it) at time 0 and at time 1; both None clears the keys.
        Applied by the next refit()"""
        def arg(m):
            return None if m is None else (C.c_float * 16)(*np.asarray(m, dtype=np.float32).T.reshape(-1).tolist())
        self._check(self._lib.hala_rt_set_node_keys(self._h, C.c_uint32(node_index), arg(open), arg(close)))

    def set_deformer_keys(self, mesh, prim, open=None, close=None):
        """the deformer's pose at time 0 and at time 1, each a dict(morph_weights=..., joint_matrices=...) as update_deformer takes
        them (a part that is None in one pose must be None in the other); both None clears the keys.  Applied by the next refit()"""
        fp = C.POINTER(C.c_float)

        def part(pose, key, cols):
            a = None if pose is None else pose.get(key)
            return None if a is None else np.ascontiguousarray(a, dtype=np.float32).reshape(-1, cols)

        wo, wc = part(open, "morph_weights", 1), part(close, "morph_weights", 1)
        mo, mc = part(open, "joint_matrices", 12), part(close, "joint_matrices", 12)
        ptr = lambda a: None if a is None else a.ctypes.data_as(fp)  # noqa: E731
        count = lambda a, b: next((x.shape[0] for x in (a, b) if x is not None), 0)  # noqa: E731
        if (wo is not None and wc is not None and wo.shape != wc.shape) or (mo is not None and mc is not None and mo.shape != mc.shape):
            raise ValueError("the two poses have the same number of weights and of joint matrices")
        self._check(self._lib.hala_rt_set_deformer_keys(self._h, C.c_uint32(mesh), C.c_uint32(prim), ptr(wo), ptr(wc), C.c_uint32(count(wo, wc)),
                                                        ptr(mo), ptr(mc), C.c_uint32(count(mo, mc))))

    def set_vertex_keys(self, mesh, prim, open=None, close=None):
        """the primitive's vertices (VERTEX_DTYPE records, the primitive's count) at time 0 and at time 1; both None clears the keys.
        Both stay on the device.  Applied by the next refit()"""
        o = None if open is None else np.ascontiguousarray(open, dtype=A.VERTEX_DTYPE)
        c = None if close is None else np.ascontiguousarray(close, dtype=A.VERTEX_DTYPE)
        if o is not None and c is not None and o.shape != c.shape:
            raise ValueError("the two keys have the same number of vertices")
        n = next((x.shape[0] for x in (o, c) if x is not None), 0)
        self._check(self._lib.hala_rt_set_vertex_keys(self._h, C.c_uint32(mesh), C.c_uint32(prim), None if o is None else C.c_void_p(o.ctypes.data),
                                                      None if c is None else C.c_void_p(c.ctypes.data), C.c_uint32(n)))

    # -- rigs and clips (docs/RENDER_SPEC.md 19; include/halart.h "Rigs and clips") -----------------------------------------------------
    def set_rig(self, rig):
        """register one deformer per binding of a rig.Rig (NativeScene.rig) on the committed scene; None clears the rig and its deformers"""
        self._check(self._lib.hala_rt_set_rig(self._h, None if rig is None else rig.desc_ptr()))
        self._rig = rig

    def pose_rig(self, clip, time=0.0):
        """record clip `clip` (None: the file's own pose) at `time`: node transforms and deformer poses, applied by the next refit()"""
        from .rig import clip_index
        self._check(self._lib.hala_rt_pose_rig(self._h, C.c_uint32(clip_index(clip)), C.c_float(time)))

    def key_rig(self, clip, t_open=0.0, t_close=0.0):
        """the clip's poses at t_open and t_close as shutter keys of its nodes and deformers (None clears them); applied by the next refit()"""
        from .rig import clip_index
        self._check(self._lib.hala_rt_key_rig(self._h, C.c_uint32(clip_index(clip)), C.c_float(t_open), C.c_float(t_close)))

    def rig_pose(self, key=0):
        """what the last pose_rig (key 0) or key_rig (0: open, 1: close) recorded -> Rig.unpack()'s dict plus clip (None: the file's pose) and time"""
        rig = getattr(self, "_rig", None)
        if rig is None:
            from . import HalaRendererError
            raise HalaRendererError("No rig is set (set_rig).")
        fp = C.POINTER(C.c_float)
        l, w, p = rig.buffers()
        clip, time = C.c_uint32(0), C.c_float(0.0)
        self._check(self._lib.hala_rt_get_rig_pose(self._h, C.c_uint32(key), C.byref(clip), C.byref(time), l.ctypes.data_as(fp), w.ctypes.data_as(fp),
                                                   p.ctypes.data_as(fp)))
        out = rig.unpack(l, w, p)
        out["clip"], out["time"] = (None if clip.value == 0xFFFFFFFF else clip.value), time.value
        return out

    def rig_status(self) -> A.RigStatus:
        """bindings of the rig, deformers registered, and the cumulative pose launches, those among them that posed two or more deformers, and the
        deformers ("segments") they posed"""
        s = A.RigStatus()
        self._check(self._lib.hala_rt_get_rig_status(self._h, C.byref(s)))
        return s

    # -- multi-GPU tile sharding ---------------------------------------------------------------------------------------
    def set_tile_shard(self, rank, world, tile_size=32):
        self._check(self._lib.hala_rt_set_tile_shard(self._h, C.c_uint32(rank), C.c_uint32(world), C.c_uint32(tile_size)))

    def stream_handle(self):
        """the renderer's hipStream_t as an integer (torch.cuda.ExternalStream(handle) wraps it)"""
        p = C.c_void_p()
        self._check(self._lib.hala_rt_get_stream(self._h, C.byref(p)))
        return p.value or 0

    def get_stream(self):
        """hala_rt_get_stream: the same handle under the C entry point's name (device arrays for refit_nodes are produced on it)"""
        return self.stream_handle()

    def tile_buffer(self, which=0):
        p = C.c_void_p(); n = C.c_size_t()
        self._check(self._lib.hala_rt_tile_buffer(self._h, C.c_int(which), C.byref(p), C.byref(n)))
        return p.value, n.value

    # -- the exchange step inside the library (RCCL; include/halart.h "hala_rt_comm_*", "hala_rt_tile_allgather*") --------------
    @staticmethod
    def comm_unique_id() -> bytes:
        """ncclGetUniqueId: made on rank 0, handed to the other ranks over any host channel"""
        from . import check, load_library
        buf = (C.c_uint8 * 128)()
        check(load_library().hala_rt_comm_unique_id(buf))
        return bytes(buf)

    def comm_init_rank(self, unique_id: bytes, rank: int, world: int):
        self._check(self._lib.hala_rt_comm_init_rank(self._h, (C.c_uint8 * 128)(*unique_id), C.c_uint32(rank), C.c_uint32(world)))

    def comm_attach(self, nccl_comm: int):
        self._check(self._lib.hala_rt_comm_attach(self._h, C.c_void_p(nccl_comm)))

    def comm_destroy(self):
        self._check(self._lib.hala_rt_comm_destroy(self._h))

    def tile_allgather(self, aovs=(0,)):
        self._check(self._lib.hala_rt_tile_allgather(self._h, C.c_uint32(sum(1 << a for a in aovs))))

    def tile_allgather_begin(self, aovs=(0,)):
        self._check(self._lib.hala_rt_tile_allgather_begin(self._h, C.c_uint32(sum(1 << a for a in aovs))))

    def tile_allgather_finish(self):
        self._check(self._lib.hala_rt_tile_allgather_finish(self._h))

    def tile_allgather_begin_external(self, aovs=(0,)):
        """the pipeline of tile_allgather_begin with the exchange left to the caller (exchange_buffers); no communicator needed"""
        self._check(self._lib.hala_rt_tile_allgather_begin_external(self._h, C.c_uint32(sum(1 << a for a in aovs))))

    def exchange_buffers(self, which=0):
        """-> (staged ptr, staged bytes, receive ptr, receive bytes, exchange hipStream_t) of the exchange in flight"""
        a = C.c_void_p(); na = C.c_size_t(); b = C.c_void_p(); nb = C.c_size_t(); st = C.c_void_p()
        self._check(self._lib.hala_rt_get_exchange_buffers(self._h, C.c_int(which), C.byref(a), C.byref(na), C.byref(b), C.byref(nb), C.byref(st)))
        return a.value, na.value, b.value, nb.value, st.value

    def gathered_buffer(self, which=0):
        p = C.c_void_p(); n = C.c_size_t()
        self._check(self._lib.hala_rt_get_gathered_buffer(self._h, C.c_int(which), C.byref(p), C.byref(n)))
        return p.value, n.value

    def scatter_gathered_tiles(self, which, d_gathered: int, nbytes: int, stream: int = 0):
        """de-interleave a gathered buffer into this renderer's row-major image; stream = a hipStream_t of the caller's (0: the renderer's)"""
        self._check(self._lib.hala_rt_scatter_gathered_tiles_on_stream(self._h, C.c_int(which), C.c_void_p(d_gathered), C.c_size_t(nbytes), C.c_void_p(stream or None)))


def denoise_default_params(**overrides) -> A.DenoiseParams:
    """hala_denoise_default_params with the fields given (not None) replaced"""
    from . import load_library
    p = A.DenoiseParams()
    load_library().hala_denoise_default_params(C.byref(p))
    for k, v in overrides.items():
        if v is not None:
            setattr(p, k, int(bool(v)) if k == "demodulate" else v)
    return p


def adaptive_default_params(**overrides) -> A.AdaptiveParams:
    """hala_adaptive_default_params with the fields given (not None) replaced"""
    from . import load_library
    p = A.AdaptiveParams()
    load_library().hala_adaptive_default_params(C.byref(p))
    for k, v in overrides.items():
        if v is not None:
            setattr(p, k, v)
    return p


def temporal_default_params(**overrides) -> A.TemporalParams:
    """hala_temporal_default_params with the fields given (not None) replaced"""
    from . import load_library
    p = A.TemporalParams()
    load_library().hala_temporal_default_params(C.byref(p))
    for k, v in overrides.items():
        if v is not None:
            setattr(p, k, v)
    return p


def temporal_clamp_default_params(**overrides) -> A.TemporalClampParams:
    """hala_temporal_clamp_default_params with the fields given (not None) replaced"""
    from . import load_library
    p = A.TemporalClampParams()
    load_library().hala_temporal_clamp_default_params(C.byref(p))
    for k, v in overrides.items():
        if v is not None:
            setattr(p, k, v)
    return p


def variant_ledger(family, reset=False):
    """hala_rt_variant_ledger -> (launched, built): bit masks over the flag combinations of kernel family `family` (_abi.VARIANT_FAMILIES:
    the first flag is bit 0 of a combination's index); per process; reset clears `launched` after reading.  Needs no GPU."""
    from . import check, load_library
    launched, built = C.c_uint64(0), C.c_uint64(0)
    check(load_library().hala_rt_variant_ledger(C.c_uint32(family), C.byref(launched), C.byref(built), C.c_int(bool(reset))))
    return launched.value, built.value


SELFTEST_RCP, SELFTEST_SQRT = 0, 1


def selftest_math(which, first, count):
    """hala_rt_selftest_math -> (mismatches, first_bad): the exact-math helper `which` (SELFTEST_RCP: rcp_rn against 1.0f / x, SELFTEST_SQRT:
    sqrt_rn against sqrtf) on the `count` consecutive binary32 bit patterns from `first`; first_bad is None when nothing differs."""
    from . import check, load_library
    bad, low = C.c_uint64(0), C.c_uint32(0)
    check(load_library().hala_rt_selftest_math(C.c_int(which), C.c_uint32(first), C.c_uint64(count), C.byref(bad), C.byref(low)))
    return bad.value, (low.value if bad.value else None)


def selftest_math_values(which, patterns):
    """hala_rt_selftest_math_values -> (helper_bits, reference_bits, mismatches): what the helper and the plain IEEE expression give, as
    uint32 bit patterns, for each of the uint32 bit patterns in `patterns`."""
    from . import check, load_library
    p = np.ascontiguousarray(patterns, dtype=np.uint32)
    helper, ref = np.empty_like(p), np.empty_like(p)
    bad = C.c_uint64(0)
    check(load_library().hala_rt_selftest_math_values(C.c_int(which), C.c_void_p(p.ctypes.data), C.c_uint32(p.size), C.c_void_p(helper.ctypes.data),
                                                      C.c_void_p(ref.ctypes.data), C.byref(bad), None))
    return helper, ref, bad.value


def selftest_collapse(left, right, node_parent, leaf_parent, first, last, node_boxes, leaf_boxes, leaf_max):
    """hala_rt_selftest_collapse: the collapse of a build (cost pass, then the level launches) on a binary tree from host arrays — child
    references with bit 31 for a leaf, parents (0xffffffff: the root, node 0), sorted positions first .. last per node, boxes [.., 6].
    -> dict(costs [n - 1, 3] float32 = C(node, 1 .. 3), choices [n - 1], keep [n - 1], refs4 [node_count, 4], levels)."""
    from . import check, load_library
    u32 = lambda x: np.ascontiguousarray(x, dtype=np.uint32)  # noqa: E731
    left, right, node_parent, leaf_parent, first, last = (u32(x) for x in (left, right, node_parent, leaf_parent, first, last))
    node_boxes, leaf_boxes = (np.ascontiguousarray(x, dtype=np.float32).reshape(-1, 6) for x in (node_boxes, leaf_boxes))
    n = leaf_parent.size
    if n < 2 or any(x.size != n - 1 for x in (left, right, node_parent, first, last)) or len(node_boxes) != n - 1 or len(leaf_boxes) != n:
        raise ValueError("a tree of n leaves has n - 1 inner nodes")
    costs = np.zeros((n - 1, 3), dtype=np.float32)
    choices, keep = np.zeros(n - 1, dtype=np.uint32), np.zeros(n - 1, dtype=np.uint32)
    refs4 = np.zeros((n - 1, 4), dtype=np.uint32)
    count, levels = C.c_uint32(0), C.c_uint32(0)
    ptr = lambda x: C.c_void_p(x.ctypes.data)  # noqa: E731
    check(load_library().hala_rt_selftest_collapse(C.c_uint32(n), C.c_uint32(leaf_max), ptr(left), ptr(right), ptr(node_parent), ptr(leaf_parent),
                                                   ptr(first), ptr(last), ptr(node_boxes), ptr(leaf_boxes), ptr(costs), ptr(choices), ptr(keep),
                                                   ptr(refs4), C.byref(count), C.byref(levels)))
    return dict(costs=costs, choices=choices, keep=keep, refs4=refs4[:count.value].copy(), levels=levels.value)


def selftest_hierarchy(boxes, pad, builder, ploc_tail=0, ploc_look_every=0):
    """hala_rt_selftest_hierarchy: the binary tree that builder 1 (SAH), 2 (PLOC) or 3 (LBVH) of a build makes over boxes [n, 6] (min xyz,
    max xyz by id), fitted boxes widened by pad.  -> dict(sorted_ids [n], left, right, first, last, node_parent [n - 1], leaf_parent [n],
    node_boxes [n - 1, 6]): the arrays selftest_collapse takes, with sorted_ids before them."""
    from . import check, load_library
    boxes = np.ascontiguousarray(boxes, dtype=np.float32)
    if boxes.ndim != 2 or boxes.shape[1] != 6:
        raise ValueError("expected boxes of shape [n, 6]")
    n = len(boxes)
    ni = max(n - 1, 1)
    out = {k: np.zeros(ni, dtype=np.uint32) for k in ("left", "right", "first", "last", "node_parent")}
    out["sorted_ids"], out["leaf_parent"] = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32)
    out["node_boxes"] = np.zeros((ni, 6), dtype=np.float32)
    ptr = lambda x: C.c_void_p(x.ctypes.data)  # noqa: E731
    check(load_library().hala_rt_selftest_hierarchy(C.c_uint32(n), ptr(boxes), C.c_float(pad), C.c_uint32(builder), C.c_uint32(ploc_tail),
                                                    C.c_uint32(ploc_look_every), *(ptr(out[k]) for k in ("sorted_ids", "left", "right", "first", "last",
                                                                                                         "node_parent", "leaf_parent", "node_boxes"))))
    return out


def denoise_images(color, albedo, normal, device_ordinal=0, **params) -> np.ndarray:
    """hala_denoise_images: the RENDER_SPEC 10 filter on host images [H, W, 3 or 4] (e.g. the PFM trio of save_images); returns the
    denoised RGBA32F [H, W, 4].  params: iterations, sigma_color, sigma_albedo, normal_power, demodulate."""
    from . import check, load_library

    def rgba(x):
        x = np.asarray(x, dtype=np.float32)
        if x.ndim != 3 or x.shape[2] not in (3, 4):
            raise ValueError("expected an image of shape [H, W, 3] or [H, W, 4]")
        if x.shape[2] == 3:
            x = np.concatenate([x, np.ones(x.shape[:2] + (1,), np.float32)], axis=2)
        return np.ascontiguousarray(x)

    c, a, n = rgba(color), rgba(albedo), rgba(normal)
    if not (c.shape == a.shape == n.shape):
        raise ValueError("color, albedo and normal must have the same size")
    h, w = c.shape[:2]
    p = denoise_default_params(**params)
    out = np.empty((h, w, 4), dtype=np.float32)
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    check(load_library().hala_denoise_images(device_ordinal, fp(c), fp(a), fp(n), w, h, C.byref(p), fp(out)))
    return out


def cryptomatte_matte(ids, coverage, manifest, names) -> np.ndarray:
    """[H, W] float32: what a compositor's keyer does with read_cryptomatte's (ids, coverage) — the coverage of the ranks whose id is one
    of `names` (looked up in `manifest`), summed in rank order"""
    missing = [n for n in names if n not in manifest]
    if missing:
        raise ValueError(f"cryptomatte_matte: no name {missing} in the manifest")
    want = np.array([int(manifest[n], 16) for n in names], dtype=np.uint32)
    bits = np.ascontiguousarray(ids, dtype=np.float32).view(np.uint32)
    cov = np.asarray(coverage, dtype=np.float32)
    sel = np.isin(bits, want) & (cov > 0)
    acc = np.zeros(bits.shape[:-1], np.float32)
    for r in range(bits.shape[-1]):
        acc = (acc + np.where(sel[..., r], cov[..., r], np.float32(0.0))).astype(np.float32)
    return acc


def view_depth(position, camera):
    """[H, W] float32 view-space depth along the camera's forward axis from a position AOV (read_image("position")) and a packed camera
    (HalaRenderer.packed_cameras()[c]): dot(xyz / w - camera position, normalize(forward)) where w > 0, +inf where no sample hit.  Computed in
    float64 and rounded once.  Depth is linear in P, so it is also the mean depth of the samples that hit."""
    p = np.asarray(position, dtype=np.float64)
    w = p[..., 3]
    fwd = np.array(camera.forward[:3], dtype=np.float64)
    fwd = fwd / np.linalg.norm(fwd)
    eye = np.array(camera.position[:3], dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        depth = (p[..., :3] @ fwd - w * float(eye @ fwd)) / w
    return np.where(w > 0.0, depth, np.inf).astype(np.float32)
