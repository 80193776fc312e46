"""The finished first-hit images — albedo, normal, position, ids and the first vertex's radiance (max_depth 1) — against the float64
numpy reference of tests/first_hit_ref.py, which is written from docs/RENDER_SPEC.md and the scene description alone.

Two tiers over the same cases and the same assertions: the CPU tier holds the oracle to the reference, the GPU tier the product.
Pixels whose discrete decisions are within 1e-4 of flipping (first_hit_ref: `fragile`) are left out; a case may set aside at most 2 % of
its pixels.  ids and coverage must be equal; the float quantities must agree within 8 m, where m is how far the reference itself moves
when every array is float32 instead of float64 (never below 16 * 2^-24 of the quantity's scale).  No tolerance is derived from the
oracle or the product.  Each comparison prints its figures (`-s` shows them; DESIGN.md "First-hit reference" records a run)."""
import functools
import math

import numpy as np
import pytest

import aov_ref
import first_hit_ref as R
import hala_renderer_amd as H
from hala_renderer_amd import _abi as A
from hala_renderer_amd import scenes
from hala_renderer_amd.scene import HalaMedium

gpu = pytest.mark.gpu
f32, f64 = np.float32, np.float64
W, HT = 48, 40
FRAGILE_CAP = 0.02
QUANTITIES = ("position", "normal", "albedo", "radiance")


class Case:
    def __init__(self, scene, w=W, h=HT, frames=1, camera=0, settings=None, build=None, instancing=False, simple=None, check=None):
        self.scene, self.w, self.h, self.frames, self.camera = scene, w, h, frames, camera
        self.settings = settings or R.Settings()
        self.build, self.instancing, self.simple, self.check = build or {}, instancing, simple, check


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------
def add_image(s, fmt, w, h, data):
    k = len(s.image_data)
    s.image_data.append(H.HalaImageData(fmt, w, h, data)); s.image2data_mapping[k] = k; s.texture2image_mapping[k] = k
    return k


def textured_bunny():
    """Disney blob with sRGB base, UNORM normal (and metallic-roughness) maps of 64 x 64; the ground takes a BGRA-tag base map of 33 x 17 and
    a float emission map of 16 x 8.  No light, SKY environment: every surface pixel's radiance is its emission."""
    s = scenes.bunny_class(subdivisions=3, aspect=W / HT, disney=True)
    scenes.attach_textures(s, sets=1, size=64)
    rng = np.random.RandomState(9)
    em = add_image(s, scenes.A_FORMAT_FLOAT, 16, 8, (rng.rand(8, 16, 4) * 2).astype(f32))
    px = (rng.rand(17, 33, 4) * 255).astype(np.uint8); px[..., 3] = 255
    bg = add_image(s, scenes.A_FORMAT_BGRA_TAG, 33, 17, px)
    s.materials[1].base_color_map_index = bg
    s.materials[1].emission = (0.4, 0.5, 0.6); s.materials[1].emission_map_index = em
    s.materials[0].emission = (0.05, 0.02, 0.01)
    return s


def grazing_plane():
    """a ground plane whose texture repeats 12 times, seen from 0.35 above it towards the horizon: near pixels magnify the maps, far ones
    reach the cosine clamp and the last levels.  sRGB base map (8-bit mip rule) and a float emission map."""
    s = H.HalaScene()
    s.materials = [H.HalaMaterial(type=0, base_color=(0.9, 0.8, 0.7), roughness=0.3, emission=(0.5, 0.25, 1.0))]
    pos = [(-20, 0, 2), (20, 0, 2), (20, 0, -38), (-20, 0, -38)]
    prim = H.HalaPrimitive(indices=np.array([0, 1, 2, 0, 2, 3], np.uint32),
                           vertices=scenes._vertices(pos, [(0, 1, 0)] * 4, [(0, 0), (12, 0), (12, 12), (0, 12)]), material_index=0)
    s.meshes = [H.HalaMesh([prim])]
    s.nodes = [H.HalaNode(name="ground", mesh_index=0),
               H.HalaNode(name="camera", camera_index=0, local_transform=scenes.look_at_node_transform((0.3, 0.35, 0.0), (0.0, 0.1, -10.0)))]
    s.cameras = [H.HalaPerspectiveCamera(aspect=W / HT, yfov=math.radians(40.0), znear=0.1)]
    base, _, _ = scenes.procedural_texture_set(64, 3)
    rng = np.random.RandomState(4)
    s.materials[0].base_color_map_index = add_image(s, base.format, base.width, base.height, base.data)
    s.materials[0].emission_map_index = add_image(s, scenes.A_FORMAT_FLOAT, 32, 16, (rng.rand(16, 32, 4) * 3).astype(f32))
    return s


def hierarchy(media=False):
    """one blob primitive referenced by two nodes — one of them mirrored and sheared (det < 0) — at the end of a parent chain of depth 3,
    and a second mesh hanging off the chain's first node.  media: the blobs bound an EMISSIVE medium, which only a ray that arrives from
    behind has crossed (RENDER_SPEC 7.1e) — none does, unless the mirrored node's normals are left pointing inwards —, and a wall behind
    them, seen from its back, emits through an ABSORB medium."""
    s = H.HalaScene()
    s.materials = [H.HalaMaterial(type=0, base_color=(0.8, 0.3, 0.2), roughness=0.2), H.HalaMaterial(type=0, base_color=(0.2, 0.5, 0.7), roughness=0.2)]
    blob = scenes.blob_mesh(2, seed=7); blob.material_index = 0
    plate = scenes._merge_quads([((-3, -1.6, 2), (3, -1.6, 2), (3, -1.2, -2), (-3, -1.2, -2))]); plate.material_index = 1
    s.meshes = [H.HalaMesh([blob]), H.HalaMesh([plate])]
    if media:
        s.materials[0].medium = HalaMedium(type=3, color=(0.3, 0.6, 0.9), density=0.5)
        s.materials.append(H.HalaMaterial(type=0, base_color=(0.6, 0.6, 0.6), roughness=0.2, emission=(1.0, 0.8, 0.6),
                                          medium=HalaMedium(type=1, color=(0.2, 0.5, 0.8), density=0.3)))
        wall = scenes._merge_quads([((-4, -1.5, -3), (-4, 3, -3), (4, 3, -3), (4, -1.5, -3))]); wall.material_index = 2  # faces -z
        s.meshes[1].primitives.append(wall)

    def xf(m3, t):
        m = np.eye(4, dtype=f32); m[:3, :3] = m3; m[:3, 3] = t
        return m
    c, sn = math.cos(0.3), math.sin(0.3)
    s.nodes = [
        H.HalaNode(name="root", local_transform=xf([[c, 0, sn], [0, 1, 0], [-sn, 0, c]], (0.2, 0.1, -0.3))),
        H.HalaNode(name="mid", parent=0, local_transform=xf(np.diag([0.9, 1.1, 0.8]), (0.0, 0.2, 0.0))),
        H.HalaNode(name="plain", parent=1, mesh_index=0, local_transform=xf(np.eye(3), (-1.5, 0.0, 0.0))),
        H.HalaNode(name="mirrored", parent=1, mesh_index=0, local_transform=xf([[-1.3, .2, 0], [.1, .7, .3], [0, -.2, 1.1]], (1.5, 0.1, 0.0))),
        H.HalaNode(name="plate", parent=0, mesh_index=1),
        H.HalaNode(name="camera", camera_index=0, local_transform=scenes.look_at_node_transform((0.3, 1.0, 6.0), (0.0, 0.0, 0.0))),
    ]
    s.cameras = [H.HalaPerspectiveCamera(aspect=W / HT, yfov=math.radians(40.0), znear=0.1)]
    return s


def sphere_lights():
    """Cornell box with two SPHERE lights: one in front of the back wall above the short block, one half hidden behind the tall block"""
    s = scenes.cornell_box(aspect=W / HT, analytic_light=False)
    for k, (pos, radius) in enumerate([((186.0, 230.0, 150.0), 35.0), ((368.0, 200.0, 480.0), 60.0)]):
        m = np.eye(4, dtype=f32); m[:3, 3] = pos
        s.nodes.append(H.HalaNode(name=f"sphere_{k}", light_index=k, local_transform=m))
        s.lights.append(H.HalaLight(color=(1.0, 0.5 + 0.25 * k, 0.25), intensity=9.0 + 4.0 * k, light_type=H.HalaLightType.SPHERE, params=(radius, 0.0)))
    return s


def quad_light_seen_from_behind():
    """Cornell box with a second QUAD light in the middle of the room that faces away from the camera: rays pass through its back"""
    s = scenes.cornell_box(aspect=W / HT)
    m = np.eye(4, dtype=f32); m[:3, 3] = (278.0, 273.0, 200.0)  # u = x, v = y: n = +z, the camera stands at z = -800
    s.nodes.append(H.HalaNode(name="turned_away", light_index=1, local_transform=m))
    s.lights.append(H.HalaLight(color=(0.2, 1.0, 0.4), intensity=5.0, light_type=H.HalaLightType.QUAD, params=(150.0, 120.0)))
    return s


def random_env():
    return (np.random.RandomState(11).rand(8, 16, 4) * 2).astype(f32)


def lod_spans_levels(case, ref):
    lod = ref.lod[~ref.fragile & np.isfinite(ref.lod)]
    assert lod.min() < 1.0 and lod.max() >= 3.0, (lod.min(), lod.max())


def sees(*kinds):
    def check(case, ref):
        for k in kinds:
            assert np.any(ref.kinds == k), k
    return check


def only_the_ceiling_light(case, ref):
    lit = ref.ids[..., 3][(ref.ids[..., 3] != 0xFFFFFFFF) & (ref.ids[..., 3] >= 0x80000000)]
    assert lit.size and np.all(lit == 0x80000000)


def sees_the_wall_from_behind(case, ref):
    wall = ref.ids[..., 2] == 2
    assert wall.sum() > 100 and np.all(ref.radiance[wall & ~ref.fragile] > 0)
    assert np.all(ref.radiance[(ref.ids[..., 2] == 0) & ~ref.fragile] == 0)  # no blob pixel is entered from behind


def sees_two_instances_and_the_mirror(case, ref):
    tri = ref.ids[..., 3] < 0x80000000
    assert {2, 3} <= set(np.unique(ref.ids[..., 0][tri]).tolist())  # both nodes of the shared primitive
    assert len(np.unique(ref.ids[..., 1][tri])) >= 3


CASES = {
    "cornell-1": lambda: Case(scenes.cornell_box(aspect=W / HT), frames=1, simple=True, check=sees(R.LIGHT, R.SURFACE)),
    "cornell-3": lambda: Case(scenes.cornell_box(aspect=W / HT), frames=3, simple=True, check=sees(R.LIGHT, R.SURFACE)),
    "cornell-50x37": lambda: Case(scenes.cornell_box(aspect=50 / 37), w=50, h=37, frames=2, simple=True),
    "bunny-textured-bundles": lambda: Case(textured_bunny(), frames=2, simple=False, build=dict(texture_bundles=True)),
    "bunny-textured-per-map": lambda: Case(textured_bunny(), frames=2, simple=False, build=dict(texture_bundles=False)),
    "grazing-plane": lambda: Case(grazing_plane(), frames=1, check=lod_spans_levels),
    "hierarchy-flattened": lambda: Case(hierarchy(), frames=2, build=dict(instancing=False), check=sees_two_instances_and_the_mirror),
    "hierarchy-instanced": lambda: Case(hierarchy(), frames=2, build=dict(instancing=True), instancing=True, check=sees_two_instances_and_the_mirror),
    # the sign of det in the normal transform cancels in the normal image (ns is flipped to face the ray either way); it decides which
    # side a ray arrives from, which a medium makes visible in image 0
    "mirrored-medium": lambda: Case(hierarchy(media=True), frames=1, build=dict(instancing=False), check=sees_the_wall_from_behind),
    "mirrored-medium-instanced": lambda: Case(hierarchy(media=True), frames=1, build=dict(instancing=True), instancing=True, check=sees_the_wall_from_behind),
    "quad-light-from-behind": lambda: Case(quad_light_seen_from_behind(), frames=1, check=only_the_ceiling_light),
    "thin-lens-view": lambda: Case(scenes.with_extra_cameras(scenes.cornell_box(aspect=W / HT), 2), frames=2, camera=1),
    "orthographic-view": lambda: Case(scenes.with_extra_cameras(scenes.cornell_box(aspect=W / HT), 2), frames=2, camera=2),
    "sphere-lights": lambda: Case(sphere_lights(), frames=2, check=sees(R.LIGHT, R.SURFACE)),
    "miss-sky": lambda: Case(scenes.bunny_class(subdivisions=1, aspect=W / HT), frames=2, check=sees(R.MISS),
                             settings=R.Settings(env_intensity=1.7, ground=(0.9, 0.4, 0.1), sky=(0.1, 0.3, 0.8))),
    "miss-envmap": lambda: Case(scenes.bunny_class(subdivisions=1, aspect=W / HT), frames=2, check=sees(R.MISS),
                                settings=R.Settings(env=scenes.sky_sun_envmap(64, 32), env_rotation=40.0, env_intensity=1.7)),
    # every texel of this map differs from its neighbours, so a lookup that is off in u or v shows at every miss pixel (the sky map above
    # varies with u only inside its sun disc)
    "miss-random-envmap": lambda: Case(scenes.bunny_class(subdivisions=1, aspect=W / HT), frames=1, check=sees(R.MISS),
                                       settings=R.Settings(env=random_env(), env_rotation=40.0, env_intensity=1.7)),
}


@functools.lru_cache(maxsize=None)
def prepared(name):
    """the case, its float64 reference, the float32 run of the same code, and the tolerances that follow from the two"""
    case = CASES[name]()
    ref = R.render(case.scene, case.w, case.h, case.frames, case.settings, case.camera, f64)
    low = R.render(case.scene, case.w, case.h, case.frames, case.settings, case.camera, f32)
    share = float(ref.fragile.mean())
    ok = ~ref.fragile
    # image 0 is compared only where no next-event term can exist: misses, light hits, and every pixel of a scene without lights under SKY
    if case.scene.lights or case.settings.env is not None:
        radiance_ok = ok & np.all(ref.kinds != R.SURFACE, axis=0)
    else:
        radiance_ok = ok
    masks = dict(position=ok, normal=ok, albedo=ok, radiance=radiance_ok)
    scale = dict(position=ref.extent, normal=1.0, albedo=1.0, radiance=radiance_scale(case, ref.extent))
    assert np.array_equal(low.ids[ok], ref.ids[ok]), "float32 rounding alone changes a hit that is not marked fragile"
    tol, m = {}, {}
    for q in QUANTITIES:
        a, b = getattr(ref, q)[..., :3][masks[q]], getattr(low, q)[..., :3][masks[q]].astype(f64)
        m[q] = float(np.abs(a - b).max()) if a.size else 0.0
        tol[q] = max(8.0 * m[q], 16.0 * 2.0 ** -24 * scale[q])
    return case, ref, masks, m, tol, share


def radiance_scale(case, extent):
    """the largest texel / intensity that can reach image 0 at the first vertex (an EMISSIVE medium: over a path as long as the scene)"""
    st, s = case.settings, case.scene
    k = abs(st.env_intensity)
    out = [k * float(st.env.max())] if st.env is not None else [k * max(st.ground), k * max(st.sky)]
    out += [float(max(l.color)) * l.intensity for l in s.lights]
    for mat in s.materials:
        img = R.texture_of(s, mat.emission_map_index)
        out.append(max(mat.emission) * (1.0 if img is None else float(R.decode_level0(img, R.srgb_lut())[..., :3].max())))
        if mat.medium.type == 3:
            out.append(max(mat.medium.color) * mat.medium.density * extent)
    return max(out)


def compare(name, tier, got):
    """got: albedo, normal, radiance, position [h, w, 4] float32 and ids [h, w, 4] uint32 of the implementation under test"""
    case, ref, masks, m, tol, share = prepared(name)
    print(f"\nFIRSTHIT {tier} {name} fragile {100 * share:.3f}% of {ref.fragile.size}")
    assert share <= FRAGILE_CAP, f"{name}: {100 * share:.2f} % of the pixels are fragile"
    if case.check:
        case.check(case, ref)
    ok = masks["position"]
    failures = []
    if not np.array_equal(got["ids"][ok], ref.ids[ok]):
        failures.append(f"ids differ on {int(np.any(got['ids'][ok] != ref.ids[ok], axis=-1).sum())} pixels")
    if not np.array_equal(got["position"][..., 3][ok], ref.position[..., 3][ok].astype(f32)):
        failures.append("coverage differs")
    for q in QUANTITIES:
        a, b = got[q][..., :3][masks[q]].astype(f64), getattr(ref, q)[..., :3][masks[q]]
        err = float(np.abs(a - b).max()) if a.size else 0.0
        print(f"FIRSTHIT {tier} {name} {q} pixels {int(masks[q].sum())} m {m[q]:.3e} tol {tol[q]:.3e} max {err:.3e}")
        if not err <= tol[q]:
            failures.append(f"{q}: max error {err:.3e} > tolerance {tol[q]:.3e} ({err / tol[q]:.1f} x)")
    assert not failures, f"{name}: " + "; ".join(failures)


# ---- CPU tier: the oracle ------------------------------------------------------------------------------------------------------------
def oracle_images(oracle, case):
    scene = scenes.swap_cameras(case.scene, case.camera) if case.camera else case.scene
    st = case.settings
    oracle.set_instancing(case.instancing)
    try:
        osc = oracle.OracleScene(scene, envmap=st.env)
        imgs, _ = osc.render(case.w, case.h, frames=case.frames, max_depth=1, rr_depth=1, ground=tuple(st.ground) + (1.0,),
                             sky=tuple(st.sky) + (1.0,), env_rotation=st.env_rotation, env_intensity=st.env_intensity)
        pos, ids = aov_ref.reference(osc, scene, oracle.pack_lights(scene)[0], case.w, case.h, case.frames)
        osc.close()
    finally:
        oracle.set_instancing(False)
    return dict(radiance=imgs[0], albedo=imgs[1], normal=imgs[2], position=pos, ids=ids)


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_against_float64(oracle, name):
    compare(name, "cpu", oracle_images(oracle, prepared(name)[0]))


def test_mip_bytes_and_lod_definition():
    """the two integer-valued pieces of the reference on values worked out by hand"""
    assert np.array_equal(R.log2a(np.array([1.0, 1.5, 2.0, 3.0, 0.25, 4096.0]), f64), [0.0, 0.5, 1.0, 1.5, -2.0, 12.0])
    lut = R.srgb_lut()
    assert lut[0] == 0.0 and lut[255] == 1.0 and np.all(np.diff(lut) > 0)
    px = np.zeros((2, 2, 4), np.uint8); px[..., 3] = 255
    px[0, 0, :3] = 255  # one white texel of four: box = 0.25 in every channel
    unorm = R.mip_chain(H.HalaImageData(scenes.A_FORMAT_UNORM, 2, 2, px))
    assert len(unorm) == 2 and unorm[1].shape == (1, 1, 4) and np.array_equal(unorm[1][0, 0], [f32(64) / f32(255)] * 3 + [1.0])
    srgb = R.mip_chain(H.HalaImageData(scenes.A_FORMAT_SRGB, 2, 2, px))
    code = int(np.argmin(np.abs(lut.astype(f64) - 0.25)))  # the code nearest to 0.25 in VALUE: 137
    assert code == 137 and np.array_equal(srgb[1][0, 0], [lut[code]] * 3 + [1.0])
    px[0, 0, :3] = (10, 20, 30)
    bgra = R.mip_chain(H.HalaImageData(scenes.A_FORMAT_BGRA_TAG, 2, 2, px))
    assert np.array_equal(bgra[0][0, 0], np.array([30, 20, 10, 255], f32) / f32(255))


def test_rng_stream_is_the_specs():
    """pcg(0) worked out by hand from RENDER_SPEC 2.3, and the stream against unbounded Python integers"""
    def pcg(v):
        s = (v * 747796405 + 2891336453) & 0xFFFFFFFF
        w = (((s >> ((s >> 28) + 4)) ^ s) * 277803737) & 0xFFFFFFFF
        return ((w >> 22) ^ w) & 0xFFFFFFFF
    for w, h, frame in [(48, 40, 0), (50, 37, 2)]:
        state = R.rng_init(w, h, frame)
        for pixel in (0, 1, w, w * h - 1):
            st = pcg((pixel + pcg((frame * 0x9E3779B9 + 0x85EBCA6B) & 0xFFFFFFFF)) & 0xFFFFFFFF)
            assert int(state[pixel]) == st
        r, nxt = R.rand(state, f32)
        assert float(r[5]) == (pcg(int(state[5])) >> 8) * 2.0 ** -24 and int(nxt[5]) == (int(state[5]) + 1) & 0xFFFFFFFF
        assert r.dtype == f32 and np.all((r >= 0) & (r < 1))


# ---- GPU tier: the product -----------------------------------------------------------------------------------------------------------
def product_images(halart, case):
    st = case.settings
    r = halart.HalaRenderer("first-hit", case.w, case.h, 1, 1, False, False, False, 0)
    try:
        if case.build:
            r.set_build_options(**case.build)
        if st.env is not None:
            r.set_envmap(st.env, st.env_rotation)
        r.set_env_intensity(st.env_intensity)
        r.set_ground_color(tuple(st.ground) + (1.0,))
        r.set_sky_color(tuple(st.sky) + (1.0,))
        r.set_scene(case.scene)
        r.commit()
        info = r.bvh_info()
        if case.simple is not None:  # cornell runs the kernels for LDS-resident scenes and the SIMPLE shade variant, the blob neither
            assert (info.lds_node_count > 0) == case.simple
        if "instancing" in case.build:
            assert (info.instance_ref_count > 0) == case.build["instancing"]
        view = 0
        if case.camera:  # two views, so that the VIEWS kernels run; the case's camera is the second one
            r.set_views([0, case.camera])
            view = 1
        r.set_aovs(True, True)
        halart.variant_ledger(4, reset=True)
        for _ in range(case.frames):
            r.update()
        out = dict(radiance=r.read_image(0, view=view), albedo=r.read_image(1, view=view), normal=r.read_image(2, view=view),
                   position=r.read_image("position", view=view), ids=r.read_ids(view=view))
        launched = halart.variant_ledger(4)[0]
    finally:
        r.close()
    return out, launched


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_product_against_float64(halart, name):
    case = prepared(name)[0]
    got, launched = product_images(halart, case)
    assert launched != 0  # the library's own ledger: a k_shade instantiation ran
    name_of, flags = A.VARIANT_FAMILIES[4]
    if case.simple is not None and "SIMPLE" in flags:
        simple_bit = flags.index("SIMPLE")
        ran_simple = any((i >> simple_bit) & 1 for i in range(64) if (launched >> i) & 1)
        assert ran_simple == case.simple, (name_of, bin(launched))
    compare(name, "gpu", got)
