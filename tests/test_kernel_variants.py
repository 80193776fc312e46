"""Every compiled instantiation of the six flag-dispatched kernel families (csrc/variants.h `dispatch`: k_trace_primary,
k_trace_batch, k_trace_shadow, k_trace_shadow_then_batch, k_shade, k_resolve) is launched here on the smallest scene that selects it and
compared with the oracle bit for bit.  Which instantiations exist and which a process has launched comes from the library's own ledger
(hala_rt_variant_ledger), so a new launch flag doubles a `built` mask and the closing test of this module fails until a case reaches
the new kernels.

The cases are not written down: `AXES` spans them, `expected_bits` says from the launcher rules which instantiations a case launches,
and `CASES` is the greedy minimal subset whose expected bits cover every built instantiation that is not in `UNREACHABLE`.  Each case
renders 24 x 17 pixels (partial 8 x 8 blocks on both edges), two frames in one update_batch, max_depth 3 (a camera launch, two bounce
launches, fused middle bounces and a last bounce), asserts that the ledger shows exactly the expected instantiations, and compares every
image the case has with the reference the feature's own test uses."""
import collections
import contextlib
import copy
import itertools
import math
import os

import numpy as np
import pytest

import aov_ref
import hala_renderer_amd as H
import ray_conditioning as RC
from hala_renderer_amd import scenes
from test_gpu_parity import make_renderer, two_level_trees
from test_gpu_ray_conditioning import two_blobs
from test_light_groups import isolated_accum

gpu = pytest.mark.gpu
f32 = np.float32
W, HT, FRAMES, MAX_DEPTH, RR_DEPTH = 24, 17, 2, 3, 2
FAR_DIAGONALS = 1.0e4  # as tests/test_gpu_ray_conditioning.py::cornell_seen_from
FAMILIES = H._abi.VARIANT_FAMILIES
NAMES = ("accum", "albedo", "normal", "final")

# Built instantiations no scene can select: {family: {bit: the lines that make the combination impossible}}.  At most 4 bits.
UNREACHABLE = {
    3: {
        # k_trace_shadow_then_batch<ALPHA, STAGED, !INST, GROUPS>, flags in dispatch order (ALPHA, STAGED, INST, GROUPS)
        0b0011: "ALPHA = sv.any_translucent: a material of any-hit class >= 2, which also sets any_invisible (rt_trees.hip attach_any_triangles: "
                "`r->any_invisible = r->any_invisible || cls[i] != 0`), so sv.tris_any is the separate d_tris_any copy (renderer_state.h view(): "
                "`sv.tris_any = any_invisible ? d_tris_any.ptr : d_tris.ptr`) and trace_shadow.hip launch_trace_shadow_then_batch returns false "
                "before it launches: `if (tree == TreeForm::Staged && sv.tris_any != sv.tris) return false;`",
        0b1011: "the same with GROUPS: the refusal comes before the flags are looked at",
    },
}
assert sum(len(v) for v in UNREACHABLE.values()) <= 4


def _library():
    if not os.path.exists(H.LIB_PATH):  # as the `halart` fixture: a missing library is built, never skipped
        import __graft_entry__
        __graft_entry__.build()
    return H.load_library()


def built_masks():
    _library()
    return [H.variant_ledger(f)[1] for f in range(len(FAMILIES))]


def bit(*flags):
    """the ledger bit of a flag combination: the flags read as a binary number, first flag least significant"""
    return 1 << sum(int(bool(x)) << i for i, x in enumerate(flags))


def describe(family, index):
    name, flags = FAMILIES[family]
    return f"{name}<" + ", ".join(f"{fl}={(index >> i) & 1}" for i, fl in enumerate(flags)) + ">"


def bits_of(mask):
    return [i for i in range(64) if (mask >> i) & 1]


# ---- the axes ---------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "tree mode alpha groups aov views count fuse kinds far")
AXES = collections.OrderedDict([
    ("tree", ("staged", "large", "inst")),        # cornell (LDS-staged) | blob_scene(3), 1280 triangles | two_blobs() with instancing
    ("mode", ("simple", "generic", "scatter")),   # untextured opaque diffuse | textured Disney + diffuse (shade_sort) | + a scattering medium
    ("alpha", (False, True)),                     # a translucent or medium-bounding material: any-hit class >= 2
    ("groups", (False, True)),                    # set_light_groups
    ("aov", (False, True)),                       # set_aovs(position, ids)
    ("views", (False, True)),                     # set_views with two cameras
    ("count", (False, True)),                     # set_counting
    ("fuse", (True, False)),                      # set_pass_fusion(2 / 0)
    ("kinds", (1, 3, 0, 2)),                      # bit 0: lights, bit 1: a sampled environment
    ("far", (False, True)),                       # a camera FAR_DIAGONALS scene diagonals away
])


def case_id(c):
    on = [k for k in ("alpha", "groups", "aov", "views", "count", "far") if getattr(c, k)]
    return "-".join([c.tree, c.mode, {0: "dark", 1: "lights", 2: "env", 3: "lights+env"}[c.kinds], "fused" if c.fuse else "separate"] + on)


def possible(c):
    return not (c.mode == "simple" and c.alpha)  # a translucent material is not a SIMPLE one (hala_types.h shade_kind_of)


def expected_bits(c):
    """per family, the instantiations the case launches (renderer.hip issue_bounces / finish_update, rt_rays.hip, the launchers of trace_closest.hip, trace_shadow.hip, shade.hip, resolve.hip)"""
    staged, inst = c.tree == "staged", c.tree == "inst"
    simple, scatter = c.mode == "simple", c.mode == "scatter"
    e = [0] * len(FAMILIES)
    e[0] = bit(c.count, staged, inst, c.views, c.far)
    # the case's two caller batches (closest and any-hit, counted when the case counts); the closest-hit bounce launches of an update
    # that does not fuse are the first of the two kernels again
    e[1] = bit(0, c.count, 0, staged, inst) | bit(1, c.count, c.alpha, staged, inst)
    # the fused launch needs lights or an environment, never counts, and refuses a staged tree with a separate any-hit triangle copy
    fused = c.fuse and not c.count and c.kinds != 0 and not (staged and c.alpha)
    if fused:
        e[3] = bit(c.alpha, staged, inst, c.groups and c.kinds & 1)
    # separate shadow launches: every bounce of an update that does not fuse; the last bounce of one that does, unless it has both kinds
    separate = c.kinds if not fused or c.kinds != 3 else 0
    if separate & 1:
        e[2] |= bit(c.count, c.alpha, staged, inst, c.groups)
    if separate & 2:
        e[2] |= bit(c.count, c.alpha, staged, inst, 0)  # environment connections carry no group
    # AOV goes only with PRIMARY (the depth-0 shade)
    e[4] = bit(1, simple, scatter, c.aov, c.groups) | bit(0, simple, scatter, 0, c.groups)
    e[5] = bit(c.aov, c.groups)
    return e


def reachable_masks():
    return [b & ~sum(1 << i for i in UNREACHABLE.get(f, {})) for f, b in enumerate(built_masks())]


def launch_sequence_goals(c):
    """what the set has to cover besides kernels, none of which is an instantiation of its own: the depth-0 AOV shade behind a far
    camera ray (it evaluates the camera ray again and adds the reported t), once per tree form; an update without any connection (closest
    hits only); an update whose every bounce issues both shadow passes as launches of their own"""
    goals = 1 << AXES["tree"].index(c.tree) if c.far and c.aov else 0
    goals |= 1 << 3 if c.kinds == 0 else 0
    goals |= 1 << 4 if c.kinds == 3 and not c.fuse and not c.count else 0
    return goals


def greedy_cases():
    """a minimal set of cases, by greedy set cover in the order of AXES, whose expected bits cover every reachable built bit (and
    launch_sequence_goals)"""
    todo = reachable_masks() + [(1 << 5) - 1]
    pool = [c for c in (Case(*v) for v in itertools.product(*AXES.values())) if possible(c)]
    exp = {c: expected_bits(c) + [launch_sequence_goals(c)] for c in pool}
    chosen = []
    while any(todo):
        gain, best = max(((sum(bin(e & t).count("1") for e, t in zip(exp[c], todo)), -k), c) for k, c in enumerate(pool))
        if gain[0] == 0:
            break  # what is left is reported by test_the_case_set_covers_every_reachable_instantiation and by the closing test
        chosen.append(best)
        todo = [t & ~e for t, e in zip(todo, exp[best])]
    return chosen


CASES = greedy_cases()
LAUNCHED = [0] * len(FAMILIES)  # the union over this module's own cases
RAN = set()


@pytest.fixture(scope="module", autouse=True)
def fresh_ledger():
    _library()
    for f in range(len(FAMILIES)):
        H.variant_ledger(f, reset=True)
    yield


# ---- CPU tier ---------------------------------------------------------------------------------------------------------------------------
def test_ledger_entry_point(halart):
    lib = halart.load_library()
    assert lib.hala_rt_variant_ledger(99, None, None, 0) != 0
    assert "99" in halart.last_error()
    with pytest.raises(halart.HalaRendererError, match="family"):
        halart.variant_ledger(len(FAMILIES))
    for f in range(len(FAMILIES)):
        assert lib.hala_rt_variant_ledger(f, None, None, 0) == 0
        assert lib.hala_rt_variant_ledger(f, None, None, 1) == 0
        launched, built = halart.variant_ledger(f)
        assert launched & ~built == 0


def test_built_instantiations_per_family(halart):
    """a new launch flag changes one of these numbers: then AXES and expected_bits need the flag too"""
    assert [bin(b).count("1") for b in built_masks()] == [24, 18, 24, 12, 18, 4]
    assert [len(flags) for _, flags in FAMILIES] == [5, 5, 5, 4, 5, 2]
    for f, bits in UNREACHABLE.items():
        for i in bits:
            assert (built_masks()[f] >> i) & 1, describe(f, i)


def test_the_case_set_covers_every_reachable_instantiation():
    covered = [0] * len(FAMILIES)
    for c in CASES:
        covered = [a | b for a, b in zip(covered, expected_bits(c))]
    missing = [describe(f, i) for f, (r, got) in enumerate(zip(reachable_masks(), covered)) for i in bits_of(r & ~got)]
    assert not missing, f"no case of AXES launches {missing}"
    assert len(CASES) <= 48, len(CASES)


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------
def with_ground(s, half_x):
    """the blob scenes get a second material to be of two kinds with: a diffuse ground quad under the blobs"""
    ground = scenes._merge_quads([((-half_x, -1.4, 3.0), (half_x + 3.0, -1.4, 3.0), (half_x + 3.0, -1.4, -3.0), (-half_x, -1.4, -3.0))])
    ground.material_index = len(s.materials)
    s.materials.append(H.HalaMaterial(type=0, base_color=(0.5, 0.5, 0.5), roughness=0.0))
    s.meshes.append(H.HalaMesh([ground]))
    s.nodes.append(H.HalaNode(name="ground", mesh_index=len(s.meshes) - 1))
    return s


def base_scene(c):
    """-> (scene, index of the material the mode changes, eye and target of camera 0, a length of the scene's size)"""
    if c.tree == "staged":
        s = scenes.cornell_box(aspect=W / HT, analytic_light=bool(c.kinds & 1))
        return s, 4, (278.0, 273.0, -800.0), (278.0, 273.0, 0.0), 150.0
    s = with_ground(RC.blob_scene(3) if c.tree == "large" else two_blobs(), 3.0)
    if c.kinds & 1:
        m = np.eye(4, dtype=f32)
        m[:3, 0] = (1, 0, 0); m[:3, 1] = (0, 0, 1); m[:3, 2] = (0, -1, 0); m[:3, 3] = (0.5, 2.8, 0.5)
        s.nodes.append(H.HalaNode(name="light", light_index=0, local_transform=m))
        s.lights = [H.HalaLight(color=(1.0, 0.9, 0.8), intensity=17.0, light_type=H.HalaLightType.QUAD, params=(1.0, 1.0))]
    return s, 0, (0.0, 0.6, 4.2), (0.0, 0.0, 0.0), 1.0


def apply_materials(s, c, main, size):
    if c.mode == "generic":
        for img in scenes.procedural_texture_set(32, 100, (0.85, 0.8, 0.7)):
            idx = len(s.image_data)
            s.image_data.append(img); s.image2data_mapping[idx] = idx; s.texture2image_mapping[idx] = idx
        s.materials[main] = H.HalaMaterial(type=1, base_color=(0.8, 0.6, 0.4), roughness=0.35, metallic=0.0, opacity=0.6 if c.alpha else 1.0,
                                           base_color_map_index=0, normal_map_index=1, metallic_roughness_map_index=2)
    elif c.mode == "scatter":
        med = H.HalaMedium(2, (0.95, 0.7, 0.4), 3.0 / size, 0.6)
        if c.alpha:  # an invisible boundary of the medium: any-hit class 3
            s.materials[main] = H.HalaMaterial(type=0, base_color=(1.0, 1.0, 1.0), roughness=0.5, opacity=0.0, medium=med)
        else:  # glass: every hit blocks a connection
            s.materials[main] = H.HalaMaterial(type=1, base_color=(1.0, 1.0, 1.0), metallic=0.0, roughness=0.15, specular_transmission=1.0, ior=1.45, medium=med)


def far_camera(mn, mx):
    """as cornell_seen_from: on a slightly oblique axis through the centre of the scene box, FAR_DIAGONALS diagonals away, looking at
    it, yfov narrowed to a window inside the box -> (node transform, camera, distance)"""
    mn = mn.astype(np.float64); mx = mx.astype(np.float64)
    ctr = 0.5 * (mn + mx); diag = float(np.linalg.norm(mx - mn))
    axis = np.array([0.03, -0.02, 1.0]); axis /= np.linalg.norm(axis)
    dist = FAR_DIAGONALS * diag
    half = 0.45 * float(min(mx[0] - mn[0], mx[1] - mn[1]))
    return (scenes.look_at_node_transform(ctr - axis * dist, ctr), H.HalaPerspectiveCamera(aspect=W / HT, yfov=2.0 * math.atan(half / dist), znear=1.0), dist)


def build_case(oracle, c):
    """-> dict: scene, env, cams (the view list), far (per view), dist (of the far camera), part (the light groups)"""
    s, main, eye, target, size = base_scene(c)
    apply_materials(s, c, main, size)
    probe = oracle.OracleScene(s)
    mn, mx = probe.bounds()
    probe.close()
    cam_node = next(k for k, n in enumerate(s.nodes) if n.camera_index == 0)
    far_xf, far_cam, dist = far_camera(mn, mx)
    cams, far = [0], [False]
    if c.views:
        if c.far:  # one near and one far camera
            xf, cam = far_xf, far_cam
        else:
            e = np.asarray(eye) + 0.1 * np.linalg.norm(np.asarray(eye) - np.asarray(target)) * np.array([1.0, 0.5, 0.0])
            xf, cam = scenes.look_at_node_transform(e, target), copy.copy(s.cameras[0])
        s.cameras = [s.cameras[0], cam]
        s.nodes.append(H.HalaNode(name="camera_1", camera_index=1, local_transform=xf))
        cams, far = [0, 1], [False, c.far]
    elif c.far:
        s.cameras = [far_cam]
        s.nodes[cam_node] = H.HalaNode(name="camera", camera_index=0, local_transform=far_xf)
        far = [True]
    env = scenes.sky_sun_envmap(64, 32, sun_gain=50.0) if c.kinds & 2 else None
    n_lights = len(oracle.pack_lights(s)[0])
    part = ([0] * n_lights, [k % 2 for k in range(len(s.materials))], 1) if c.groups else None  # the lights | the environment; the materials split
    return dict(scene=s, env=env, cams=cams, far=far, dist=dist, part=part, bounds=(mn, mx))


def oracle_scene_of_view(oracle, b, v):
    scene = scenes.swap_cameras(b["scene"], b["cams"][v]) if b["cams"][v] else b["scene"]  # the rule of tests/test_views.py
    return scene, oracle.OracleScene(scene, envmap=b["env"])


# ---- the position AOV of a far camera against float64 ------------------------------------------------------------------------------------
# Between the float32 camera ray (o, d), the hit distance t that RENDER_SPEC 4.2 reports, and the stored mean there are four roundings
# that any evaluation in the spec's order goes through, each of a value no larger than the camera's distance D (o, t and every partial
# result lie within D + one diagonal of the origin), so each is at most half the float32 spacing at D:
#   4.2   o' = fma(d, ts, o)      1 rounding      (the re-based origin)
#   4.2   t  = t' + ts            1 rounding      (the reported distance)
#   13    P  = madd(d, t, o)      1 rounding
#   8     fold_mean of 2 frames   1 rounding      (mean x 1 and / 2 are exact)
# Against origin + t * direction evaluated in float64 from the oracle's (o, t, d) of each frame the bound is therefore
# 4 x 1/2 = 2 spacings at D.  (A kernel that added t to the re-based origin, or t' to the given one, is off by ts: 10^7 spacings.)
POSITION_FACTOR = 2.0


def position_error_in_bound(oracle, osc, scene, position, dist, bounds):
    """max |position.xyz - float64 mean of origin + t * direction| over the pixels whose sample hit a triangle in every frame, in units of
    the bound; and how many pixels that were"""
    lights = oracle.pack_lights(scene)[0]
    mn, mx = bounds
    spacing = float(np.spacing(f32(dist + float(np.linalg.norm(mx.astype(np.float64) - mn.astype(np.float64))))))
    ref = np.zeros((HT * W, 3)); ok = np.ones(HT * W, dtype=bool)
    for f in range(FRAMES):
        rays = osc.camera_rays(W, HT, f)
        assert RC.max_origin_ratio(rays, mn, mx) > RC.K  # the oracle re-bases these rays too
        hit = osc.trace(rays, 0, brute=True)
        ids = aov_ref.first_hits(osc, scene, lights, W, HT, f)[1].reshape(-1, 4)
        ok &= (hit["prim"] != RC.MISS) & (ids[:, 3] == hit["prim"])  # not a light in front of the triangle
        ref += rays["origin"].astype(np.float64) + hit["t"].astype(np.float64)[:, None] * rays["direction"].astype(np.float64)
    ref /= FRAMES
    got = position.reshape(-1, 4)
    assert (got[ok, 3] == 1.0).all()
    err = np.abs(got[ok, :3].astype(np.float64) - ref[ok]).max() if ok.any() else 0.0
    return err / (POSITION_FACTOR * spacing), int(ok.sum())


FAR_AOV_CASES = [c for c in CASES if c.far and c.aov]


def test_some_case_checks_the_far_position_aov():
    assert {c.tree for c in FAR_AOV_CASES} == set(AXES["tree"]), "k_shade<PRIMARY, AOV> behind a far camera ray: one case per tree form"


@pytest.mark.parametrize("c", FAR_AOV_CASES, ids=case_id)
def test_oracle_far_position_stays_inside_the_float64_bound(oracle, c):
    """CPU: the reference the GPU cases are compared with bit for bit is itself within the bound of the float64 evaluation"""
    with two_level_trees(oracle) if c.tree == "inst" else contextlib.nullcontext():
        b = build_case(oracle, c)
        v = b["far"].index(True)
        scene, osc = oracle_scene_of_view(oracle, b, v)
        pos, _ = aov_ref.reference(osc, scene, oracle.pack_lights(scene)[0], W, HT, FRAMES)
        err, n = position_error_in_bound(oracle, osc, scene, pos, b["dist"], b["bounds"])
        osc.close()
    print(f"{case_id(c)}: {n} pixels, error {err:.3g} of the bound")
    assert n > W * HT // 8 and err <= 1.0, (n, err)


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------------------
def assert_same(got, want, what):
    if got.tobytes() != want.tobytes():
        bad = np.any(got.reshape(HT, W, -1) != want.reshape(HT, W, -1), axis=-1)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} pixels differ")


@gpu
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_variant_case(halart, oracle, c):
    with two_level_trees(oracle) if c.tree == "inst" else contextlib.nullcontext():
        run_case(halart, oracle, c)


def run_case(halart, oracle, c):
    b = build_case(oracle, c)
    s, env, cams = b["scene"], b["env"], b["cams"]
    mn, mx = b["bounds"]
    kw = dict(width=W, height=HT, max_depth=MAX_DEPTH, rr_depth=RR_DEPTH, tonemap=(False, False, False), env_rotation=0.0, env_intensity=1.0, exposure=1.0)
    expected = expected_bits(c)
    for f in range(len(FAMILIES)):
        halart.variant_ledger(f, reset=True)
    r = make_renderer(halart, s, W, HT, max_depth=MAX_DEPTH, rr_depth=RR_DEPTH, env=env, build=dict(instancing=c.tree == "inst"))
    try:
        info = r.bvh_info()
        assert (info.lds_node_count > 0) == (c.tree == "staged"), "the case landed on another tree form"
        assert (info.instance_ref_count > 0) == (c.tree == "inst"), "the case landed on another tree form"
        r.set_pass_fusion(2 if c.fuse else 0)
        r.set_counting(c.count)
        if c.aov:
            r.set_aovs(position=True, ids=True)
        if c.groups:
            r.set_light_groups(lights=b["part"][0], environment=b["part"][2], materials=b["part"][1], group_count=2)
        if c.views:
            r.set_views(cams)
        r.update_batch(FRAMES)
        r.render()
        images = [[r.read_image(k, view=v) for k in range(4)] for v in range(len(cams))]
        aovs = [(r.read_image(4, view=v), r.read_ids(view=v)) for v in range(len(cams))] if c.aov else None
        group_images = [[r.read_light_group(g, view=v) for g in range(2)] for v in range(len(cams))] if c.groups else None
        st = r.statistics()
        # the two caller batches: view 0's camera rays, closest and any hit
        scene0, osc0 = oracle_scene_of_view(oracle, b, 0)
        rays = osc0.camera_rays(W, HT, 0)
        batches = [r.trace_rays_host(rays, mode, count_steps=c.count) for mode in (0, 1)]
        nodes, tris = r.download_bvh()
        refs = r.download_instance_refs()
        launched = [halart.variant_ledger(f)[0] for f in range(len(FAMILIES))]
    finally:
        r.close()
    for f in range(len(FAMILIES)):
        LAUNCHED[f] |= launched[f]
    RAN.add(c)

    # the ledger: exactly the instantiations the launcher rules give
    for f in range(len(FAMILIES)):
        assert launched[f] == expected[f], (f"{FAMILIES[f][0]}: launched {[describe(f, i) for i in bits_of(launched[f])]}, "
                                            f"expected {[describe(f, i) for i in bits_of(expected[f])]}")

    # the caller batches against brute force (and, counted, the oracle's walk over the downloaded tree)
    two = refs if len(refs) else None
    for mode in (0, 1):
        got = batches[mode][0] if c.count else batches[mode]
        want = osc0.trace(rays, mode, brute=True)
        if mode == 0:
            assert got.tobytes() == want.tobytes(), "closest-hit batch"
        else:
            assert np.array_equal(got["t"], want["t"]), "any-hit batch"
        # counted: the oracle's walk over the renderer's own tree, with the scene's materials (an any-hit ray passes translucent
        # surfaces, which a tree traced without its scene cannot know)
        if c.count:
            osc0.use_bvh(nodes, tris, two)
            ohits, ocnt = osc0.trace_on_used_bvh(rays, mode)
            osc0.use_bvh(None)
            assert np.array_equal(got["t"], ohits["t"]), f"mode {mode}: the oracle's walk over the downloaded tree differs"
            assert batches[mode][1] == ocnt, f"step counts of the caller batch, mode {mode}: {batches[mode][1]} != {ocnt}"
    osc0.close()

    # every view against the oracle's render of the scene with that view's camera as camera 0
    onodes = otris = 0
    for v in range(len(cams)):
        scene, osc = oracle_scene_of_view(oracle, b, v)
        orays = osc.camera_rays(W, HT, 0)
        assert (RC.max_origin_ratio(orays, mn, mx) > RC.K) == b["far"][v], "the oracle re-bases the rays of the far cameras, and of no other"
        if c.count:
            osc.use_bvh(nodes, tris, two)  # step counts are compared on the renderer's own tree; the images do not depend on the tree
        want, ost = osc.render(W, HT, frames=FRAMES, max_depth=MAX_DEPTH, rr_depth=RR_DEPTH)
        onodes += ost.nodes_visited; otris += ost.triangles_tested
        if c.count:
            osc.use_bvh(None)
        for k, name in enumerate(NAMES):
            assert_same(images[v][k], want[k], f"view {v} {name}")
        if c.aov:
            pos, ids = aov_ref.reference(osc, scene, oracle.pack_lights(scene)[0], W, HT, FRAMES)
            assert_same(aovs[v][0], pos, f"view {v} position")
            assert_same(aovs[v][1], ids, f"view {v} ids")
            if b["far"][v]:
                err, n = position_error_in_bound(oracle, osc, scene, aovs[v][0], b["dist"], b["bounds"])
                print(f"view {v}: far position AOV, {n} pixels, error {err:.3g} of the bound")
                assert n > W * HT // 8 and err <= 1.0, (n, err)
        if c.groups:
            for g in range(2):
                assert_same(group_images[v][g], isolated_accum(oracle, scene, env, kw, b["part"], g, FRAMES), f"view {v} light group {g}")
        osc.close()
    if c.count:
        got = (st.nodes_closest_total + st.nodes_shadow_total, st.tris_closest_total + st.tris_shadow_total)
        print(f"step counts: renderer {got}, oracle {(onodes, otris)}")
        assert got == (onodes, otris), f"step counts of the update: {got} != {(onodes, otris)}"


@gpu
def test_every_built_instantiation_was_launched():
    """the closing test: per family, launched | unreachable == built, from this module's own cases"""
    if len(RAN) < len(CASES):
        pytest.skip(f"only {len(RAN)} of the module's {len(CASES)} cases ran (deselected?): their union says nothing")
    missing, beyond = [], []
    for f, built in enumerate(built_masks()):
        un = sum(1 << i for i in UNREACHABLE.get(f, {}))
        missing += [describe(f, i) for i in bits_of(built & ~(LAUNCHED[f] | un))]
        beyond += [describe(f, i) for i in bits_of(LAUNCHED[f] & (un | ~built))]
    assert not beyond, f"launched although held unreachable or not built: {beyond}"
    assert not missing, f"built, but launched by no case: {missing}"
