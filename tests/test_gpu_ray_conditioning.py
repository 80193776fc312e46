"""GPU tier (-m gpu): the kernels on GPU-built trees outside the comfortable regime (docs/RENDER_SPEC.md 4.1b, 4.2 "far origins") — the
inputs of tests/test_ray_conditioning.py, which holds the oracle to ground truth on them.  Everything is bit-exact, as in
tests/test_gpu_parity.py: closest hits equal the oracle's brute force in t, u, v and primitive, any hits in t; step counts equal the
oracle's walk over the downloaded tree; the tree passes the structural check."""
import math

import numpy as np
import pytest

import hala_renderer_amd as H
import ray_conditioning as RC
from hala_renderer_amd import scenes
from test_gpu_parity import make_renderer, two_level_trees, validate_tree

pytestmark = pytest.mark.gpu
f32 = np.float32
N = 4000  # rays per family
BUILDERS = ("lbvh", "ploc", "sah")  # the ones tests/test_gpu_parity.py::test_small_trees runs
_REF = {}


def base_scene(name):
    return {"blob": RC.blob_scene, "cornell": scenes.cornell_box, "sheets": lambda: scenes.stacked_sheets(64), "tiny_on_huge": RC.tiny_on_huge}[name]()


def family_rays(osc, far=(1, 2, 3, 4)):
    mn, mx = osc.bounds()
    rays = [RC.near_rays(mn, mx, N, 11), RC.near_axis_rays(mn, mx, N, 12)] + [RC.far_rays(mn, mx, k, N, 20 + k) for k in far]
    return np.concatenate(rays)


def reference(oracle, key, make_scene, make_rays, instancing=False):
    """scene, oracle scene, rays and the oracle's brute-force hits of both ray kinds: computed once per key, shared by the builders"""
    if key not in _REF:
        s = make_scene()
        oracle.set_instancing(instancing)
        try:
            osc = oracle.OracleScene(s)
        finally:
            oracle.set_instancing(False)
        rays = make_rays(s, osc)
        _REF[key] = (s, osc, rays, [osc.trace(rays, mode, brute=True) for mode in (0, 1)])
    return _REF[key]


def assert_renderer_matches(oracle, r, osc, rays, brute, what):
    rc = validate_tree(oracle, osc, r)[0]
    assert rc == 0, f"{what}: validate_tree {rc}"
    nodes, tris = r.download_bvh()
    refs = r.download_instance_refs()
    for mode in (0, 1):
        hits, cnt = r.trace_rays_host(rays, mode, count_steps=True)
        if mode == 0:
            diff = np.nonzero(hits["prim"] != brute[0]["prim"])[0]
            assert hits.tobytes() == brute[0].tobytes(), \
                f"{what}: {len(diff)} of {len(rays)} closest hits name another primitive than brute force, first ray {rays[diff[:1]]} got {hits[diff[:1]]} want {brute[0][diff[:1]]}"
        else:
            assert np.array_equal(hits["t"], brute[1]["t"]), f"{what}: {int((hits['t'] != brute[1]['t']).sum())} any-hit rays differ"
        ohits, ocnt = oracle.trace_on_bvh(nodes, tris, rays, mode, refs if len(refs) else None, bounds=osc.bounds())
        assert cnt == ocnt, f"{what}, mode {mode}: step counts {cnt} != {ocnt}"
        assert np.array_equal(hits["t"], ohits["t"]), f"{what}, mode {mode}: the oracle's walk over the downloaded tree differs"


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("transform", RC.TRANSFORMS, ids=RC.transform_id)
@pytest.mark.parametrize("name", ["cornell", "blob"])
def test_placed_scenes_near_far_and_near_axis_rays(halart, oracle, name, transform, builder):
    """cornell (a tree the kernels hold in LDS) and the 1280-triangle blob (above the 40-KB threshold of RENDER_SPEC 4.4b), scaled and
    offset, with every builder: Morton codes against the scene box, leaf boxes with the box pad, node quantisation — and rays from inside
    the scene, from 10^1 ... 10^4 diagonals away, and nearly along an axis"""
    s, osc, rays, brute = reference(oracle, (name, transform), lambda: RC.placed(base_scene(name), *transform), lambda s, osc: family_rays(osc))
    r = make_renderer(halart, s, 16, 16, build=dict(builder=builder, instancing=False))
    info = r.bvh_info()
    assert (info.lds_node_count > 0) == (name == "cornell")
    omn, omx = osc.bounds()
    assert list(info.scene_min) == list(omn) and list(info.scene_max) == list(omx)
    assert_renderer_matches(oracle, r, osc, rays, brute, f"{name} {RC.transform_id(transform)} {builder}")
    r.close()


@pytest.mark.parametrize("name", ["cornell", "sheets"])
def test_lattice_rays(halart, oracle, name):
    """exactly axis-aligned rays that start on vertex coordinates and run inside face planes"""
    s, osc, rays, brute = reference(oracle, (name, "lattice"), lambda: base_scene(name), lambda s, osc: RC.lattice_rays(osc.triangles(), 4 * N, 31))
    r = make_renderer(halart, s, 16, 16)
    assert_renderer_matches(oracle, r, osc, rays, brute, f"{name} lattice")
    r.close()


@pytest.mark.parametrize("builder", BUILDERS)
def test_tiny_object_on_a_huge_ground(halart, oracle, builder):
    """a 1e-3-sized blob on a 2000-unit quad: pad, Morton grid and node quanta follow the ground, the hits are on the blob"""
    s, osc, rays, brute = reference(oracle, "tiny_on_huge", RC.tiny_on_huge, lambda s, osc: np.concatenate([RC.tiny_on_huge_rays(4 * N, 41), family_rays(osc)]))
    assert ((brute[0]["prim"] != RC.MISS) & (brute[0]["prim"] < 1280)).mean() > 0.1
    r = make_renderer(halart, s, 16, 16, build=dict(builder=builder, instancing=False))
    assert_renderer_matches(oracle, r, osc, rays, brute, f"tiny on huge {builder}")
    r.close()


@pytest.mark.parametrize("levels", ["host", "gpu"])
def test_two_level_tree_with_extreme_instances(halart, oracle, levels):
    """one primitive instanced as it is, with scale 1e-3, scale 1e3, a mirrored scale and at offset 1e4: instance boxes, the entry and
    exit transforms of the two-level walk, instance levels built on the host and on the GPU"""
    s, osc, rays, brute = reference(oracle, "instances", RC.instanced_extremes,
                                    lambda s, osc: np.concatenate([RC.instance_aimed_rays(s, 4 * N, 51), family_rays(osc)]), instancing=True)
    assert set((brute[0]["prim"][brute[0]["prim"] != RC.MISS] // 1280).tolist()) == {0, 1, 2, 3, 4}
    r = make_renderer(halart, s, 16, 16, build=dict(instancing=True, instance_levels=levels))
    info = r.bvh_info()
    assert info.instance_ref_count == 5 and info.stored_triangle_count == 1280
    assert_renderer_matches(oracle, r, osc, rays, brute, f"instances, levels on the {levels}")
    r.close()


def two_blobs():
    s = RC.blob_scene(3)
    m = np.eye(4, dtype=f32); m[:3, 3] = (3.0, 0.5, -1.0)
    s.nodes.insert(1, H.HalaNode(name="blob_b", mesh_index=0, local_transform=m))
    return s


@pytest.mark.parametrize("edit", ["offset", "scale"])
@pytest.mark.parametrize("two_level", [False, True], ids=["one_level", "two_level"])
def test_refit_into_a_bad_regime(halart, oracle, two_level, edit):
    """built near the origin, then the mesh node moved to (1e5, -1e5, 1e5), or scaled by 1e-3, and refitted: the box pad and the far limit
    depend on the scene's largest coordinate, so both must follow the refit.  Hits equal brute force on the edited scene and the bytes a
    fresh commit of the edited scene gives"""
    s = two_blobs() if two_level else RC.blob_scene(3)
    build = dict(instancing=two_level)
    r = make_renderer(halart, s, 16, 16, build=build)
    assert (r.bvh_info().instance_ref_count > 0) == two_level
    m = np.eye(4, dtype=f32)
    if edit == "offset":
        m[:3, 3] = (1e5, -1e5, 1e5)
    else:
        m[:3, :3] *= f32(1e-3)
    r.update_node_transform(0, m)
    r.refit()
    s.nodes[0].local_transform = m
    oracle.set_instancing(two_level)
    try:
        osc = oracle.OracleScene(s)
    finally:
        oracle.set_instancing(False)
    info = r.bvh_info()
    omn, omx = osc.bounds()
    assert list(info.scene_min) == list(omn) and list(info.scene_max) == list(omx)
    rays = np.concatenate([RC.instance_aimed_rays(s, 2 * N, 61), family_rays(osc)])
    brute = [osc.trace(rays, mode, brute=True) for mode in (0, 1)]
    assert (brute[0]["prim"] != RC.MISS).mean() > 0.2
    assert_renderer_matches(oracle, r, osc, rays, brute, f"refit {edit}")
    fresh = make_renderer(halart, s, 16, 16, build=build)
    for mode in (0, 1):
        assert r.trace_rays_host(rays, mode).tobytes() == fresh.trace_rays_host(rays, mode).tobytes()
    r.close(); fresh.close()


def cornell_seen_from(distance_in_diagonals, kind):
    """cornell with its camera on a slightly oblique axis through the box centre, `distance_in_diagonals` away, looking in through the
    open front: orthographic with a 500-unit window, or perspective with yfov narrowed to that window"""
    s = scenes.cornell_box()
    c = np.array([278.0, 274.4, 279.6]); diag = math.sqrt(556.0 ** 2 + 548.8 ** 2 + 559.2 ** 2)
    axis = np.array([0.03, -0.02, 1.0]); axis /= np.linalg.norm(axis)
    dist = distance_in_diagonals * diag
    cam = next(k for k, n in enumerate(s.nodes) if n.camera_index == 0)
    s.nodes[cam] = H.HalaNode(name="camera", camera_index=0, local_transform=scenes.look_at_node_transform(c - axis * dist, c))
    return s, dist


@pytest.mark.parametrize("kind", ["orthographic", "perspective"])
def test_far_cameras(halart, oracle, kind):
    """a camera 10^4 scene diagonals away: the frame is the oracle's bit for bit (the camera-ray launch re-bases as the oracle does),
    and no pixel that the same camera sees as a hit from one diagonal away, moved along its axis, becomes a miss — the window lies
    inside the box's opening, so there every pixel is a hit: a crack would show"""
    w = h = 32
    hit = {}
    for where in (1.0, 1.0e4):
        s, dist = cornell_seen_from(where, kind)
        if kind == "orthographic":
            s.cameras = [H.HalaOrthographicCamera(xmag=250.0, ymag=250.0)]
        else:
            far_dist = cornell_seen_from(1.0e4, kind)[1]
            s.cameras = [H.HalaPerspectiveCamera(aspect=1.0, yfov=2.0 * math.atan(250.0 / far_dist), znear=1.0)]  # the same camera at both places
        osc = oracle.OracleScene(s)
        rays = osc.camera_rays(w, h, 0)
        mn, mx = osc.bounds()
        assert (RC.max_origin_ratio(rays, mn, mx) > RC.K) == (where > 1.0)
        r = make_renderer(halart, s, w, h)
        got = r.trace_rays_host(rays, 0)
        assert got.tobytes() == osc.trace(rays, 0, brute=True).tobytes()
        hit[where] = got["prim"] != RC.MISS
        if where > 1.0:
            r.update(); r.render()
            img, _ = osc.render(w, h, frames=1)
            assert r.read_image(0).tobytes() == img[0].tobytes()
            assert np.isfinite(img[0]).all() and (img[0][..., :3] > 0).any()
        r.close()
    assert hit[1.0].all()
    assert not (hit[1.0] & ~hit[1.0e4]).any()
