"""The control-flow paths of the large-scene traversal kernels (csrc/traverse.h: trav_step, LaneStack; csrc/trace_loop.h: persistent_trace)
against the oracle, bit for bit — no tolerances anywhere.

A wave step decides once, for all its lanes, whether a push or a pop of this step can come near the lane's spill area, and takes a form
without exec-mask regions if none can; the wave loop keeps which lanes hold a ray as scalar lane masks.  What can go wrong there shows
where lanes of ONE wave stand on both sides of such a decision, so every ray set here interleaves rays that build deep stacks (through
the pile of scenes.stacked_sheets: three pushes per step) with rays that never push (they miss the scene) and with camera rays.  Every
scene is larger than the 40-KB LDS staging budget: the large-scene kernels run, never the staged ones."""
import numpy as np
import pytest

import hala_renderer_amd as H
import multihit_ref as MR
from hala_renderer_amd import scenes
from test_gpu_parity import make_renderer
from test_oracle_render import random_rays

gpu = pytest.mark.gpu
f32 = np.float32
A = H._abi
LDS_STAGE_BUDGET = 40 * 1024  # csrc: kLdsStageBudget
STACK_LDS = 8                 # csrc/traverse.h: RT_STACK_LDS, RT_STACK_LDS_INST


def missing_rays(n, mn, mx, seed):
    """rays that start outside the scene box and point away from its centre: they visit the root, hit no child, push nothing"""
    rng = np.random.RandomState(seed)
    c, half = 0.5 * (mn + mx), 0.5 * (mx - mn)
    d = rng.randn(n, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros(n, dtype=A.RAY_DTYPE)
    rays["origin"] = (c + d * (2.5 * float(np.linalg.norm(half)))).astype(f32)
    rays["direction"] = d.astype(f32)
    rays["tmax"] = 3.0e38
    return rays


def interleave(*sets):
    """ray k of every set in turn: neighbouring lanes of a wave get rays of different kinds"""
    n = min(len(s) for s in sets)
    out = np.zeros(n * len(sets), dtype=A.RAY_DTYPE)
    for i, s in enumerate(sets):
        out[i::len(sets)] = s[:n]
    return out


def mixed_rays(osc, w, h, n, seed):
    mn, mx = osc.bounds()
    pad = (mx - mn) * 0.2
    return interleave(osc.camera_rays(w, h, 0), random_rays(n, mn - pad, mx + pad, seed), missing_rays(n, mn, mx, seed + 1))


def assert_large(r, two_level=False):
    i = r.bvh_info()
    assert i.node_count * 64 + i.triangle_count * 48 > LDS_STAGE_BUDGET and i.lds_node_count == 0
    assert (i.instance_ref_count > 0) == two_level
    return i


_SHEETS = {}


def sheets(oracle, count):
    """(scene, oracle scene, rays, brute-force hits per mode): once per count"""
    if count not in _SHEETS:
        s = scenes.stacked_sheets(count)
        osc = oracle.OracleScene(s)
        rays = mixed_rays(osc, 26, 26, 676, 5 + count)  # 3 x 676 = 2028 rays
        _SHEETS[count] = (s, osc, rays, [osc.trace(rays, mode, brute=True) for mode in (0, 1)])
    return _SHEETS[count]


# ---- the spill boundary ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", [0, 1], ids=["closest", "any"])
@pytest.mark.parametrize("count", [512, 2048])
def test_stacks_on_both_sides_of_the_lds_entries(halart, oracle, count, mode):
    s, osc, rays, brute = sheets(oracle, count)
    r = make_renderer(halart, s, 16, 16, build=dict(instancing=False))
    try:
        i = assert_large(r)
        assert 3 * i.max_depth > STACK_LDS  # rays through the pile (three pushes a level) go past the LDS entries; rays that miss never push
        nodes, tris = r.download_bvh()
        hits, cnt = r.trace_rays_host(rays, mode, count_steps=True)
        assert hits.tobytes() == brute[mode].tobytes()
        ohits, ocnt = oracle.trace_on_bvh(nodes.reshape(-1), tris, rays, mode)
        assert cnt == ocnt
        assert hits.tobytes() == ohits.tobytes()
        if mode == 0:  # both kinds of ray are there, in every wave (interleaved by three)
            found = hits["prim"] != 0xFFFFFFFF
            assert found[0::3].any() and found[1::3].any() and not found[2::3].any()
    finally:
        r.close()


# ---- instance variants ---------------------------------------------------------------------------------------------------------------------
_SPONZA = {}


def sponza(oracle, two_level):
    if two_level not in _SPONZA:
        s = scenes.sponza_class(target_triangles=60000, disney=False)
        oracle.set_instancing(two_level)
        try:
            osc = oracle.OracleScene(s)
        finally:
            oracle.set_instancing(False)
        _SPONZA[two_level] = (s, osc, mixed_rays(osc, 32, 18, 576, 31))
    return _SPONZA[two_level]


@gpu
@pytest.mark.parametrize("two_level", [True, False], ids=["two_level", "flattened"])
def test_instanced_and_flattened_tree_walks_are_the_oracles(halart, oracle, two_level):
    s, osc, rays = sponza(oracle, two_level)
    r = make_renderer(halart, s, 16, 16, build=dict(instancing=two_level))
    try:
        assert_large(r, two_level)
        nodes, tris = r.download_bvh()
        refs = r.download_instance_refs()
        for mode in (0, 1):
            hits, cnt = r.trace_rays_host(rays, mode, count_steps=True)
            ohits, ocnt = oracle.trace_on_bvh(nodes.reshape(-1), tris, rays, mode, refs)
            assert cnt == ocnt, mode
            assert hits.tobytes() == ohits.tobytes(), mode
            assert r.trace_rays_host(rays, mode).tobytes() == ohits.tobytes(), mode  # the variant that does not count
    finally:
        r.close()


# ---- ragged batches on a tree that is not staged ------------------------------------------------------------------------------------------
@gpu
def test_ragged_batches_on_a_large_tree(halart, oracle):
    s, osc, _ = sponza(oracle, False)
    mn, mx = osc.bounds()
    r = make_renderer(halart, s, 16, 16, build=dict(instancing=False))
    try:
        assert_large(r)
        for n in (1, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049):  # 2048 = 16 shards x 128
            rays = random_rays(n, mn, mx, 100 + n)
            rays["tmax"][::7] = 0.0
            z = np.arange(n) % 5 == 3  # zero direction components, no NaN: the other two components keep the direction's length above zero
            rays["direction"][z, n % 3] = 0.0
            for mode in (0, 1):
                assert r.trace_rays_host(rays, mode).tobytes() == osc.trace(rays, mode).tobytes(), (n, mode)
    finally:
        r.close()


# ---- fused against per-pass frames ---------------------------------------------------------------------------------------------------------
@gpu
def test_fused_and_per_pass_frames_are_the_oracles(halart, oracle):
    w, h = 64, 36
    s = scenes.sponza_class(target_triangles=60000, disney=False)
    mn, mx = oracle.OracleScene(s).bounds()
    lm = np.eye(4, dtype=f32)
    lm[:3, :3] = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], dtype=f32)  # the quad faces down
    lm[:3, 3] = (0.5 * (mn[0] + mx[0]), mn[1] + 0.8 * (mx[1] - mn[1]), 0.5 * (mn[2] + mx[2]))
    s.nodes.append(H.HalaNode(name="quad_light", light_index=len(s.lights), local_transform=lm))
    s.lights = list(s.lights) + [H.HalaLight(color=(1.0, 0.9, 0.8), intensity=40.0, light_type=H.HalaLightType.QUAD, params=(1.0, 1.0))]
    env = scenes.sky_sun_envmap(128, 64, sun_gain=300.0)
    want, _ = oracle.OracleScene(s, envmap=env).render(w, h, frames=2, max_depth=5, rr_depth=3)
    want = [x.tobytes() for x in want]
    for fusion in (2, 0):
        for in_flight in (1, 2):
            r = make_renderer(halart, s, w, h, max_depth=5, rr_depth=3, env=env, build=dict(instancing=False))
            try:
                assert_large(r)
                r.set_pass_fusion(fusion)
                r.set_frames_in_flight(in_flight)
                r.update_batch(2)
                r.render()
                got = [r.read_image(k).tobytes() for k in range(4)]
            finally:
                r.close()
            assert got == want, (fusion, in_flight)


# ---- multi-hit: the stepper shares LaneStack and the instance entry / exit ---------------------------------------------------------------
@gpu
def test_multi_hit_lists_through_the_pile(halart, oracle):
    s, osc, rays, _ = sheets(oracle, 512)
    rays = rays[:900]
    full = MR.Twin(s, osc, False).lists(rays)
    want, want_counts = MR.cut(full, 4)
    r = make_renderer(halart, s, 16, 16, build=dict(instancing=False))
    try:
        assert_large(r)
        got, counts = r.trace_rays_multi_host(rays, 4)
        assert got.tobytes() == want.tobytes()
        assert counts.tobytes() == want_counts.tobytes()
    finally:
        r.close()
