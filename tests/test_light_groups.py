"""Light groups (docs/RENDER_SPEC.md 14): the beauty image split by emitter, and the relight of the accumulated frame.  Image g of a renderer
equals, bit for bit, the oracle's accum of the isolated scene of g (every emitter outside g zeroed: tests/light_group_ref.py::isolate).
CPU tier: the header and the exports, the descriptor's refusals before any device call, the isolation helper on the oracle alone, the
relight twin.  GPU tier: group images against the oracle's isolated scenes — random scenes with random partitions (SKY and MAP), the
SIMPLE kernels, a textured Disney scene, two-level trees, update_batch, views, adaptive sampling, pass fusion and the tail overlap —
images 0-5 unchanged by the feature, the relight, and the refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import light_group_ref as R
from conftest import ROOT
from hala_renderer_amd import scenes

gpu = pytest.mark.gpu
W, H = 61, 37
f32 = np.float32
SEEDS = [17, 25, 20, 12, 22]  # the random scenes of test_aovs.py: every light type, EMISSIVE media, emission maps, SKY and MAP
CPU_SEEDS = [17, 22, 25, 20, 28]
ENTRY_POINTS = ("hala_rt_set_light_groups", "hala_rt_read_light_group", "hala_rt_relight", "hala_rt_read_relit", "hala_rt_get_relit_buffer")


# ---- CPU tier ----------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_light_group_entry_points(halart):
    text = open(os.path.join(ROOT, "include", "halart.h")).read()
    assert re.search(r"typedef struct hala_light_groups \{.*?\} hala_light_groups;", text, flags=re.S)
    for fn in ENTRY_POINTS:
        assert re.search(r"int " + fn + r"\(hala_rt_renderer\* r,", text), fn
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*typedef struct hala_light_groups", text, flags=re.S)
    assert m
    for w in ("RENDER_SPEC.md 14", "isolated scene", "0 * inf", "world > 1", "restarts the accumulation", "2^29"):
        assert w in m.group(1), w
    lib = C.CDLL(halart.LIB_PATH)
    for fn in ENTRY_POINTS:
        assert fn in halart._abi.EXPORTS and hasattr(lib, fn), fn
    assert C.sizeof(halart._abi.LightGroups) == 32


def descriptor(halart, group_count=2, env=0, lights=(0, 1), materials=(1,), null_lights=False, null_materials=False):
    A = halart._abi
    g = A.LightGroups()
    g.group_count, g.environment_group = group_count, env
    la, ma = (C.c_uint32 * max(len(lights), 1))(*lights), (C.c_uint32 * max(len(materials), 1))(*materials)
    g.light_count, g.material_count = len(lights), len(materials)
    g.light_group = None if null_lights else C.cast(la, C.POINTER(C.c_uint32))
    g.material_group = None if null_materials else C.cast(ma, C.POINTER(C.c_uint32))
    return g, (la, ma)


@pytest.mark.parametrize("kw,word", [
    (dict(group_count=0), "group_count"), (dict(group_count=9), "group_count"),
    (dict(env=2), "environment"), (dict(lights=(0, 2)), "light 1"), (dict(materials=(0, 0, 5)), "material 2"),
    (dict(null_lights=True), "null"), (dict(null_materials=True), "null"),
])
def test_invalid_descriptors_are_refused_before_any_device_call(halart, kw, word):
    lib = halart.load_library()
    g, keep = descriptor(halart, **kw)
    assert lib.hala_rt_set_light_groups(None, C.byref(g)) == 1  # validated before the renderer handle is looked at
    assert word in halart.last_error()


def test_valid_descriptor_reaches_the_handle_check(halart):
    lib = halart.load_library()
    g, keep = descriptor(halart, group_count=8, env=7, lights=(7, 0, 3), materials=())
    assert lib.hala_rt_set_light_groups(None, C.byref(g)) == 1 and "null" in halart.last_error()
    for fn, args in (("hala_rt_read_light_group", (C.c_uint32(0), C.c_uint32(0), None)), ("hala_rt_relight", (C.c_uint32(0), None, C.c_uint32(1))),
                     ("hala_rt_read_relit", (C.c_int(0), None))):
        assert getattr(lib, fn)(None, *args) == 1 and "null" in halart.last_error(), fn


def isolated_accum(oracle, scene, env, kw, part, g, frames, first_frame=0):
    lg, mg, eg = part
    iso, keep_env = R.isolate(scene, lg, mg, eg, g)
    osc = oracle.OracleScene(iso, envmap=env)
    imgs, _ = osc.render(kw["width"], kw["height"], frames=frames, first_frame=first_frame, max_depth=kw["max_depth"], rr_depth=kw["rr_depth"],
                         env_rotation=kw["env_rotation"] if env is not None else 0.0, env_intensity=kw["env_intensity"] if keep_env else 0.0,
                         exposure=kw["exposure"], tonemap=kw["tonemap"])
    osc.close()
    return imgs[0]


def test_isolation_helper_zeroes_exactly_the_other_groups(oracle):
    from random_scenes import random_scene
    s, env, kw = random_scene(17)
    lights, _ = oracle.pack_lights(s)
    part = ([0] * len(lights), [k % 2 for k in range(len(s.materials))], 1)
    iso, keep_env = R.isolate(s, *part, 0)
    assert keep_env is False
    packed, _ = oracle.pack_lights(iso)
    assert len(packed) == len(lights)
    for a, b in zip(packed, lights):  # group 0 keeps every light as it was
        assert bytes(a) == bytes(b)
    for m, (a, b) in enumerate(zip(iso.materials, s.materials)):
        if m % 2 == 0:
            assert a == b
        else:
            assert a.emission == (0.0, 0.0, 0.0) and a.base_color == b.base_color
            assert a.medium.type == b.medium.type and a.medium.density == b.medium.density
            if b.medium.type == 3:
                assert a.medium.color == (0.0, 0.0, 0.0)
    iso1, keep1 = R.isolate(s, *part, 1)
    assert keep1 is True and all(L.intensity[0] == 0.0 for L in oracle.pack_lights(iso1)[0])


@pytest.mark.parametrize("seed", CPU_SEEDS)
def test_isolated_scenes_sum_to_the_full_render(oracle, seed):
    """the oracle alone: the isolated renders of a random partition into three groups sum to the full render (float tolerance: the
    sums are rounded in another order)"""
    from random_scenes import random_scene
    s, env, kw = random_scene(seed)
    kw = dict(kw, width=32, height=20)
    lights, _ = oracle.pack_lights(s)
    part = R.random_partition(np.random.RandomState(seed), len(lights), len(s.materials), 3)
    osc = oracle.OracleScene(s, envmap=env)
    full, _ = osc.render(32, 20, frames=2, max_depth=kw["max_depth"], rr_depth=kw["rr_depth"], env_rotation=kw["env_rotation"] if env is not None else 0.0,
                         env_intensity=kw["env_intensity"])
    osc.close()
    total = sum(isolated_accum(oracle, s, env, kw, part, g, 2).astype(np.float64) for g in range(3))
    want = full[0].astype(np.float64)
    assert np.all(np.abs(total[..., :3] - want[..., :3]) <= 1e-4 + 1e-4 * np.abs(want[..., :3]))
    assert np.abs(want[..., :3]).max() > 0.0


def test_cpu_seeds_cover_every_source_kind():
    import hala_renderer_amd as HR
    from random_scenes import random_scene
    types, emed, emap, has_env, has_sky = set(), False, False, False, False
    for seed in CPU_SEEDS:
        s, env, _ = random_scene(seed)
        types |= {L.light_type for L in s.lights}
        emed |= any(m.medium.type == HR.HalaMediumType.EMISSIVE for m in s.materials)
        emap |= any(m.emission_map_index != HR.scene.INVALID and max(m.emission) > 0 for m in s.materials)
        has_env |= env is not None
        has_sky |= env is None
    assert types == {0, 1, 2, 3, 4} and emed and emap and has_env and has_sky


def test_relight_twin_arithmetic():
    rs = np.random.RandomState(3)
    imgs = (rs.standard_normal((3, 5, 7, 4)) * 10).astype(f32)
    imgs[..., 3] = 1.0
    for g in range(3):  # one-hot scales: the image itself
        sc = np.zeros((3, 3), f32); sc[g] = 1.0
        assert R.relight(imgs, sc)[..., :3].tobytes() == imgs[g][..., :3].tobytes()
    sc = rs.uniform(-2.0, 3.0, (3, 3)).astype(f32)
    want = np.zeros((5, 7, 3), f32)
    for g in range(3):  # ascending, from 0, one rounding per product and per sum
        want = want + sc[g] * imgs[g][..., :3]
    got = R.relight(imgs, sc)
    assert got[..., :3].tobytes() == want.tobytes() and np.all(got[..., 3] == 1.0)
    assert np.all(R.relight(imgs, np.zeros((3, 3), f32))[..., :3] == 0.0)
    # float32 arithmetic: not the float64 sum
    big = np.array([[[[1e8, 0, 0, 1]]], [[[1.0, 0, 0, 1]]], [[[-1e8, 0, 0, 1]]]], f32)
    assert R.relight(big, np.ones((3, 3), f32))[0, 0, 0] == 0.0


# ---- GPU tier ----------------------------------------------------------------------------------------------------------------------
def assert_same(got, want, what):
    if got.tobytes() != want.tobytes():
        bad = np.any(got.reshape(-1, 4) != want.reshape(-1, 4), axis=-1)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} pixels differ")


def make(halart, scene, kw, env=None, part=None, groups=None, instances=False, aovs=True):
    r = halart.HalaRenderer("lgroups", kw["width"], kw["height"], kw["max_depth"], kw["rr_depth"], *kw["tonemap"], 0)
    if instances:
        r.set_build_options(instancing=True)
    if env is not None:
        r.set_envmap(env, kw["env_rotation"])
    r.set_env_intensity(kw["env_intensity"])
    r.set_exposure_value(kw["exposure"])
    r.set_scene(scene)
    r.commit()
    if aovs:
        r.set_aovs(True, True)
    if part is not None:
        lg, mg, eg = part
        r.set_light_groups(lights=lg, environment=eg, materials=mg, group_count=groups)
    return r


def scene_kw(w=W, h=H, md=5, rr=3, tm=(False, False, False), env_rotation=0.0, env_intensity=1.0, exposure=1.0):
    return dict(width=w, height=h, max_depth=md, rr_depth=rr, tonemap=tm, env_rotation=env_rotation, env_intensity=env_intensity, exposure=exposure)


def check_groups(oracle, r, scene, env, kw, part, groups, frames, what, view=0):
    out = []
    for g in range(groups):
        want = isolated_accum(oracle, scene, env, kw, part, g, frames)
        got = r.read_light_group(g, view=view)
        assert_same(got, want, f"{what}: group {g}")
        out.append(got)
    return out


def all_images(r):
    return [r.read_image(k) for k in range(6)]


@gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_random_scenes(halart, oracle, seed):
    from random_scenes import random_scene
    s, env, kw = random_scene(seed)
    lights, _ = oracle.pack_lights(s)
    G = 2 + seed % 3
    part = R.random_partition(np.random.RandomState(seed + 1), len(lights), len(s.materials), G)
    r, off = make(halart, s, kw, env, part, G), make(halart, s, kw, env)
    try:
        for frames in (1, 2):
            r.update_batch(frames); off.update_batch(frames)
        check_groups(oracle, r, s, env, kw, part, G, 3, f"seed {seed}")
        for k, (a, b) in enumerate(zip(all_images(r), all_images(off))):
            assert_same(a, b, f"seed {seed}: image {k} with groups on")
        assert r.statistics().rays_total == off.statistics().rays_total
    finally:
        r.close(); off.close()


def cornell_part(oracle, scene):
    """the quad light, the emissive fixture and everything else (with the sky): three groups"""
    lights, _ = oracle.pack_lights(scene)
    emissive = [m for m, M in enumerate(scene.materials) if max(M.emission) > 0.0]
    assert len(lights) >= 1 and emissive
    return [0] * len(lights), [1 if m in emissive else 2 for m in range(len(scene.materials))], 2


@gpu
def test_cornell_box_simple_kernels(halart, oracle):
    scene = scenes.cornell_box(aspect=W / H)
    kw = scene_kw()
    part = cornell_part(oracle, scene)
    r, off = make(halart, scene, kw, part=part), make(halart, scene, kw)
    try:
        assert r.bvh_info().lds_node_count > 0
        for _ in range(3):
            r.update(); off.update()
        imgs = check_groups(oracle, r, scene, None, kw, part, 3, 3, "cornell")
        assert all(np.abs(i[..., :3]).max() > 0.0 for i in imgs[:2])
        for k, (a, b) in enumerate(zip(all_images(r), all_images(off))):
            assert_same(a, b, f"cornell: image {k} with groups on")
    finally:
        r.close(); off.close()


def textured_scene(w=W, h=H, cameras=1):
    s = scenes.bunny_class(subdivisions=4, aspect=w / h, disney=True)
    scenes.attach_textures(s, sets=1, size=64)
    if cameras > 1:
        s = scenes.with_extra_cameras(s, cameras - 1)
    return s, scenes.sky_sun_envmap(128, 64, sun_gain=300.0)


def textured_kw():
    return scene_kw(md=4, rr=2, tm=(True, True, False), env_rotation=40.0, exposure=1.5)


def textured_part(s, lights):
    return [k % 2 for k in range(lights)], [1 + (m % 2) for m in range(len(s.materials))], 0


@gpu
def test_textured_disney_scene(halart, oracle):
    s, env = textured_scene()
    kw = textured_kw()
    part = textured_part(s, len(oracle.pack_lights(s)[0]))
    r = make(halart, s, kw, env, part, 3)
    try:
        assert r.bvh_info().lds_node_count == 0
        for _ in range(2):
            r.update()
        check_groups(oracle, r, s, env, kw, part, 3, 2, "textured")
    finally:
        r.close()


@gpu
@pytest.mark.parametrize("seed", [9, 17])
def test_two_level_trees(halart, oracle, seed):
    from random_scenes import random_scene
    oracle.set_instancing(True)
    try:
        s, env, kw = random_scene(seed, instances=True)
        lights, _ = oracle.pack_lights(s)
        part = R.random_partition(np.random.RandomState(seed), len(lights), len(s.materials), 3)
        r = make(halart, s, kw, env, part, 3, instances=True)
        try:
            assert r.bvh_info().instance_ref_count > 0
            r.update(); r.update()
            check_groups(oracle, r, s, env, kw, part, 3, 2, f"two-level seed {seed}")
        finally:
            r.close()
    finally:
        oracle.set_instancing(False)


@gpu
def test_update_batch_equals_single_updates(halart):
    s, env = textured_scene()
    kw = textured_kw()
    out = []
    for batched in (True, False):
        r = make(halart, s, kw, env)
        try:
            r.set_light_groups(lights=[k % 2 for k in range(len(r.packed_lights()[0]))], environment=1, materials=2)
            if batched:
                r.update_batch(5)
            else:
                for _ in range(5):
                    r.update()
            out.append([r.read_light_group(g) for g in range(3)] + all_images(r))
        finally:
            r.close()
    for k, (a, b) in enumerate(zip(*out)):
        assert_same(a, b, f"output {k}")


@gpu
def test_views_equal_the_swapped_scenes(halart, oracle):
    views = [2, 0, 1]
    scene = scenes.with_extra_cameras(scenes.cornell_box(aspect=W / H), 2)
    kw = scene_kw()
    part = cornell_part(oracle, scene)
    r = make(halart, scene, kw, part=part)
    try:
        r.set_views(views)
        r.update(); r.update_batch(2)
        for v, c in enumerate(views):
            check_groups(oracle, r, scenes.swap_cameras(scene, c), None, kw, part, 3, 3, f"view {v} (camera {c})", view=v)
    finally:
        r.close()


@gpu
def test_adaptive_sampling(halart, oracle):
    scene = scenes.cornell_box(aspect=W / H)
    kw = scene_kw()
    part = cornell_part(oracle, scene)
    r = make(halart, scene, kw)
    off = make(halart, scene, kw)
    try:
        for x in (r, off):
            x.set_adaptive_sampling(0.2, min_samples=2, interval=2)
        r.set_light_groups(lights=part[0], environment=part[2], materials=part[1])
        frames, snap = 0, None
        for batch in (2, 2, 2, 3, 3):
            r.update_batch(batch); off.update_batch(batch)
            frames += batch
            counts = r.read_sample_counts()
            imgs = [r.read_light_group(g) for g in range(3)]
            if snap is not None:  # pixels of blocks that had converged before this batch keep their group images
                done = snap[0] < frames - batch
                for a, b in zip(imgs, snap[1]):
                    assert np.array_equal(a[done], b[done])
            snap = (counts, imgs)
        counts = r.read_sample_counts()
        assert counts.min() < frames, "no block converged"
        assert np.array_equal(counts, off.read_sample_counts())
        for k, (a, b) in enumerate(zip(all_images(r), all_images(off))):
            assert_same(a, b, f"adaptive image {k}")
        for g in range(3):  # each pixel: the isolated render at that pixel's own sample count
            for n in np.unique(counts):
                want = isolated_accum(oracle, scene, None, kw, part, g, int(n))
                sel = counts == n
                assert np.array_equal(snap[1][g][sel], want[sel]), (g, n)
    finally:
        r.close(); off.close()


def play(halart, timing_period, fusion):
    s, env = textured_scene()
    kw = textured_kw()
    out = []
    r = make(halart, s, kw, env)
    try:
        r.set_pass_fusion(fusion)
        r.set_launch_timing_period(timing_period)
        n = len(r.packed_lights()[0])
        r.set_light_groups(lights=[k % 2 for k in range(n)], environment=1, materials=2)
        for frames in (1, 2, 1):
            r.update_batch(frames)
            r.render()
            out += [r.read_light_group(g) for g in range(3)]
        out += all_images(r)
        out += list(r.relight([(1.0, 0.5, 0.25), 2.0, (0.0, 1.0, -1.0)]))
    finally:
        r.close()
    return out


@gpu
def test_pass_fusion_and_tail_overlap(halart):
    ref = play(halart, 1, 0)  # serial: timed updates, one launch per pass
    for period, fusion in ((0, 1), (0, 2), (1, 2)):
        got = play(halart, period, fusion)
        assert len(got) == len(ref)
        for i, (a, b) in enumerate(zip(got, ref)):
            assert a.tobytes() == b.tobytes(), (period, fusion, i)


@gpu
def test_relight(halart, oracle):
    from random_scenes import random_scene
    s, env, kw = random_scene(17)
    kw = dict(kw, tonemap=(True, True, False), exposure=1.7)
    lights, _ = oracle.pack_lights(s)
    part = R.random_partition(np.random.RandomState(4), len(lights), len(s.materials), 3)
    r = make(halart, s, kw, env, part, 3)
    try:
        r.update_batch(3)
        imgs = np.stack([r.read_light_group(g) for g in range(3)])
        for g in range(3):  # one-hot: the group image itself
            sc = np.zeros((3, 3), f32); sc[g] = 1.0
            lin, _ = r.relight(sc)
            assert_same(lin[..., :3].copy(), imgs[g][..., :3].copy(), f"one-hot {g}")
        sc = np.random.RandomState(1).uniform(-1.0, 4.0, (3, 3)).astype(f32)
        lin, tm = r.relight(sc)
        assert_same(lin, R.relight(imgs, sc), "arbitrary scales")
        want_tm = oracle.tonemap_pixels((lin * f32(kw["exposure"])).astype(f32), *kw["tonemap"])
        assert np.array_equal(tm[..., :3], want_tm[..., :3]) and np.all(tm[..., 3] == 1.0)
        ptr, nbytes = r.relit_buffer(1)
        assert ptr and nbytes == kw["width"] * kw["height"] * 16
        lin1, _ = r.relight(np.ones((3, 3), f32))
        accum = r.read_image(0)
        assert np.allclose(lin1[..., :3], accum[..., :3], rtol=1e-5, atol=1e-5)
    finally:
        r.close()


@gpu
def test_refusals_leave_the_renderer_as_it_was(halart, oracle):
    scene = scenes.cornell_box(aspect=W / H)
    kw = scene_kw()
    r = make(halart, scene, kw, aovs=False)
    lib = halart.load_library()
    try:
        def frame(n=2):
            r.reset_accumulation()
            r.update_batch(n)
            return [r.read_image(k).tobytes() for k in range(4)]

        before = frame()
        for kwargs in (dict(group_count=0), dict(group_count=9), dict(env=3, group_count=2), dict(lights=(0, 2))):
            g, keep = descriptor(halart, **kwargs)
            with pytest.raises(halart.HalaRendererError):
                halart.check(lib.hala_rt_set_light_groups(r._h, C.byref(g)))
        with pytest.raises(halart.HalaRendererError, match="off"):
            r.read_light_group(0)
        with pytest.raises(halart.HalaRendererError, match="off"):
            r.relight([1.0])
        with pytest.raises(halart.HalaRendererError, match="Nothing relit"):
            r.relit_buffer(0)
        assert frame() == before
        part = cornell_part(oracle, scene)
        r.set_light_groups(lights=part[0], environment=part[2], materials=part[1])
        r.update_batch(2)
        assert r.statistics().total_frames == 2
        with pytest.raises(halart.HalaRendererError, match="does not exist"):
            r.read_light_group(3)
        with pytest.raises(halart.HalaRendererError, match="does not exist"):
            r.read_light_group(0, view=1)
        with pytest.raises(halart.HalaRendererError, match="group_count"):
            r.relight([1.0, 1.0])
        with pytest.raises(halart.HalaRendererError, match="finite"):
            r.relight([1.0, float("inf"), 1.0])
        with pytest.raises(halart.HalaRendererError, match="sharded"):
            r.set_tile_shard(0, 2, 16)
        assert r.statistics().total_frames == 2
        g0 = r.read_light_group(0)
        # an update whose scene has more materials than the tables cover fails before any device work
        r.set_light_groups(lights=part[0], environment=part[2], materials=part[1][:-1], group_count=3)
        with pytest.raises(halart.HalaRendererError, match="light groups cover"):
            r.update()
        r.set_light_groups(lights=part[0], environment=part[2], materials=part[1])
        assert r.statistics().total_frames == 0
        r.update_batch(2)
        assert_same(r.read_light_group(0), g0, "group 0 after the refusals")
        assert [r.read_image(k).tobytes() for k in range(4)] == before
        r.set_light_groups()
        with pytest.raises(halart.HalaRendererError, match="off"):
            r.read_light_group(0)
        assert frame() == before
        # a sharded renderer refuses the groups
        r.set_tile_shard(0, 2, 16)
        with pytest.raises(halart.HalaRendererError, match="sharded"):
            r.set_light_groups(lights=part[0], environment=part[2], materials=part[1])
    finally:
        r.close()
