"""First-hit AOVs (docs/RENDER_SPEC.md 13): image 4 `position` (running mean of (P, hit)) and image 5 `ids` (node, instance, material,
triangle id of frame 0's first hit).  CPU tier: the exact fma emulation of the numpy reference, the light twin and the instance / node /
material tables against the oracle, the header.  GPU tier: the AOVs against the numpy reference on the oracle's camera rays and hits, bit
for bit, with images 0-3 unchanged by the feature — the SIMPLE kernels, random scenes (opacity, media, every light type, thin-lens and
orthographic cameras, env map, textures), a textured Disney scene, two-level trees, batches, views, tile shards, adaptive sampling, the
tail overlap and the refusals."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import aov_ref as R
from conftest import ROOT
from hala_renderer_amd import scenes

gpu = pytest.mark.gpu
W, H = 61, 37
f32 = np.float32
SEEDS = [17, 25, 20, 12, 22]  # between them: lights of all five types, opacity, media, thin lens, orthographic, env map, textures


def exact_fma(a, b, c):
    x = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    # round the exact rational to the nearest float32 (ties to even) by bracketing it between neighbours
    lo = f32(float(x))
    while Fraction(float(lo)) > x:
        lo = np.nextafter(lo, f32(-np.inf))
    while Fraction(float(np.nextafter(lo, f32(np.inf)))) <= x:
        lo = np.nextafter(lo, f32(np.inf))
    hi = np.nextafter(lo, f32(np.inf))
    if Fraction(float(lo)) == x:
        return lo
    dl, dh = x - Fraction(float(lo)), Fraction(float(hi)) - x
    if dl != dh:
        return lo if dl < dh else hi
    return lo if (int(np.array(lo).view(np.uint32)) & 1) == 0 else hi


# ---- CPU tier ----------------------------------------------------------------------------------------------------------------------
def test_fma_emulation_is_exactly_rounded():
    rs = np.random.RandomState(5)
    a = (rs.standard_normal(3000) * np.exp2(rs.randint(-20, 20, 3000))).astype(f32)
    b = (rs.standard_normal(3000) * np.exp2(rs.randint(-20, 20, 3000))).astype(f32)
    c = (-(a.astype(np.float64) * b) * (1.0 + rs.standard_normal(3000) * 1e-6)).astype(f32)  # heavy cancellation half the time
    c[::2] = (rs.standard_normal(1500) * np.exp2(rs.randint(-30, 30, 1500))).astype(f32)
    got = R.fma(a, b, c)
    for i in range(a.size):
        assert got[i] == exact_fma(a[i], b[i], c[i]), (a[i], b[i], c[i])
    # built midpoints: a*b + c lies just off the half-way point between two float32 by a tail (2^-70) that a float64 sum drops; a
    # float64 sum followed by a float32 rounding (double rounding) then rounds the wrong way, round-to-odd does not
    def double_rounded(a, b, c):
        return f32(float(a) * float(b) + float(c))
    a1 = f32(1.0 + 2.0 ** -23)
    for k in range(64):
        m = f32(1.0 + (2 * k + 1) * 2.0 ** -23)  # odd significand
        for sb in (1.0, -1.0):
            for sc in (1.0, -1.0):
                b1, c1 = f32(sb * (2.0 ** -24 - 2.0 ** -47)), f32(sc * float(m))
                want = exact_fma(a1, b1, c1)
                assert want == c1
                assert R.fma(a1, b1, c1) == want, (k, sb, sc)
                assert double_rounded(a1, b1, c1) != want  # the case is a real one


@pytest.mark.parametrize("seed", [3, 9, 10, 17, 19, 20, 25])
def test_light_twin_and_tables_agree_with_the_oracle(oracle, seed):
    from random_scenes import random_scene
    s, env, kw = random_scene(seed, instances=True)
    w, h = kw["width"], kw["height"]
    lights, _ = oracle.pack_lights(s)
    lnode = R.light_nodes(s)
    assert len(lnode) == len(lights)
    for k, L in enumerate(lights):
        d = s.lights[s.nodes[lnode[k]].light_index]
        assert L.type == d.light_type
        assert np.array_equal(np.array(L.intensity[:3], f32), (np.array(d.color, f32) * f32(d.intensity)).astype(f32))
    world = oracle.world_transforms(s)
    inst_node, inst_mat, first = R.instance_table(s)
    xf, md = oracle.pack_instances(s)
    assert len(md) == len(inst_node) and int(first[-1]) == oracle.OracleScene(s).triangle_count
    for i, m in enumerate(md):
        assert m.material_index == inst_mat[i]
        assert np.array_equal(np.array(m.transform[:16], f32), world[inst_node[i]])
    # the light twin classifies every camera ray of frame 0 like the oracle's depth-0 shade: a light hit leaves normal 0 and albedo
    # min(intensity, 1) of that light, a triangle hit a unit normal
    osc = oracle.OracleScene(s, envmap=env)
    pos, ids = R.first_hits(osc, s, lights, w, h, 0)
    imgs, _ = osc.render(w, h, frames=1, max_depth=1, rr_depth=1, env_rotation=kw["env_rotation"] if env is not None else 0.0)
    albedo, normal = imgs[1], imgs[2]
    is_light = (ids[..., 3] != R.ABSENT) & ((ids[..., 3] & 0x80000000) != 0)
    is_tri = (ids[..., 3] != R.ABSENT) & ~is_light
    assert np.all(normal[is_light][:, :3] == 0.0)
    for k, L in enumerate(lights):
        sel = is_light & ((ids[..., 3] & 0x7FFFFFFF) == k)
        assert np.all(albedo[sel][:, :3] == np.minimum(np.array(L.intensity[:3], f32), f32(1.0)))
    assert np.all(np.abs(np.linalg.norm(normal[is_tri][:, :3], axis=-1) - 1.0) < 1e-3)
    assert np.all(pos[~(is_light | is_tri)] == 0.0) and np.all(pos[is_light | is_tri][:, 3] == 1.0)
    osc.close()


def test_light_twin_sees_quads_and_spheres(oracle):
    """the scenes of the GPU tier hit QUAD and SPHERE lights with camera rays, and the Cornell box hits its quad light"""
    from random_scenes import random_scene
    seen = set()
    for s, w, h in [(lambda t: (t[0], t[2]["width"], t[2]["height"]))(random_scene(seed)) for seed in SEEDS] + [(scenes.cornell_box(aspect=W / H), W, H)]:
        lights, _ = oracle.pack_lights(s)
        osc = oracle.OracleScene(s)
        _, ids = R.first_hits(osc, s, lights, w, h, 0)
        osc.close()
        hit = ids[..., 3][(ids[..., 3] != R.ABSENT) & ((ids[..., 3] & 0x80000000) != 0)] & 0x7FFFFFFF
        seen |= {lights[int(k)].type for k in np.unique(hit)}
    assert {3, 4} <= seen


def test_header_declares_set_aovs():
    text = open(os.path.join(ROOT, "include", "halart.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int hala_rt_set_aovs\(hala_rt_renderer\* r, uint32_t mask\);", text, flags=re.S)
    assert m
    for w in ("RENDER_SPEC.md 13", "position", "ids", "restarts the accumulation", "save_images"):
        assert w in m.group(1), w


def test_view_depth_helper():
    from hala_renderer_amd import _abi as A, view_depth
    cam = A.GpuCamera()
    cam.position[:] = (1.0, 2.0, 3.0)
    cam.forward[:] = (0.0, 0.0, -2.0)
    pos = np.zeros((2, 2, 4), f32)
    pos[0, 0] = (1.0, 2.0, -2.0, 1.0)          # 5 in front
    pos[0, 1] = (0.5 * 4.0, 0.0, 0.5 * 1.0, 0.5)  # half coverage: mean point (4, 0, 1), 2 in front
    d = view_depth(pos, cam)
    assert d[0, 0] == 5.0 and d[0, 1] == 2.0 and np.isinf(d[1, 0]) and np.isinf(d[1, 1])


# ---- GPU tier ----------------------------------------------------------------------------------------------------------------------
def assert_same(got, want, what):
    if got.tobytes() != want.tobytes():
        bad = np.any(got.reshape(-1, 4) != want.reshape(-1, 4), axis=-1)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} pixels differ")


def make(halart, scene, w=W, h=H, env=None, md=5, rr=3, tm=(False, False, False), aovs=(True, True), build=None, shard=None, env_rot=0.0):
    r = halart.HalaRenderer("aovs", w, h, md, rr, *tm, 0)
    if build is not None:
        r.set_build_options(**build)
    if shard is not None:
        r.set_tile_shard(*shard)
    if env is not None:
        r.set_envmap(env, env_rot)
    r.set_scene(scene)
    r.commit()
    if aovs is not None:
        r.set_aovs(*aovs)
    return r


def images(r, view=0):
    return [r.read_image(k, view=view) for k in range(4)]


def check(oracle, r, off, scene, w, h, frames, what, env=None):
    lights, _ = oracle.pack_lights(scene)
    osc = oracle.OracleScene(scene, envmap=env)
    pos, ids = R.reference(osc, scene, lights, w, h, frames)
    osc.close()
    assert_same(r.read_image("position"), pos, f"{what}: position")
    assert_same(r.read_ids(), ids, f"{what}: ids")
    if off is not None:
        for k, (a, b) in enumerate(zip(images(r), images(off))):
            assert_same(a, b, f"{what}: image {k} with the AOVs on")
    return pos, ids


@gpu
def test_cornell_box_simple_kernels(halart, oracle):
    scene = scenes.cornell_box(aspect=W / H)
    r, off = make(halart, scene), make(halart, scene, aovs=None)
    try:
        assert r.bvh_info().lds_node_count > 0
        r.update(); off.update()
        check(oracle, r, off, scene, W, H, 1, "cornell x1")
        for _ in range(4):
            r.update(); off.update()
        pos, ids = check(oracle, r, off, scene, W, H, 5, "cornell x5")
        assert np.any((ids[..., 3] & 0x80000000) != 0) and np.any(ids[..., 3] < 0x80000000)  # the quad light and triangles
    finally:
        r.close(); off.close()


def random_renderer(halart, seed, instances=False, aovs=(True, True)):
    from random_scenes import random_scene
    s, env, kw = random_scene(seed, instances=instances)
    r = halart.HalaRenderer("aovs", kw["width"], kw["height"], kw["max_depth"], kw["rr_depth"], *kw["tonemap"], 0)
    if instances:
        r.set_build_options(instancing=True)
    if env is not None:
        r.set_envmap(env, kw["env_rotation"])
        r.set_env_intensity(kw["env_intensity"])
    r.set_exposure_value(kw["exposure"])
    r.set_scene(s)
    r.commit()
    if aovs is not None:
        r.set_aovs(*aovs)
    return r, s, env, kw


@gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_random_scenes(halart, oracle, seed):
    r, s, env, kw = random_renderer(halart, seed)
    off = random_renderer(halart, seed, aovs=None)[0]
    try:
        for frames in (1, 2):
            r.update_batch(frames); off.update_batch(frames)
        check(oracle, r, off, s, kw["width"], kw["height"], 3, f"seed {seed}", env)
    finally:
        r.close(); off.close()


def textured_scene(w=W, h=H, cameras=1):
    s = scenes.bunny_class(subdivisions=4, aspect=w / h, disney=True)
    scenes.attach_textures(s, sets=1, size=64)
    if cameras > 1:
        s = scenes.with_extra_cameras(s, cameras - 1)
    return s, scenes.sky_sun_envmap(128, 64, sun_gain=300.0)


@gpu
def test_textured_disney_scene(halart, oracle):
    s, env = textured_scene()
    r = make(halart, s, env=env, md=4, rr=2, tm=(True, True, False), env_rot=40.0)
    off = make(halart, s, env=env, md=4, rr=2, tm=(True, True, False), env_rot=40.0, aovs=None)
    try:
        assert r.bvh_info().lds_node_count == 0
        for _ in range(3):
            r.update(); off.update()
        check(oracle, r, off, s, W, H, 3, "textured")
    finally:
        r.close(); off.close()


@gpu
@pytest.mark.parametrize("seed", [9, 17])
def test_two_level_trees(halart, oracle, seed):
    oracle.set_instancing(True)
    try:
        r, s, env, kw = random_renderer(halart, seed, instances=True)
        off = random_renderer(halart, seed, instances=True, aovs=None)[0]
        try:
            assert r.bvh_info().instance_ref_count > 0
            r.update(); r.update(); off.update(); off.update()
            _, ids = check(oracle, r, off, s, kw["width"], kw["height"], 2, f"two-level seed {seed}", env)
            inst = ids[..., 1][(ids[..., 3] & 0x80000000) == 0]
            assert len(np.unique(inst)) >= 2
        finally:
            r.close(); off.close()
    finally:
        oracle.set_instancing(False)


@gpu
def test_update_batch_equals_single_updates(halart):
    s, env = textured_scene()
    out = []
    for batched in (True, False):
        r = make(halart, s, env=env, md=4, rr=2, env_rot=40.0)
        try:
            if batched:
                r.update_batch(5)
            else:
                for _ in range(5):
                    r.update()
            out.append(images(r) + [r.read_image(4), r.read_image(5)])
        finally:
            r.close()
    for k in range(6):
        assert_same(out[0][k], out[1][k], f"image {k}")


@gpu
def test_views_equal_single_view_references(halart, oracle):
    views = [2, 0, 1, 2]
    scene = scenes.with_extra_cameras(scenes.cornell_box(aspect=W / H), 2)
    r = make(halart, scene)
    try:
        r.set_views(views)
        r.update(); r.update_batch(2)
        for v, c in enumerate(views):
            sw = scenes.swap_cameras(scene, c)
            lights, _ = oracle.pack_lights(sw)
            osc = oracle.OracleScene(sw)
            pos, ids = R.reference(osc, sw, lights, W, H, 3)
            osc.close()
            assert_same(r.read_image(4, view=v), pos, f"view {v} position")
            assert_same(r.read_ids(view=v), ids, f"view {v} ids")
    finally:
        r.close()


@gpu
@pytest.mark.parametrize("world,ts", [(2, 16), (3, 12)])
def test_tile_shards_gathered(halart, world, ts):
    import torch
    from hala_renderer_amd.dist import _DeviceView
    s, env = textured_scene()
    full = make(halart, s, env=env, md=4, rr=2, env_rot=40.0)
    ranks = [make(halart, s, env=env, md=4, rr=2, env_rot=40.0, shard=(k, world, ts)) for k in range(world)]
    try:
        for r in [full] + ranks:
            r.update(); r.update()
        with pytest.raises(halart.HalaRendererError):
            ranks[0].read_image(4)  # sharded: gather first
        aovs = (0, 4, 5)
        for r in ranks:
            r.tile_allgather_begin_external(aovs)
        me = ranks[-1]
        for which in aovs:
            _, sn, rp, rn, stream = me.exchange_buffers(which)
            assert rn == sn * world
            ext = torch.cuda.ExternalStream(stream, device="cuda:0")
            recv = torch.as_tensor(_DeviceView(rp, rn // 4), device="cuda:0")
            for k, r in enumerate(ranks):
                sp, sn_k, _, _, stream_k = r.exchange_buffers(which)
                torch.cuda.ExternalStream(stream_k, device="cuda:0").synchronize()
                staged = torch.as_tensor(_DeviceView(sp, sn_k // 4), device="cuda:0")
                with torch.cuda.stream(ext):
                    recv[k * (sn // 4):(k + 1) * (sn // 4)].copy_(staged)
        for r in ranks:
            r.tile_allgather_finish()
        for which in aovs:
            assert_same(me.read_image(which), full.read_image(which), f"world {world} image {which}")
        # the plain scatter entry point on a buffer gathered by hand
        for which in (4, 5):
            parts = []
            for r in ranks:
                r.wait_idle()
                ptr, nbytes = r.tile_buffer(which)
                parts.append(torch.as_tensor(_DeviceView(ptr, nbytes // 4), device="cuda:0").clone())
            g = torch.cat(parts).contiguous()
            ranks[0].scatter_gathered_tiles(which, g.data_ptr(), g.numel() * 4)
            torch.cuda.synchronize()
            assert_same(ranks[0].read_image(which), full.read_image(which), f"world {world} scatter {which}")
    finally:
        for r in [full] + ranks:
            r.close()


@gpu
def test_adaptive_sampling(halart, oracle):
    scene = scenes.cornell_box(aspect=W / H)
    r = make(halart, scene)
    off = make(halart, scene, aovs=None)
    try:
        for x in (r, off):
            x.set_adaptive_sampling(0.2, min_samples=2, interval=2)
        r.set_aovs(True, True)
        frames, snap = 0, None
        for batch in (2, 2, 2, 3, 3):
            r.update_batch(batch); off.update_batch(batch)
            frames += batch
            counts = r.read_sample_counts()
            pos, ids = r.read_image(4), r.read_ids()
            if snap is not None:  # pixels of blocks that had converged before this batch keep their AOVs
                done = snap[0] < frames - batch
                assert np.array_equal(pos[done], snap[1][done]) and np.array_equal(ids[done], snap[2][done])
            snap = (counts, pos, ids)
        counts = r.read_sample_counts()
        assert counts.min() < frames, "no block converged"
        assert counts.max() == frames
        assert np.array_equal(counts, off.read_sample_counts())
        for k, (a, b) in enumerate(zip(images(r), images(off))):
            assert_same(a, b, f"adaptive image {k}")
        lights, _ = oracle.pack_lights(scene)
        osc = oracle.OracleScene(scene)
        want_pos, want_ids = R.reference(osc, scene, lights, W, H, frames)
        # a converged pixel: the mean over its own samples
        done_pos, _ = R.reference(osc, scene, lights, W, H, int(counts.min()))
        osc.close()
        active = counts == frames
        assert np.array_equal(pos[active], want_pos[active])
        conv = counts == counts.min()
        assert np.array_equal(pos[conv], done_pos[conv])
        assert_same(ids, want_ids, "adaptive ids")
    finally:
        r.close(); off.close()


def play(halart, timing_period):
    s, env = textured_scene()
    out = []
    r = make(halart, s, env=env, md=4, rr=2, env_rot=40.0)
    try:
        r.set_launch_timing_period(timing_period)
        for frames in (1, 2, 1):
            r.update_batch(frames)
            r.render()
            out.append(r.read_image(4))
            out.append(r.read_image(5))
        r.set_aovs(position=True)
        r.update(); r.update()
        out += [r.read_image(k) for k in range(5)]
    finally:
        r.close()
    return out


@gpu
def test_tail_overlap(halart):
    overlapped, serial = play(halart, 0), play(halart, 1)
    assert len(overlapped) == len(serial)
    for i, (a, b) in enumerate(zip(overlapped, serial)):
        assert a.tobytes() == b.tobytes(), i


@gpu
def test_refusals_leave_the_renderer_as_it_was(halart):
    scene = scenes.cornell_box(aspect=W / H)
    r = make(halart, scene, aovs=None)
    lib = halart.load_library()
    try:
        def frame(n=2):
            r.reset_accumulation()
            r.update_batch(n)
            return [x.tobytes() for x in images(r)]

        before = frame()
        with pytest.raises(halart.HalaRendererError, match="unknown AOV bits"):
            halart.check(lib.hala_rt_set_aovs(r._h, C.c_uint32(4)))
        for which in (4, 5):
            with pytest.raises(halart.HalaRendererError, match="Invalid image selector"):
                r.read_image(which)
        with pytest.raises(halart.HalaRendererError, match="Invalid argument"):
            r.tile_buffer(4)
        with pytest.raises(halart.HalaRendererError, match="Invalid AOV mask"):
            r.tile_allgather_begin_external((0, 4))
        assert frame() == before
        # one AOV on: the other one is still refused; a set_aovs call restarts the accumulation
        r.set_aovs(position=True)
        with pytest.raises(halart.HalaRendererError, match="Invalid image selector"):
            r.read_image(5)
        with pytest.raises(halart.HalaRendererError, match="Invalid AOV mask"):
            r.tile_allgather_begin_external((5,))
        r.update_batch(2)
        assert r.statistics().total_frames == 2
        with pytest.raises(halart.HalaRendererError, match="unknown AOV bits"):
            halart.check(lib.hala_rt_set_aovs(r._h, C.c_uint32(7)))
        assert r.statistics().total_frames == 2
        r.read_image(4)
        r.set_aovs(position=True, ids=True)
        assert r.statistics().total_frames == 0
        r.update_batch(2)
        assert [x.tobytes() for x in images(r)] == before
        r.set_aovs()
        with pytest.raises(halart.HalaRendererError, match="Invalid image selector"):
            r.read_image(4)
        assert frame() == before
    finally:
        r.close()
