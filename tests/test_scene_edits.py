"""Interactive scene edits (include/halart.h: hala_rt_update_node_transform / _update_vertices / _update_material + hala_rt_refit;
INTEGRATION.md §6) with every later feature on.  The catalogue of edits lives in tests/scene_edits.py.

CPU tier: every edit changes the oracle's image of its scene, the edit and its inverse give the original image back byte for byte, and an
edit changes only the packed records it names.  GPU tier: after refit the renderer equals the oracle of the EDITED scene rendered from
frame 0 (images, tree, ray batches), the inverse gives the original frame and tree back, an edit does nothing before its refit, and the
same holds with views, first-hit AOVs, light groups, adaptive sampling, tile shards and the tail overlap; refused edits change nothing."""
import contextlib

import numpy as np
import pytest

import adaptive_ref as AR
import aov_ref
import denoise_ref
import light_group_ref as LG
import hala_renderer_amd as H
import scene_edits as E
from hala_renderer_amd import scenes

gpu = pytest.mark.gpu
f32 = np.float32
CPU_FRAMES = 2


def oracle_images(oracle, base, scene, frames, first_frame=0, images=None, env_intensity=None):
    kw = base.kw
    osc = oracle.OracleScene(scene, envmap=base.env)
    imgs, st = osc.render(kw["width"], kw["height"], frames=frames, first_frame=first_frame, images=images, max_depth=kw["max_depth"],
                          rr_depth=kw["rr_depth"], tonemap=kw["tonemap"], env_rotation=kw["env_rotation"] if base.env is not None else 0.0,
                          env_intensity=(kw["env_intensity"] if base.env is not None else 1.0) if env_intensity is None else env_intensity,
                          exposure=kw["exposure"])
    osc.close()
    return imgs


def packed(oracle, scene):
    """the packed records of a scene, by kind, as bytes"""
    lights, boxes = oracle.pack_lights(scene)
    t, md = oracle.pack_instances(scene)
    return {"cameras": b"".join(bytes(c) for c in oracle.pack_cameras(scene)),
            "lights": b"".join(bytes(x) for x in lights) + b"".join(bytes(x) for x in boxes),
            "instances": t.tobytes(),
            "materials": b"".join(bytes(oracle.pack_material(m)) for m in scene.materials),
            "vertices": b"".join(p.vertices.tobytes() for m in scene.meshes for p in m.primitives)}


_BASES = {}


def base_of(name):
    if name not in _BASES:
        _BASES[name] = E.BASES[name]()
    return _BASES[name]


def case_id(c):
    return f"{c[0]}-{c[1]}"


# ---- CPU tier -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.CASES, ids=case_id)
def test_edit_changes_the_oracle_image_and_its_inverse_restores_it(oracle, case):
    base = base_of(case[0])
    fwd, inv = E.edit_ops(case[1], base.scene)
    cam = E.EDITS[case[1]].camera  # (render that camera: the oracle renders camera 0)
    before = oracle_images(oracle, base, scenes.swap_cameras(base.scene, cam), CPU_FRAMES)
    edited = E.apply_to_scene(base.scene, fwd)
    after = oracle_images(oracle, base, scenes.swap_cameras(edited, cam), CPU_FRAMES)
    changed = int(np.any(after[0] != before[0], axis=-1).sum())
    assert changed > 0, f"{case}: the edit leaves the oracle's image as it was"
    back = oracle_images(oracle, base, scenes.swap_cameras(E.apply_to_scene(edited, inv), cam), CPU_FRAMES)
    for k in range(4):
        assert back[k].tobytes() == before[k].tobytes(), f"{case}: image {k} after the inverse"


@pytest.mark.parametrize("case", E.CASES, ids=case_id)
def test_edit_touches_only_what_it_names(oracle, case):
    base = base_of(case[0])
    fwd, inv = E.edit_ops(case[1], base.scene)
    want = E.EDITS[case[1]].touches
    before = packed(oracle, base.scene)
    edited = E.apply_to_scene(base.scene, fwd)
    after = packed(oracle, edited)
    changed = {k for k in before if before[k] != after[k]}
    assert changed == set(want), (case, changed, want)
    assert packed(oracle, E.apply_to_scene(edited, inv)) == before
    assert packed(oracle, base.scene) == before  # apply_to_scene works on a copy


def test_header_documents_the_edit_contract():
    import os
    import re

    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "halart.h")).read()
    for fn, words in (("hala_rt_update_node_transform", ("committed scene", "next hala_rt_refit", "refused call changes nothing")),
                      ("hala_rt_update_vertices", ("Takes effect at the next hala_rt_refit",)),
                      ("hala_rt_refit", ("restarts", "views", "light-group", "adaptive", "hala_rt_read_denoised"))):
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int " + fn + r"\(", text, flags=re.S)
        assert m, fn
        for w in words:
            assert w in re.sub(r"\s*\n \*\s*", " ", m.group(1)), (fn, w)


def test_catalogue_covers_the_issue_list():
    ids = {e.split("-")[0] for e in E.EDITS}
    assert ids == {f"E{k}" for k in range(1, 10)}
    assert {c[1] for c in E.CASES} == set(E.EDITS)


# ---- GPU tier -----------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def tree_form(oracle, two_level):
    """RENDER_SPEC 4.5 on both sides while inside: oracle scenes created here intersect instanced primitives in object space"""
    oracle.set_instancing(bool(two_level))
    try:
        yield dict(instancing=True) if two_level else None
    finally:
        oracle.set_instancing(False)


def make(halart, base, scene=None, build=None, shard=None):
    kw = base.kw
    r = halart.HalaRenderer("edits", kw["width"], kw["height"], kw["max_depth"], kw["rr_depth"], *kw["tonemap"], 0)
    if build is not None:
        r.set_build_options(**build)
    if shard is not None:
        r.set_tile_shard(*shard)
    if base.env is not None:
        r.set_envmap(base.env, kw["env_rotation"])
        r.set_env_intensity(kw["env_intensity"])
    r.set_exposure_value(kw["exposure"])
    r.set_scene(base.scene if scene is None else scene)
    r.commit()
    return r


def assert_same(got, want, what):
    if got.tobytes() != want.tobytes():
        bad = np.any(got.reshape(-1, 4) != want.reshape(-1, 4), axis=-1) if got.shape[-1:] == (4,) else got != want
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} values differ")


def assert_images(r, want, what, view=0):
    for k in range(4):
        assert_same(r.read_image(k, view=view), want[k], f"{what}: image {k}")


def validate_tree(oracle, osc, r):
    nodes, tris = r.download_bvh()
    refs = r.download_instance_refs()
    if len(refs):
        return oracle.validate_bvh_two_level(osc, nodes, tris, refs)[0]
    return oracle.validate_bvh(nodes, tris, osc.triangles())[0]


def rays_of(osc, base):
    from test_oracle_render import random_rays
    mn, mx = osc.bounds()
    pad = (mx - mn) * 0.2
    return np.concatenate([osc.camera_rays(base.kw["width"] * 2, base.kw["height"] * 2, 0), random_rays(3000, mn - pad, mx + pad, 5)])


def matrix_cases():
    out = []
    for b, e in E.CASES:
        out.append((b, e, False))
        if E.EDITS[e].two_level and E.shared_mesh(base_of(b).scene) is not None:
            out.append((b, e, True))
    return out


@gpu
@pytest.mark.parametrize("case", matrix_cases(), ids=lambda c: f"{c[0]}-{c[1]}-{'two_level' if c[2] else 'one_level'}")
def test_edit_refit_equals_the_oracle_of_the_edited_scene(halart, oracle, case):
    """an accumulation under way, then the edit + refit: images 0-3 of update_batch(2) + update() equal the oracle's render of the edited
    scene from frame 0, the tree passes the structural check, closest-hit and any-hit ray batches equal the oracle's; the inverse edit +
    refit gives the original frame back, and the original tree bytes when the tree form did not change"""
    b, e, two_level = case
    base = base_of(b)
    fwd, inv = E.edit_ops(e, base.scene)
    edited = E.apply_to_scene(base.scene, fwd)
    with tree_form(oracle, two_level) as build:
        r = make(halart, base, build=build)
        try:
            assert (r.bvh_info().instance_ref_count > 0) == two_level
            n0, t0 = r.download_bvh()
            refs0 = r.download_instance_refs()
            r.update_batch(2); r.render()
            E.apply_to_renderer(r, fwd)
            r.refit()
            r.update_batch(2); r.update(); r.render()
            assert_images(r, oracle_images(oracle, base, edited, 3), f"{case} after the refit")
            assert r.statistics().total_frames == 3
            osc = oracle.OracleScene(edited, envmap=base.env)
            assert validate_tree(oracle, osc, r) == 0
            rays = rays_of(osc, base)
            for mode in (0, 1):
                assert r.trace_rays_host(rays, mode).tobytes() == osc.trace(rays, mode).tobytes(), (case, mode)
            osc.close()
            E.apply_to_renderer(r, inv)
            r.refit()
            r.update_batch(3); r.render()
            assert_images(r, oracle_images(oracle, base, base.scene, 3), f"{case} after the inverse")
            n1, t1 = r.download_bvh()
            assert n1.tobytes() == n0.tobytes() and t1.tobytes() == t0.tobytes(), f"{case}: the tree after the inverse"
            assert r.download_instance_refs().tobytes() == refs0.tobytes()
        finally:
            r.close()


@gpu
@pytest.mark.parametrize("case", [("cornell", e, False) for e in E.EDITS] + [("cornell", "E4-deform-shared", True), ("cornell", "E9-singular", True)],
                         ids=lambda c: f"{c[1]}-{'two_level' if c[2] else 'one_level'}")
def test_edit_takes_effect_at_the_refit(halart, oracle, case):
    """between an edit and its refit, updates render the unedited scene and continue its accumulation (the header: "takes effect at the
    next hala_rt_refit" — for E4 also after update_vertices has copied the vertices to the device); the refit then applies it"""
    b, e, two_level = case
    base = base_of(b)
    fwd, _ = E.edit_ops(e, base.scene)
    with tree_form(oracle, two_level) as build:
        r = make(halart, base, build=build)
        try:
            r.update_batch(2)
            E.apply_to_renderer(r, fwd)
            r.update(); r.update_batch(2); r.render()
            assert_images(r, oracle_images(oracle, base, base.scene, 5), f"{case} before the refit")
            assert r.statistics().total_frames == 5
            r.refit()
            r.update_batch(2)
            assert_images(r, oracle_images(oracle, base, E.apply_to_scene(base.scene, fwd), 2), f"{case} after the refit")
        finally:
            r.close()


VIEWS = [2, 0, 1]


@gpu
@pytest.mark.parametrize("edit", ["E1-move-mesh-node", "E2-move-lights", "E3-move-camera-1"])
def test_views_survive_the_refit(halart, oracle, edit):
    """set_views([2, 0, 1]) before the edit: after the refit view v equals the oracle of swap_cameras(edited scene, c_v) from frame 0,
    without set_views being called again"""
    base = base_of("cornell")
    fwd, _ = E.edit_ops(edit, base.scene)
    edited = E.apply_to_scene(base.scene, fwd)
    r = make(halart, base)
    try:
        r.set_views(VIEWS)
        r.update_batch(2)
        for v, c in enumerate(VIEWS):
            assert_images(r, oracle_images(oracle, base, scenes.swap_cameras(base.scene, c), 2), f"{edit}: view {v} before", view=v)
        E.apply_to_renderer(r, fwd)
        r.refit()
        r.update(); r.update_batch(2); r.render()
        for v, c in enumerate(VIEWS):
            assert_images(r, oracle_images(oracle, base, scenes.swap_cameras(edited, c), 3), f"{edit}: view {v} after the refit", view=v)
    finally:
        r.close()


def aov_reference(oracle, base, scene, frames):
    lights, _ = oracle.pack_lights(scene)
    osc = oracle.OracleScene(scene, envmap=base.env)
    pos, ids = aov_ref.reference(osc, scene, lights, base.kw["width"], base.kw["height"], frames)
    osc.close()
    return pos, ids


@gpu
@pytest.mark.parametrize("case", [("cornell", "E1-move-mesh-node", False), ("cornell", "E2-move-lights", False), ("cornell", "E9-singular", True),
                                  ("cornell", "E8-emission-on", False), ("cornell", "E5-glass-to-diffuse", False), ("random", "E1-move-mesh-node", True)],
                         ids=lambda c: f"{c[0]}-{c[1]}")
def test_aovs_after_the_refit(halart, oracle, case):
    """position and ids on: after the refit both equal aov_ref on the edited scene (ids from frame 0 after the restart), images 0-3 the
    oracle's"""
    b, e, two_level = case
    base = base_of(b)
    fwd, _ = E.edit_ops(e, base.scene)
    edited = E.apply_to_scene(base.scene, fwd)
    with tree_form(oracle, two_level) as build:
        r = make(halart, base, build=build)
        try:
            r.set_aovs(True, True)
            r.update_batch(3)
            pos, ids = aov_reference(oracle, base, base.scene, 3)
            assert_same(r.read_image("position"), pos, "position before")
            assert_same(r.read_ids(), ids, "ids before")
            E.apply_to_renderer(r, fwd)
            r.refit()
            r.update(); r.update(); r.render()
            pos2, ids2 = aov_reference(oracle, base, edited, 2)
            assert_same(r.read_image("position"), pos2, f"{case}: position after the refit")
            assert_same(r.read_ids(), ids2, f"{case}: ids after the refit")
            assert_images(r, oracle_images(oracle, base, edited, 2), f"{case}: images with the AOVs on")
            assert pos2.tobytes() != pos.tobytes() or ids2.tobytes() != ids.tobytes() or e == "E8-emission-on"
        finally:
            r.close()


def cornell_part(oracle, scene):
    """the lights in group 0, the emissive materials in 1, every other material and the environment in 2"""
    lights, _ = oracle.pack_lights(scene)
    return [0] * len(lights), [1 if max(M.emission) > 0.0 else 2 for M in scene.materials], 2


def isolated(oracle, base, scene, part, g, frames):
    lg, mg, eg = part
    iso, keep_env = LG.isolate(scene, lg, mg, eg, g)
    return oracle_images(oracle, base, iso, frames, env_intensity=None if keep_env else 0.0)[0]


@gpu
@pytest.mark.parametrize("edit", ["E2-move-lights", "E8-emission-on", "E8-emission-off", "E8-emissive-medium", "E5-glass-to-diffuse"])
def test_light_groups_after_the_refit(halart, oracle, edit):
    """a partition with the lights, the emissive materials and the environment in three groups: after the edit + refit every group
    image equals the oracle's isolated edited scene, relight equals the numpy twin, and the descriptor survived; afterwards a set_scene +
    commit with one light more is refused by the coverage check"""
    base = base_of("cornell")
    fwd, _ = E.edit_ops(edit, base.scene)
    edited = E.apply_to_scene(base.scene, fwd)
    part = cornell_part(oracle, base.scene)
    r = make(halart, base)
    try:
        r.set_light_groups(lights=part[0], environment=part[2], materials=part[1], group_count=3)
        r.update_batch(2)
        E.apply_to_renderer(r, fwd)
        r.refit()
        assert r.light_group_count == 3
        r.update(); r.update(); r.render()
        imgs = []
        for g in range(3):
            want = isolated(oracle, base, edited, part, g, 2)
            got = r.read_light_group(g)
            assert_same(got, want, f"{edit}: group {g}")
            imgs.append(got)
        assert_images(r, oracle_images(oracle, base, edited, 2), f"{edit}: images with the groups on")
        sc = np.random.RandomState(3).uniform(-1.0, 3.0, (3, 3)).astype(f32)
        lin, _ = r.relight(sc)
        assert_same(lin, LG.relight(np.stack(imgs), sc), f"{edit}: relight")
        # the coverage refusal after a new scene with one light more
        more = E.apply_to_scene(base.scene, [])
        quad = next(nd for nd in more.nodes if nd.light_index == 0)
        more.lights.append(more.lights[0])
        more.nodes.append(H.HalaNode(name="light_2", light_index=len(more.lights) - 1, local_transform=quad.local_transform @ E._translate((0.0, 0.0, 50.0))))
        r.set_scene(more); r.commit()
        with pytest.raises(halart.HalaRendererError, match="light groups cover"):
            r.update()
    finally:
        r.close()


@gpu
@pytest.mark.parametrize("converged", [False, True])
def test_adaptive_sampling_restarts_at_the_refit(halart, oracle, converged):
    """adaptive sampling under way (some blocks converged, or every block) when the edit lands: after the refit every block is active
    again, and the status, the sample counts and the images equal the twin and the oracle of the edited scene from frame 0"""
    base = base_of("cornell")
    fwd, _ = E.edit_ops("E1-move-mesh-node", base.scene)
    edited = E.apply_to_scene(base.scene, fwd)
    w, h = base.kw["width"], base.kw["height"]
    ms, iv, frames = 4, 3, 13

    def snaps(scene, n):
        imgs = [np.zeros((h, w, 4), f32) for _ in range(4)]
        out = []
        for f in range(n):
            oracle_images(oracle, base, scene, 1, first_frame=f, images=imgs)
            out.append([i.copy() for i in imgs])
        return out

    before = snaps(base.scene, frames)
    after = snaps(edited, frames)
    thr = 1e30 if converged else float(AR.pick_threshold([x[0] for x in before], ms, iv))
    r = make(halart, base)
    try:
        r.set_adaptive_sampling(thr, min_samples=ms, interval=iv)
        for _ in range(frames):
            r.update()
        st = r.adaptive_status()
        assert st.active_blocks == 0 if converged else 0 < st.active_blocks < st.total_blocks
        E.apply_to_renderer(r, fwd)
        r.refit()
        st = r.adaptive_status()
        assert (st.active_blocks, st.samples) == (st.total_blocks, 0)
        for _ in range(frames):
            r.update()
        r.render()
        counts = r.read_sample_counts()
        want_counts, cb, s = AR.simulate([x[0] for x in after], thr, ms, iv)
        assert_same(counts, want_counts, "sample counts against the twin")
        ys, xs = np.mgrid[0:h, 0:w]
        for k in range(4):
            assert_same(r.read_image(k), np.stack([x[k] for x in after])[counts - 1, ys, xs], f"image {k} at each pixel's count")
        st = r.adaptive_status()
        assert (st.enabled, st.samples, st.last_snapshot, st.active_blocks) == (1, frames, s, int((cb == 0).sum()))
    finally:
        r.close()


@gpu
@pytest.mark.parametrize("edit", ["E1-move-mesh-node", "E6-invisible"])
def test_tile_shards_after_the_refit(halart, oracle, edit):
    """three emulated ranks each apply the edit and refit: the gathered frame equals the unsharded oracle frame of the edited scene,
    padding slots stay zero, and denoising after the gather equals denoise_ref on the new frame.  Between the refit and the new gather the
    accumulation is empty: denoise is refused, read_denoised still returns the last result"""
    import torch

    from hala_renderer_amd.dist import TileLayout
    base = base_of("cornell")
    fwd, _ = E.edit_ops(edit, base.scene)
    edited = E.apply_to_scene(base.scene, fwd)
    w, h, world, ts = base.kw["width"], base.kw["height"], 3, 16
    L = TileLayout(w, h, world, ts)
    parts = {k: [] for k in range(3)}
    last = None
    try:
        for rank in range(world):
            r = make(halart, base, shard=(rank, world, ts))
            if last is not None:
                last.close()
            last = r
            r.update_batch(2)
            E.apply_to_renderer(r, fwd)
            r.refit()
            r.update_batch(2); r.render(); r.wait_idle()
            pad = L.rank_pixel_map(rank)[:, 0] < 0
            for k in range(3):
                ptr, nbytes = r.tile_buffer(k)
                t = torch.as_tensor(halart.dist._DeviceView(ptr, nbytes // 4), device="cuda:0").clone()
                torch.cuda.synchronize()
                assert not t.cpu().numpy().reshape(-1, 4)[pad].view(np.uint32).any(), (rank, k)
                parts[k].append(t)
        want = oracle_images(oracle, base, edited, 2)
        gathered = {k: torch.cat(parts[k]).contiguous() for k in range(3)}
        torch.cuda.synchronize()
        for k in range(3):
            last.scatter_gathered_tiles(k, gathered[k].data_ptr(), gathered[k].numel() * 4)
            assert_same(last.read_image(k), want[k], f"{edit}: gathered AOV {k}")
        last.denoise()
        p = H.denoise_default_params()
        d = denoise_ref.denoise(want[0], want[1], want[2], iterations=p.iterations, sigma_color=p.sigma_color, sigma_albedo=p.sigma_albedo,
                                normal_power=p.normal_power, demodulate=bool(p.demodulate))
        first = last.read_denoised()
        assert_same(first, d, f"{edit}: denoised gathered frame")
        # a refit empties the accumulation: nothing to denoise until new samples (and, sharded, a new gather); the last result stays
        last.refit()
        with pytest.raises(halart.HalaRendererError, match="no sample"):
            last.denoise()
        assert_same(last.read_denoised(), first, "read_denoised after the refit")
        last.update_batch(2)
        with pytest.raises(halart.HalaRendererError, match="gather"):
            last.denoise()
        assert_same(last.read_denoised(), first, "read_denoised before the new gather")
    finally:
        if last is not None:
            last.close()


def play_edits(halart, oracle, timing_period, fusion, two_level):
    """edits and refits right behind update_batch + render (a tail may still run), then more updates -> what was read, in order"""
    base = base_of("cornell")
    out = []
    with tree_form(oracle, two_level) as build:
        r = make(halart, base, build=build)
        try:
            r.set_pass_fusion(fusion)
            r.set_launch_timing_period(timing_period)
            for e in ("E6-translucent", "E1-move-mesh-node", "E4-deform-shared", "E7-scatter-medium", "E5-glass-to-diffuse", "E6-alpha-map"):
                fwd, _ = E.edit_ops(e, base.scene)
                r.update_batch(2); r.render()
                E.apply_to_renderer(r, fwd)
                r.update_batch(1); r.render()
                r.refit()
                r.update_batch(2); r.update(); r.render()
                out += [(f"{e}/image{k}", r.read_image(k)) for k in range(4)]
                st = r.statistics()
                out.append((f"{e}/totals", (st.total_frames, st.rays_closest_total, st.rays_shadow_total, st.rays_primary_total)))
        finally:
            r.close()
    return out


@gpu
@pytest.mark.parametrize("two_level", [False, True], ids=["one_level", "two_level"])
@pytest.mark.parametrize("fusion", [2, 0])
def test_edits_behind_an_open_tail(halart, oracle, fusion, two_level):
    """update_material / update_node_transform / update_vertices / refit right behind update_batch + render, while the frame's tail may
    still run beside it: the overlapped run (no per-launch timing) equals the serial one (timing on every update) bit for bit"""
    overlapped = play_edits(halart, oracle, 0, fusion, two_level)
    serial = play_edits(halart, oracle, 1, fusion, two_level)
    assert [w for w, _ in overlapped] == [w for w, _ in serial]
    for (what, got), (_, want) in zip(overlapped, serial):
        if isinstance(got, np.ndarray):
            assert_same(got, want, what)
        else:
            assert got == want, what


@gpu
def test_refused_edits_change_nothing(halart, oracle):
    """before commit every update_* is refused; on a committed scene out-of-range indices, a vertex count that differs, a non-finite
    position and a material type above 1 are refused.  Afterwards the renderer renders the old scene bit for bit, and the edits made
    before the refusals still apply at the next refit"""
    base = base_of("cornell")
    s = base.scene
    v = s.meshes[1].primitives[0].vertices.copy()
    mat = s.materials[4]
    r = make(halart, base)
    try:
        fresh = halart.HalaRenderer("edits", base.kw["width"], base.kw["height"], 5, 3, False, False, False, 0)
        try:
            for call in (lambda: fresh.update_node_transform(0, np.eye(4, dtype=f32)), lambda: fresh.update_material(0, mat),
                         lambda: fresh.update_vertices(1, 0, v), fresh.refit):
                with pytest.raises(halart.HalaRendererError):
                    call()
            fresh.set_scene(s)  # set, not committed
            for call in (lambda: fresh.update_node_transform(0, np.eye(4, dtype=f32)), lambda: fresh.update_material(0, mat),
                         lambda: fresh.update_vertices(1, 0, v), fresh.refit):
                with pytest.raises(halart.HalaRendererError, match="none"):
                    call()
        finally:
            fresh.close()
        r.update_batch(2)
        before = [r.read_image(k).tobytes() for k in range(4)]
        fwd, _ = E.edit_ops("E1-move-mesh-node", s)
        E.apply_to_renderer(r, fwd)  # accepted: applies at the refit below
        bad_v = v.copy(); bad_v["position"][3, 1] = np.nan
        inf_v = v.copy(); inf_v["position"][0, 2] = np.inf
        bad_mat = E.apply_to_scene(s, []).materials[4]; bad_mat.type = 2
        refusals = [(lambda: r.update_node_transform(len(s.nodes), np.eye(4, dtype=f32)), "node"),
                    (lambda: r.update_material(len(s.materials), mat), "material"),
                    (lambda: r.update_material(4, bad_mat), "type"),
                    (lambda: r.update_vertices(len(s.meshes), 0, v), "mesh"),
                    (lambda: r.update_vertices(1, 1, v), "primitive"),
                    (lambda: r.update_vertices(1, 0, v[:-1]), "count"),
                    (lambda: r.update_vertices(1, 0, np.concatenate([v, v[:1]])), "count"),
                    (lambda: r.update_vertices(1, 0, bad_v), "finite"),
                    (lambda: r.update_vertices(1, 0, inf_v), "finite")]
        for call, word in refusals:
            with pytest.raises(halart.HalaRendererError, match=word):
                call()
        # the refusals (and the accepted edit) changed nothing yet: the accumulation goes on with the old scene
        r.reset_accumulation()
        r.update_batch(2)
        assert [r.read_image(k).tobytes() for k in range(4)] == before
        r.refit()
        r.update_batch(2)
        assert_images(r, oracle_images(oracle, base, E.apply_to_scene(s, fwd), 2), "the accepted edit at the refit")
    finally:
        r.close()
