"""The history clamp of temporal reprojection (docs/RENDER_SPEC.md 16 "History clamp"; include/halart.h "hala_rt_set_temporal_clamp").

CPU tier: the numpy twin (tests/temporal_clamp_ref.py) on the oracle's frames of the scene_edits bases, 48 x 36, default temporal
parameters.  With the clamp off it equals the two existing twins bytewise; with it on, stale light after a lighting edit is removed (g-space
MSE against 1024 frames of the edited scene), good history is kept (a regression cap), and the defined cases of the rule are pinned on
synthetic frames against a scalar restatement of the spec text; parameter validation and the surface of the entry points.
GPU tier: csrc/temporal.hip equals the twin byte for byte on both output images for every radius, on partial tiles and frames smaller than
the halo, with vertex motion, through a chain of captures, behind an open tail, and with the feature turned off again; refusals."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import scene_edits as E
import temporal_clamp_ref as K
import temporal_ref as T
import temporal_vertex_ref as V
import test_temporal as TT
import test_temporal_vertex as TV
from conftest import ROOT
from hala_renderer_amd import _abi as A
from test_temporal import base_of, frames_of, g_space

gpu = pytest.mark.gpu
f32 = np.float32
DEFAULT = T.Params()
CLAMP = K.DEFAULT_CLAMP


# ---- CPU tier: the clamp off -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edit", ["E1-move-mesh-node", "E2-move-lights", "E4-deform-shared"])
def test_clamp_off_equals_the_existing_twins(oracle, edit):
    """clamp=None: temporal_ref.resolve's bytes with the marks as instance marks, temporal_vertex_ref.resolve's with them as vertex marks
    and a snapshot (E4 then takes the vertex-motion path)"""
    base = base_of("cornell")
    prev, cur = frames_of(oracle, "cornell", None, 0, 3), frames_of(oracle, "cornell", edit, 0, 4)
    im, mm = T.marks_of(base.scene, E.edit_ops(edit, base.scene)[0])
    args = (cur.C, cur.Pm, cur.I, cur.n)
    want = T.resolve(*args, prev.history(), cur.cam, cur.world, im, mm, params=DEFAULT)
    got = K.resolve(*args, prev.history(), cur.cam, cur.world, im, mm, params=DEFAULT)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert (want[0][..., 3] > cur.n).any()
    tris = V.tris_of(cur.scene, cur.world)
    for hist in (prev.history(), TV.vertex_history(prev)):
        want = V.resolve(*args, hist, cur.cam, cur.world, None, mm, params=DEFAULT, tris_cur=tris, vertex_marked=im)
        got = K.resolve(*args, hist, cur.cam, cur.world, None, mm, params=DEFAULT, tris_cur=tris, vertex_marked=im)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    if edit == "E4-deform-shared":
        marked = TV.marked_hits(cur, im)
        assert (want[0][marked][:, 3] > cur.n).any(), "the vertex-motion path carried history"
    # no history at all
    got = K.resolve(*args, None, cur.cam, cur.world, clamp=CLAMP)
    want = T.resolve(*args, None, cur.cam, cur.world)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


# ---- CPU tier: quality -------------------------------------------------------------------------------------------------------------------
_REFS = {}


def edited_scene(base_name, edit):
    """(scene, ops) of a scene_edits edit, or of "camera": the move of camera 0's node that test_temporal.quality_case makes"""
    base = base_of(base_name)
    if edit == "camera":
        node = next(i for i, nd in enumerate(base.scene.nodes) if nd.camera_index == 0)
        move = np.asarray(base.scene.nodes[node].local_transform, f32) @ E._translate((0.04 * E._extent(base.scene), 0.0, 0.0)) @ E._rot(ry=0.05)
        ops = [("node", node, move)]
    else:
        ops = E.edit_ops(edit, base.scene)[0]
    return E.apply_to_scene(base.scene, ops), ops


def quality(oracle, base_name, edit, clamp=CLAMP, hist_frames=64, new_frames=4, ref_frames=1024):
    """-> g-space MSE against ref_frames of the edited scene of: the accumulation of new_frames, the temporal image, the clamped one"""
    base = base_of(base_name)
    scene, ops = edited_scene(base_name, edit)
    prev = frames_of(oracle, base_name, None, 0, hist_frames)
    key = (base_name, edit, new_frames)
    if key not in _REFS:
        kw = base.kw
        osc = oracle.OracleScene(scene, envmap=base.env)
        ref, _ = osc.render(kw["width"], kw["height"], frames=ref_frames, max_depth=kw["max_depth"], rr_depth=kw["rr_depth"], tonemap=kw["tonemap"],
                            env_rotation=kw["env_rotation"] if base.env is not None else 0.0,
                            env_intensity=kw["env_intensity"] if base.env is not None else 1.0, exposure=kw["exposure"])
        osc.close()
        cur = frames_of(oracle, base_name, edit, 0, new_frames) if edit != "camera" else TT.Frames(oracle, base, scene, new_frames)
        _REFS[key] = (g_space(ref[0]), cur)
    ref, cur = _REFS[key]
    im, mm = T.marks_of(base.scene, ops)
    args = (cur.C, cur.Pm, cur.I, cur.n, prev.history(), cur.cam, cur.world, im, mm)
    plain, _ = T.resolve(*args, params=DEFAULT)
    clamped, _ = K.resolve(*args, params=DEFAULT, clamp=clamp)
    mse = lambda x: float(np.mean((g_space(x) - ref) ** 2))  # noqa: E731
    return dict(accum=mse(cur.C), temporal=mse(plain), clamped=mse(clamped))


def test_stale_light_is_removed(oracle):
    """cornell, 64 history frames + 4 new ones against 1024 of the edited scene, g-space MSE x 1e-4, defaults (r = 1, gamma = 2).
    Measured with this twin (accumulation / temporal / clamped):
      E8-emission-on   64.6 / 296.7 / 43.2      E2-move-lights   37.7 / 21.0 / 13.3
    After a material starts to emit, the unclamped temporal image is worse than the four new samples alone; the clamped one is better
    than both.  Each gap is far wider than any float32 / float64 difference."""
    q = quality(oracle, "cornell", "E8-emission-on")
    print("cornell E8-emission-on:", q)
    assert q["clamped"] < q["accum"] < q["temporal"]
    q = quality(oracle, "cornell", "E2-move-lights")
    print("cornell E2-move-lights:", q)
    assert q["clamped"] < q["temporal"]


@pytest.mark.parametrize("edit", ["E1-move-mesh-node", "camera"])
def test_good_history_is_kept(oracle, edit):
    """A regression cap, not a tuning result: where the geometric checks already leave only good history (a moved mesh node, a moved
    camera), the clamp may cost at most 5 %.  Measured with this twin, clamped / unclamped g-space MSE at the defaults:
      cornell E1-move-mesh-node  x 1.005 (5.86 -> 5.89 e-4)      cornell camera 0 moved  x 0.941 (8.86 -> 8.35 e-4)"""
    q = quality(oracle, "cornell", edit)
    print(f"cornell {edit}:", q, "ratio", q["clamped"] / q["temporal"])
    assert q["temporal"] < q["accum"], "the history is good"
    assert q["clamped"] <= 1.05 * q["temporal"]


# ---- CPU tier: defined cases on synthetic frames -----------------------------------------------------------------------------------------
def synthetic(W, H, C_rgb, H_rgb, n=4, h=8.0, absent=None):
    """a static frame seen by an orthographic camera, one instance, the history captured from the same camera: every pixel reprojects
    onto itself with weight 1 exactly, so Hrgb of pixel p is H_rgb[p] bit for bit"""
    cam = T.Camera(np.array([0, 0, 5], f32), np.array([1, 0, 0], f32), np.array([0, 1, 0], f32), np.array([0, 0, -1], f32), f32(0.0),
                   f32(1.0), f32(1.0), 1)
    ys, xs = np.mgrid[0:H, 0:W]
    Pm = np.stack([xs * 0.1, ys * 0.1, np.zeros((H, W)), np.ones((H, W))], axis=-1).astype(f32)
    I = np.zeros((H, W, 4), np.uint32)
    if absent is not None:
        I[absent, 1] = T.ABSENT
    Cc = np.concatenate([np.broadcast_to(np.asarray(C_rgb, f32), (H, W, 3)), np.full((H, W, 1), f32(n))], axis=-1).astype(f32)
    Hc = np.concatenate([np.broadcast_to(np.asarray(H_rgb, f32), (H, W, 3)), np.full((H, W, 1), f32(h))], axis=-1).astype(f32)
    world = np.eye(4, dtype=f32).reshape(1, 16)
    return dict(C=Cc, Pm=Pm, I=I, n=n, hist=T.History(Hc, Pm.copy(), np.zeros((H, W, 4), np.uint32), cam, world), cam_cur=cam, world_cur=world)


def blend(hrgb, h, c, n):
    hrgb, c, h, n = np.asarray(hrgb, f32), np.asarray(c, f32), f32(h), f32(n)
    with np.errstate(invalid="ignore"):
        return (((hrgb * h).astype(f32) + (c * n).astype(f32)).astype(f32) / f32(h + n)).astype(f32)


def scalar_bounds(C, x, y, r, gamma):
    """steps 1-3 of the rule for one pixel, one float32 operation at a time as the spec writes them -> lo, hi [3], k"""
    Hh, W = C.shape[:2]
    taps = [(x + dx, y + dy) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if 0 <= x + dx < W and 0 <= y + dy < Hh]
    lo, hi = np.empty(3, f32), np.empty(3, f32)
    with np.errstate(all="ignore"):
        for c in range(3):
            k, s1 = f32(0.0), f32(0.0)
            for qx, qy in taps:
                k = f32(k + f32(1.0))
                s1 = f32(s1 + C[qy, qx, c])
            mu = f32(s1 / k)
            s2 = f32(0.0)
            for qx, qy in taps:
                d = f32(C[qy, qx, c] - mu)
                s2 = f32(s2 + f32(d * d))
            v = f32(s2 / k)
            half = f32(f32(gamma) * np.sqrt(f32(v / k)))
            lo[c], hi[c] = f32(mu - half), f32(mu + half)
    return lo, hi, len(taps)


def test_constant_neighbourhood_clamps_the_history_onto_it():
    """a constant C has variance 0: lo = hi = C, so whatever the history holds, T.rgb = C exactly"""
    s = synthetic(7, 6, (0.5, 0.25, 2.0), (9.0, 0.0, 2.0))
    for r in (1, 2, 3):
        lo, hi, _ = K.clamp_bounds(s["C"], r, 2.0)
        assert lo.tobytes() == hi.tobytes() == s["C"][..., :3].tobytes()
        Tm, M = K.resolve(**s, clamp=(r, 2.0))
        assert (Tm[..., 3] == 12.0).all() and (M[..., 3] == 1).all()
        assert Tm[..., :3].tobytes() == blend(s["C"][..., :3], 8.0, s["C"][..., :3], 4).tobytes()
    plain, _ = K.resolve(**s)
    assert plain[..., :3].tobytes() == blend(s["hist"].Hc[..., :3], 8.0, s["C"][..., :3], 4).tobytes(), "Hrgb is the history pixel itself"


@pytest.mark.parametrize("shape", [(1, 1), (2, 5), (8, 8), (19, 17)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_bounds_equal_the_scalar_restatement_and_the_history_lands_on_them(shape):
    """frames smaller than the neighbourhood (1 x 1, 2 x 5 with r = 3), the tap counts at corners and edges, and step 4: Hrgb inside the
    box is untouched bitwise, above / below it lands exactly on hi / lo; T.w, the motion image and pixels without history are the
    unclamped ones"""
    W, H = shape
    rng = np.random.default_rng(W * 100 + H)
    C_rgb = (rng.random((H, W, 3)) * np.where(rng.random((H, W, 1)) < 0.1, 50.0, 1.0)).astype(f32)  # a few bright HDR pixels
    H_rgb = (rng.random((H, W, 3)) * 1.2).astype(f32)  # around the neighbourhood means of the dim pixels, far below those of the bright ones
    absent = rng.random((H, W)) < 0.15 if W * H > 4 else None
    s = synthetic(W, H, C_rgb, H_rgb, absent=absent)
    plain_t, plain_m = K.resolve(**s)
    carried = plain_t[..., 3] == 12.0
    assert carried.all() if absent is None else (carried == ~absent).all()
    for r, gamma in ((1, 2.0), (2, 0.5), (3, 2.0), (3, 6.0)):
        lo, hi, k = K.clamp_bounds(s["C"], r, gamma)
        for y in range(H):
            for x in range(W):
                slo, shi, sk = scalar_bounds(s["C"], x, y, r, gamma)
                assert k[y, x] == sk and lo[y, x].tobytes() == slo.tobytes() and hi[y, x].tobytes() == shi.tobytes(), (x, y, r)
        assert k[0, 0] == min(r + 1, W) * min(r + 1, H)
        if shape == (8, 8) and r == 3:
            assert k[0, 0] == 16 and k[4, 4] == 49 and k[0, 4] == 28
        if shape == (1, 1):
            assert lo.tobytes() == hi.tobytes() == C_rgb.tobytes(), "one tap: no variance"
        Tm, M = K.resolve(**s, clamp=(r, gamma))
        assert M.tobytes() == plain_m.tobytes() and Tm[..., 3].tobytes() == plain_t[..., 3].tobytes()
        assert Tm[~carried].tobytes() == plain_t[~carried].tobytes()
        assert Tm[~carried][:, :3].tobytes() == s["C"][~carried][:, :3].tobytes() and (Tm[~carried][:, 3] == 4).all()
        below, above = H_rgb < lo, H_rgb > hi
        inside = ~below & ~above
        want = np.where(below, lo, np.where(above, hi, H_rgb))
        assert Tm[carried][:, :3].tobytes() == blend(want, 8.0, C_rgb, 4)[carried].tobytes()
        untouched = carried[..., None] & inside
        assert Tm[..., :3][untouched].tobytes() == plain_t[..., :3][untouched].tobytes()
        if W * H > 100:
            assert (carried[..., None] & below).any() and (carried[..., None] & above).any() and untouched.any()


def test_nan_history_stays_and_nan_bounds_leave_the_history():
    C_rgb = np.full((5, 5, 3), 0.5, f32)
    C_rgb[2, 2, 0] = np.nan   # channel 0 of the 3 x 3 around (2, 2): NaN bounds
    C_rgb[0, 4, 1] = np.inf   # inf - inf: NaN bounds too
    H_rgb = np.full((5, 5, 3), 3.0, f32)
    H_rgb[4, 0] = np.nan
    s = synthetic(5, 5, C_rgb, H_rgb)
    Tm, _ = K.resolve(**s, clamp=(1, 2.0))
    plain, _ = K.resolve(**s)
    lo, hi, _ = K.clamp_bounds(s["C"], 1, 2.0)
    assert np.isnan(lo[1:4, 1:4, 0]).all() and np.isnan(lo[0:2, 3:5, 1]).all() and not np.isnan(lo[..., 2]).any()
    assert Tm[1:4, 1:4, 0].tobytes() == plain[1:4, 1:4, 0].tobytes(), "NaN bounds: Hrgb unchanged"
    assert Tm[0:2, 3:5, 1].tobytes() == plain[0:2, 3:5, 1].tobytes()
    assert np.isnan(Tm[4, 0, :3]).all(), "a NaN history stays NaN"
    assert Tm[0, 0, :3].tobytes() == np.full(3, 0.5, f32).tobytes(), "and everything else is clamped onto the constant"


# ---- CPU tier: parameters, surface ---------------------------------------------------------------------------------------------------
def test_clamp_params_layout_and_defaults(halart):
    assert C.sizeof(A.TemporalClampParams) == 16
    offsets = {f: getattr(A.TemporalClampParams, f).offset for f, _ in A.TemporalClampParams._fields_}
    assert offsets == {"radius": 0, "gamma": 4, "reserved": 8}
    assert re.search(r"\}\s*hala_temporal_clamp_params;\s*/\*\s*16 B", open(os.path.join(ROOT, "include", "halart.h")).read())
    p = halart.temporal_clamp_default_params()
    assert (p.radius, p.gamma, list(p.reserved)) == (K.DEFAULT_CLAMP[0], f32(K.DEFAULT_CLAMP[1]), [0, 0]) == (1, 2.0, [0, 0])
    assert K.check_params(p.radius, p.gamma) == ""
    assert C.sizeof(A.TemporalParams) == 32, "the temporal parameters keep their layout"


BAD_PARAMS = [("radius", 0), ("radius", 4), ("gamma", 0.0), ("gamma", -1.0), ("gamma", math.nan), ("gamma", math.inf), ("gamma", 1000.5)]


@pytest.mark.parametrize("field,value", BAD_PARAMS)
def test_invalid_clamp_params_are_refused_before_the_handle_is_looked_at(halart, field, value):
    lib = halart.load_library()
    p = halart.temporal_clamp_default_params(**{field: value})
    want = K.check_params(p.radius, p.gamma)
    assert field in want
    assert lib.hala_rt_set_temporal_clamp(None, C.byref(p)) == 1
    assert halart.last_error() == want


def test_reserved_words_and_null_handle_are_refused(halart):
    lib = halart.load_library()
    for k in (0, 1):
        p = halart.temporal_clamp_default_params()
        p.reserved[k] = 7
        assert lib.hala_rt_set_temporal_clamp(None, C.byref(p)) == 1 and halart.last_error() == K.check_params(1, 2.0, (1, 0))
    for gamma in (1e-3, 1000.0):
        p = halart.temporal_clamp_default_params(radius=3, gamma=gamma)
        assert K.check_params(3, gamma) == ""
        assert lib.hala_rt_set_temporal_clamp(None, C.byref(p)) == 1 and "null" in halart.last_error()
    assert lib.hala_rt_set_temporal_clamp(None, None) == 1 and "null" in halart.last_error()


def test_header_exports_and_binding_carry_the_entry_points(halart):
    raw = open(os.path.join(ROOT, "include", "halart.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\bvoid hala_temporal_clamp_default_params\s*\(\s*hala_temporal_clamp_params\s*\*\s*out\s*\)", text)
    assert re.search(r"\bint hala_rt_set_temporal_clamp\s*\(\s*hala_rt_renderer\s*\*\s*r\s*,\s*const hala_temporal_clamp_params\s*\*\s*p\s*\)", text)
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int hala_rt_set_temporal_clamp\(", raw, flags=re.S)
    assert m and "RENDER_SPEC 16" in m.group(1), "cites its section of the spec"
    lib = C.CDLL(halart.LIB_PATH)
    rust = open(os.path.join(ROOT, "rust", "hala-renderer-halart", "src", "lib.rs")).read()
    for name in ("hala_temporal_clamp_default_params", "hala_rt_set_temporal_clamp"):
        assert name in A.EXPORTS and name in A.PROTOTYPES, name
        assert hasattr(lib, name), name
        assert name in rust, name
    assert callable(getattr(halart.HalaRenderer, "set_temporal_clamp")) and callable(halart.temporal_clamp_default_params)


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------------------
class CTwin(TV.VTwin):
    """the renderer's temporal state with the clamp: test_temporal_vertex.VTwin resolved by temporal_clamp_ref"""

    def __init__(self, r, scene, clamp=CLAMP, vertex=False, params=DEFAULT):
        super().__init__(r, scene, 0, params, on=vertex)
        self.clamp = clamp

    def tris(self):
        return super().tris() if self.on else None

    def resolve(self, clamp="own"):
        return K.resolve(hist=self.hist, clamp=self.clamp if clamp == "own" else clamp, **self._marks(self.tris()), **self.state())

    def capture(self):
        tris = self.tris()
        self.hist = K.capture(hist=self.hist, snapshot=self.on and tris is not None, clamp=self.clamp, **self._marks(tris), **self.state())
        self.clear_marks()


def make(halart, base, clamp=CLAMP, vertex=False, **temporal):
    r = TT.make(halart, base, build=dict(instancing=False))
    r.set_temporal(**temporal)
    if vertex:
        r.set_temporal_vertex_motion()
    if clamp is not None:
        r.set_temporal_clamp(*clamp)
    return r


def clamp_bit(twin, want_t):
    """how many pixels the clamp changed"""
    plain, _ = twin.resolve(clamp=None)
    return int(np.any(plain.view(np.uint32) != want_t.view(np.uint32), axis=-1).sum())


RADIUS_CASES = [("cornell", "E2-move-lights"), ("cornell", "E8-emission-on"), ("textured", "E1-move-mesh-node"), ("random", "E1-move-mesh-node")]


@gpu
@pytest.mark.parametrize("case", RADIUS_CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_kernel_equals_the_twin_for_every_radius(halart, case):
    """5 frames, capture, the edit, refit, update_batch(4): both output images equal the twin's byte for byte with r = 1, 2, 3 at
    gamma = 2 (and gamma = 0.5 on cornell E2); the radius and gamma are launch arguments, so one renderer runs them all"""
    b, e = case
    base = base_of(b)
    fwd, _ = E.edit_ops(e, base.scene)
    r = make(halart, base)
    try:
        twin = CTwin(r, base.scene)
        r.update_batch(5)
        TT.check_resolve(r, twin, f"{case} before any capture")
        TT.edit_round(r, twin, fwd, lambda r: r.update_batch(4))
        clamps = [(1, 2.0), (2, 2.0), (3, 2.0)] + ([(1, 0.5)] if case == RADIUS_CASES[0] else [])
        for clamp in clamps:
            r.set_temporal_clamp(*clamp)
            twin.clamp = clamp
            t, _ = TT.check_resolve(r, twin, f"{case} {clamp}")
            assert (t[..., 3] > 4).any(), "some pixels carry history"
            assert clamp_bit(twin, t) > 20, "and the clamp changed some of them"
        r.update()
        TT.check_resolve(r, twin, f"{case} one update later")
    finally:
        r.close()


@gpu
@pytest.mark.parametrize("size", [(37, 23), (5, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_partial_tiles_and_frames_smaller_than_the_halo(halart, size):
    """37 x 23 is no multiple of the 16 x 16 tile: the threads outside the frame stage and meet the barrier before they return; 5 x 3 is
    narrower than the r = 3 neighbourhood, so every pixel has fewer than 49 taps"""
    base = E.cornell(*size)
    fwd, _ = E.edit_ops("E2-move-lights", base.scene)
    r = make(halart, base, clamp=(3, 2.0))
    try:
        twin = CTwin(r, base.scene, clamp=(3, 2.0))
        for _ in range(5):
            r.update()
        TT.edit_round(r, twin, fwd, lambda r: [r.update() for _ in range(3)])
        t, _ = TT.check_resolve(r, twin, f"{size}")
        assert (t[..., 3] > 3).any() and clamp_bit(twin, t) > 0
        for clamp in ((1, 2.0), (2, 1.0)):
            r.set_temporal_clamp(*clamp)
            twin.clamp = clamp
            TT.check_resolve(r, twin, f"{size} {clamp}")
    finally:
        r.close()


@gpu
def test_vertex_motion_and_clamp_together(halart):
    """cornell E4 with set_temporal_vertex_motion: the instantiation with both on"""
    base = base_of("cornell")
    fwd, _ = TV.e4_ops("cornell")
    r = make(halart, base, vertex=True)
    try:
        twin = CTwin(r, base.scene, vertex=True)
        r.update_batch(5)
        TT.edit_round(r, twin, fwd, lambda r: r.update_batch(4))
        assert twin.hist.tris is not None and twin.im.any()
        for clamp in ((1, 2.0), (3, 2.0)):
            r.set_temporal_clamp(*clamp)
            twin.clamp = clamp
            t, _ = TT.check_resolve(r, twin, f"E4 {clamp}")
            marked = TV.marked_now(r, twin)
            assert marked.sum() > 20 and (t[marked][:, 3] > 4).sum() >= 0.8 * marked.sum(), "the deformed surface carries history"
            plain, _ = twin.resolve(clamp=None)
            assert np.any(plain[marked] != t[marked]), "which the clamp changed"
    finally:
        r.close()


@gpu
def test_chain_of_two_edits_hands_the_clamped_image_on(halart):
    """capture, E8, 4 frames, capture, E2, 4 frames, resolve: the second capture keeps the clamped image as the history"""
    base = base_of("cornell")
    e8, _ = E.edit_ops("E8-emission-on", base.scene)
    e2, _ = E.edit_ops("E2-move-lights", base.scene)
    r = make(halart, base)
    try:
        twin = CTwin(r, base.scene)
        r.update_batch(8)
        TT.edit_round(r, twin, e8, lambda r: r.update_batch(4))
        t, _ = TT.check_resolve(r, twin, "after E8")
        plain, _ = twin.resolve(clamp=None)
        assert clamp_bit(twin, t) > 20
        TT.edit_round(r, twin, e2, lambda r: r.update_batch(4))
        assert twin.hist.Hc.tobytes() == t.tobytes() != plain.tobytes(), "the history is the clamped image"
        t, _ = TT.check_resolve(r, twin, "after E8 and E2")
        assert float(t[..., 3].max()) == 8 + 4 + 4
    finally:
        r.close()


@gpu
def test_resolve_directly_behind_an_update(halart):
    """no wait between update() and the resolve: the staging loads go behind the open tail, whose k_resolve still folds the image they read"""
    base = base_of("cornell")
    fwd, _ = E.edit_ops("E2-move-lights", base.scene)
    r = make(halart, base, clamp=(2, 2.0))
    try:
        r.set_launch_timing_period(0)  # untimed updates: the ones that leave their tail open
        twin = CTwin(r, base.scene, clamp=(2, 2.0))
        r.update_batch(3)
        TT.edit_round(r, twin, fwd, lambda r: r.update_batch(2))
        TT.check_resolve(r, twin, "first resolve (uploads the table)")
        for k in range(3):
            r.update()
            r.temporal_resolve()  # straight behind the update
            want_t, want_m = twin.resolve()  # (the read-backs in here wait)
            TT.assert_same(r.read_temporal(0), want_t, f"tail overlap {k}: temporal")
            TT.assert_same(r.read_temporal(1), want_m, f"tail overlap {k}: motion")
        r.update()
        r.temporal_capture()  # the same for a capture
        twin.capture()
        r.update()
        TT.check_resolve(r, twin, "after a capture behind an update")
    finally:
        r.close()


@gpu
def test_feature_on_then_off_and_the_frame_path_is_untouched(halart):
    """turned off again the resolve is the existing twin's; images 0-5 and the statistics are the same with the clamp on"""
    base = base_of("cornell")
    fwd, _ = E.edit_ops("E2-move-lights", base.scene)
    got = []
    for on in (False, True):
        r = make(halart, base, clamp=CLAMP if on else None)
        try:
            twin = CTwin(r, base.scene, clamp=CLAMP if on else None)
            r.update_batch(3); r.update()
            TT.edit_round(r, twin, fwd, lambda r: (r.update_batch(2), r.update()))
            t, _ = TT.check_resolve(r, twin, f"clamp {on}")
            assert r.statistics().total_frames == 3
            if on:
                assert clamp_bit(twin, t) > 20
                r.set_temporal_clamp(enable=False)
                assert r.statistics().total_frames == 3, "the accumulation goes on"
                plain = TT.Twin(r, base.scene)
                plain.hist, plain.im, plain.mm = twin.hist, twin.im, twin.mm
                off_t, _ = TT.check_resolve(r, plain, "turned off: the existing twin")
                assert off_t.tobytes() != t.tobytes()
                assert (off_t[..., 3] > 3).any(), "the history stayed"
            st = r.statistics()
            got.append(([r.read_image(k).tobytes() for k in range(6)],
                        [getattr(st, f) for f in ("total_frames", "rays_total", "rays_closest_total", "rays_shadow_total", "rays_primary_total", "updates_rendered")]))
        finally:
            r.close()
    assert got[0][1] == got[1][1]
    for k in range(6):
        assert got[0][0][k] == got[1][0][k], f"image {k}"


@gpu
def test_refusals_leave_the_renderer_as_it_was(halart):
    base = base_of("cornell")
    fwd, _ = E.edit_ops("E2-move-lights", base.scene)
    Err = halart.HalaRendererError
    r = TT.make(halart, base, build=dict(instancing=False))
    try:
        r.update_batch(2)
        before = [r.read_image(k).tobytes() for k in range(6)]
        for enable in (True, False):
            with pytest.raises(Err, match="temporal reprojection is off"):
                r.set_temporal_clamp(enable=enable)
        assert r.statistics().total_frames == 2 and [r.read_image(k).tobytes() for k in range(6)] == before
        r.set_temporal()
        r.set_temporal_clamp(2, 3.0)
        assert r.statistics().total_frames == 2, "the accumulation goes on"
        twin = CTwin(r, base.scene, clamp=(2, 3.0))
        TT.edit_round(r, twin, fwd, lambda r: r.update_batch(3))
        t, _ = TT.check_resolve(r, twin, "(2, 3)")
        assert clamp_bit(twin, t) > 0
        # bad parameters: the state is untouched
        for bad, what in ((dict(radius=4), "radius"), (dict(radius=0), "radius"), (dict(gamma=0.0), "gamma"), (dict(gamma=math.nan), "gamma")):
            with pytest.raises(Err, match=what):
                r.set_temporal_clamp(**bad)
        TT.check_resolve(r, twin, "(2, 3) after refused parameters")
        # set_temporal(NULL) turns the clamp off with it
        r.set_temporal(False)
        with pytest.raises(Err, match="temporal reprojection is off"):
            r.set_temporal_clamp()
        r.set_temporal()
        plain = TT.Twin(r, base.scene)
        r.update_batch(2)
        TT.edit_round(r, plain, E.edit_ops("E2-move-lights", base.scene)[1], lambda r: r.update_batch(3))
        off_t, _ = TT.check_resolve(r, plain, "back on without the clamp: the existing twin")
        assert (off_t[..., 3] > 3).any()
    finally:
        r.close()
