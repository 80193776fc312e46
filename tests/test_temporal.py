"""Temporal reprojection of the accumulated frame across scene edits (docs/RENDER_SPEC.md 16; include/halart.h "hala_rt_set_temporal").

CPU tier: the numpy twin (tests/temporal_ref.py) is fed with the oracle's own first hits (aov_ref.first_hits) on the scene_edits bases.
Its motion vectors are checked against a float64 geometric model, and its defined cases (static frame, whole-pixel camera shift,
uncovered background, marks, singular transforms, points behind the camera, max_history, parameter validation) are pinned.
GPU tier: csrc/temporal.hip equals the twin byte for byte on both output images through edits, tree forms, an odd frame size, batches, the
tail overlap and a chain of captures; images 0-5 and the statistics do not change with the feature on; refusals; quality.

The CPU scenes are 48 x 36 pixels, so one pixel is 1/36 of the view: the mean hit point of a pixel (image 4) moves by a sizeable fraction
of `tol * depth` from one accumulation to the next.  The geometric tests therefore run with tol = 0.2 where they are not about tol."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import aov_ref
import denoise_ref
import hala_renderer_amd as H
import scene_edits as E
import temporal_ref as T
from conftest import ROOT
from hala_renderer_amd import _abi as A
from hala_renderer_amd import scenes

gpu = pytest.mark.gpu
f32 = np.float32
ABSENT = np.uint32(0xFFFFFFFF)
WIDE = T.Params(tol=0.2)

# Largest |twin motion - float64 model| over every case of test_motion_agrees_with_the_float64_model, measured on the CPU before the
# bound was written down (that test's docstring has the figures).  The bound must be at least 4 x that and at most 0.01 px; 1e-4 px is
# 14 x the measured deviation: float32 rounding (6e-8) of pixel coordinates up to 48, through about twenty operations.
MEASURED_MOTION_DEVIATION = 7.3e-6
MOTION_BOUND = 1e-4
assert 4 * MEASURED_MOTION_DEVIATION <= MOTION_BOUND <= 0.01

_BASES = {}


def base_of(name):
    if name not in _BASES:
        _BASES[name] = E.BASES[name]()
    return _BASES[name]


def viewed(scene, cam):
    return scenes.swap_cameras(scene, cam) if cam else scene


class Frames:
    """what the renderer would hold after `frames` updates of `scene` (camera 0), from the oracle: accum, images 4 and 5, the packed
    camera and instance transforms, and the (triangle, u, v) of every sample's first hit"""

    def __init__(self, oracle, base, scene, frames):
        kw = base.kw
        self.w, self.h, self.n, self.scene = kw["width"], kw["height"], frames, scene
        osc = oracle.OracleScene(scene, envmap=base.env)
        imgs, _ = osc.render(self.w, self.h, frames=frames, max_depth=kw["max_depth"], rr_depth=kw["rr_depth"], tonemap=kw["tonemap"],
                             env_rotation=kw["env_rotation"] if base.env is not None else 0.0,
                             env_intensity=kw["env_intensity"] if base.env is not None else 1.0, exposure=kw["exposure"])
        self.C = imgs[0]
        lights = oracle.pack_lights(scene)[0]
        self.Pm, self.I = aov_ref.reference(osc, scene, lights, self.w, self.h, frames)
        self.hits = []
        for f in range(frames):
            hit = osc.trace(osc.camera_rays(self.w, self.h, f), 0)
            _, ids = aov_ref.first_hits(osc, scene, lights, self.w, self.h, f)
            tri = np.where(ids.reshape(-1, 4)[:, 1] != ABSENT, hit["prim"], ABSENT).astype(np.uint32)  # a light in front: not a triangle hit
            self.hits.append((tri, hit["u"].copy(), hit["v"].copy()))
        osc.close()
        self.camrec = oracle.pack_cameras(scene)[0]
        self.cam = T.camera_of(self.camrec)
        self.world = np.array([list(m.transform) for m in oracle.pack_instances(scene)[1]], dtype=f32)
        self.node_world = oracle.world_transforms(scene)

    def history(self):
        return T.History(np.concatenate([self.C[..., :3], np.full(self.C.shape[:2] + (1,), f32(self.n))], axis=-1), self.Pm, self.I,
                         self.cam, self.world)


_FRAMES = {}


def frames_of(oracle, base_name, edit, cam, frames):
    """cached Frames of a base scene, edited or not (edit None), seen through camera `cam`"""
    key = (base_name, edit, cam, frames)
    if key not in _FRAMES:
        base = base_of(base_name)
        scene = base.scene if edit is None else E.apply_to_scene(base.scene, E.edit_ops(edit, base.scene)[0])
        _FRAMES[key] = Frames(oracle, base, viewed(scene, cam), frames)
    return _FRAMES[key]


def hit_mask(fr):
    return (fr.I[..., 1] != ABSENT) & (fr.Pm[..., 3] > 0)


# ---- CPU tier: motion against float64 ------------------------------------------------------------------------------------------------
MOTION_CASES = [("cornell", "E1-move-mesh-node", 0), ("cornell", "E3-move-camera-1", 1), ("cornell", "E1-move-mesh-node", 1),
                ("cornell", "E1-move-mesh-node", 2), ("textured", "E1-move-mesh-node", 0)]


@pytest.mark.parametrize("case", MOTION_CASES, ids=lambda c: f"{c[0]}-{c[1]}-cam{c[2]}")
def test_motion_agrees_with_the_float64_model(oracle, case):
    """A moved mesh node (E1; in cornell it is short_copy_1, one of three nodes that reference mesh 1: an instanced node), a moved
    thin-lens camera (E3 through camera 1), the moved node seen through the thin-lens and the orthographic camera (cornell cameras 1 and
    2), a textured scene.  On every pixel whose four samples hit one triangle the twin's motion equals the float64 model's: the same surface
    points placed under the pre-edit node transforms and projected through the pre-edit camera.

    Measured on the CPU (pixels compared / of them moved by more than 0.05 px / largest motion / largest |difference|):
      cornell E1 cam0   917 / 15 /  0.73 px / 3.8e-6 px      cornell E3 cam1   865 / 865 / 2.14 px / 7.3e-6 px
      cornell E1 cam1   875 / 17 /  1.04 px / 5.6e-6 px      cornell E1 cam2   720 /   8 / 0.27 px / 3.8e-6 px
      textured E1 cam0  703 / 76 / 12.03 px / 5.7e-6 px
    Largest 7.3e-6 px; the bound asserted is MOTION_BOUND = 1e-4 px (at least 4 x the measurement, at most 0.01 px).  The random base is
    not here: its moved object is tessellated so finely that at 48 x 36 no pixel on it has four samples in one triangle (776 pixels
    compared, none of them moved); the GPU tier runs it against the twin."""
    b, e, cam = case
    prev, cur = frames_of(oracle, b, None, cam, 3), frames_of(oracle, b, e, cam, 4)
    _, M = T.resolve(cur.C, cur.Pm, cur.I, cur.n, prev.history(), cur.cam, cur.world, params=WIDE)
    model, points, same = T.model_motion(prev.scene, cur.scene, prev.node_world, cur.node_world, prev.camrec, cur.camrec, cur.hits, cur.w, cur.h)
    M = M.reshape(-1, 4)
    sel = same & (M[:, 3] == 1.0)
    assert sel.sum() > 0.5 * hit_mask(cur).sum(), "most hit pixels are compared"
    # the model's surface points are image 4's (float32 against float64 of the same points)
    pw = cur.Pm.reshape(-1, 4)[sel, :3] / cur.Pm.reshape(-1, 4)[sel, 3:4]
    assert np.abs(pw - points[sel]).max() <= 1e-4 * max(1.0, np.abs(points[sel]).max())
    dev = np.abs(M[sel, :2].astype(np.float64) - model[sel])
    moved = int((np.abs(model[sel]).max(axis=-1) > 0.05).sum())
    print(f"{case}: {int(sel.sum())} pixels compared, {moved} moved, largest motion {np.abs(model[sel]).max():.3f} px, largest deviation {dev.max():.3e} px")
    assert moved >= 5, "the edit moves something the camera sees"
    assert dev.max() <= MOTION_BOUND, dev.max()


def test_static_frame_reprojects_onto_itself_exactly(oracle):
    """no edit, static camera: motion is exactly 0 on every hit pixel and T is the closed form (H h + C n) / (h + n) bit for bit"""
    for cam in (0, 1, 2):
        prev, cur = frames_of(oracle, "cornell", None, cam, 3), frames_of(oracle, "cornell", None, cam, 2)
        Tm, M = T.resolve(cur.C, cur.Pm, cur.I, cur.n, prev.history(), cur.cam, cur.world, params=WIDE)
        hit = hit_mask(cur)
        assert hit.sum() > 1000
        assert (M[hit][:, :2] == 0).all() and (M[hit][:, 3] == 1).all() and (M[~hit] == 0).all()
        h, n = f32(prev.n), f32(cur.n)
        closed = ((prev.C[..., :3] * h).astype(f32) + (cur.C[..., :3] * n).astype(f32)).astype(f32) / f32(h + n)
        took = Tm[..., 3] == f32(h + n)
        assert took.sum() > 0.9 * hit.sum(), (cam, took.sum(), hit.sum())
        assert not took[~hit].any()
        assert Tm[took][:, :3].tobytes() == closed.astype(f32)[took].tobytes()
        rest = ~took
        assert Tm[rest].tobytes() == np.concatenate([cur.C[..., :3], np.full(cur.C.shape[:2] + (1,), n)], axis=-1)[rest].tobytes()


def test_orthographic_camera_shifted_by_whole_pixels(oracle):
    """camera 2 (orthographic) moved along its own x axis by exactly k pixel pitches: motion is (+k, 0) to the measured bound and interior
    pixels take the history of pixel x + k"""
    base = base_of("cornell")
    k = 3
    s2 = viewed(base.scene, 2)
    node = next(i for i, nd in enumerate(s2.nodes) if nd.camera_index == 0)
    pitch = 2.0 * s2.cameras[0].xmag / base.kw["width"]
    shift = np.eye(4, dtype=f32)
    shift[0, 3] = k * pitch
    moved = E.apply_to_scene(s2, [("node", node, np.asarray(s2.nodes[node].local_transform, f32) @ shift)])
    prev, cur = Frames(oracle, base, s2, 3), Frames(oracle, base, moved, 2)
    assert prev.cam.type == 1
    hist = prev.history()
    Tm, M = T.resolve(cur.C, cur.Pm, cur.I, cur.n, hist, cur.cam, cur.world, params=WIDE)
    hit = hit_mask(cur)
    assert np.abs(M[hit][:, 0] - k).max() <= MOTION_BOUND and np.abs(M[hit][:, 1]).max() <= MOTION_BOUND
    took = Tm[..., 3] > cur.n
    took[:, -k:] = False
    assert took.sum() > 0.6 * hit.sum()
    Hs = np.roll(hist.Hc, -k, axis=1)  # Hs[y, x] = Hc[y, x + k]
    h, n = Hs[..., 3], f32(cur.n)
    want = (Hs[..., :3] * h[..., None] + cur.C[..., :3] * n) / (h + n)[..., None]
    assert np.allclose(Tm[took][:, :3], want[took], rtol=1e-3, atol=1e-6)
    assert np.allclose(Tm[took][:, 3], (h + n)[took], rtol=1e-3)


def test_uncovered_background_starts_without_history(oracle):
    """a moved object uncovers what was behind it: those pixels see a static surface whose history pixel shows the object"""
    prev, cur = frames_of(oracle, "cornell", None, 0, 3), frames_of(oracle, "cornell", "E1-move-mesh-node", 0, 4)
    Tm, M = T.resolve(cur.C, cur.Pm, cur.I, cur.n, prev.history(), cur.cam, cur.world, params=WIDE)
    moved_inst = [i for i in range(len(cur.world)) if cur.world[i].tobytes() != prev.world[i].tobytes()]
    assert len(moved_inst) == 1
    uncovered = (prev.I[..., 1] == moved_inst[0]) & (cur.I[..., 1] != moved_inst[0]) & hit_mask(cur)
    assert uncovered.sum() > 10
    assert (Tm[uncovered][:, 3] == cur.n).all()
    assert Tm[uncovered][:, :3].tobytes() == cur.C[uncovered][:, :3].tobytes()
    assert (M[uncovered][:, :2] == 0).all()  # the wall itself did not move
    static = (cur.I[..., 1] != moved_inst[0]) & (prev.I[..., 1] == cur.I[..., 1]) & hit_mask(cur)
    assert (Tm[static][:, 3] > cur.n).mean() > 0.8


@pytest.mark.parametrize("edit", ["E4-deform-shared", "E5-glass-to-diffuse"])
def test_marked_instances_and_materials_start_without_history(oracle, edit):
    base = base_of("cornell")
    prev, cur = frames_of(oracle, "cornell", None, 0, 3), frames_of(oracle, "cornell", edit, 0, 2)
    im, mm = T.marks_of(base.scene, E.edit_ops(edit, base.scene)[0])
    assert im.any() != mm.any()
    Tm, M = T.resolve(cur.C, cur.Pm, cur.I, cur.n, prev.history(), cur.cam, cur.world, im, mm, params=WIDE)
    hit = hit_mask(cur)
    marked = hit & (im[np.minimum(cur.I[..., 1], len(im) - 1)] | mm[np.minimum(cur.I[..., 2], len(mm) - 1)])
    assert marked.sum() > 20
    assert (Tm[marked][:, 3] == cur.n).all() and (M[marked] == 0).all()
    assert Tm[marked][:, :3].tobytes() == cur.C[marked][:, :3].tobytes()
    assert (Tm[hit & ~marked][:, 3] > cur.n).mean() > 0.8  # everything else keeps its history
    plain, _ = T.resolve(cur.C, cur.Pm, cur.I, cur.n, prev.history(), cur.cam, cur.world, params=WIDE)
    assert (plain[marked][:, 3] > cur.n).any()  # ... which the marks took away


def test_singular_transform_starts_without_history(oracle):
    """E9 squashes the shared node flat: W_cur is singular, D undefined, the instance counts as marked.  The same on the unedited frame
    with the singular transform handed in, where the instance is sure to be seen"""
    base = base_of("cornell")
    prev, cur = frames_of(oracle, "cornell", None, 0, 3), frames_of(oracle, "cornell", "E9-singular", 0, 2)
    flat = [i for i in range(len(cur.world)) if cur.world[i].tobytes() != prev.world[i].tobytes()]
    assert len(flat) == 1
    D, ok = T.motion_matrix(prev.world[flat[0]], cur.world[flat[0]])
    assert not ok and D.tobytes() == np.eye(4, dtype=f32)[:3].tobytes()
    Tm, M = T.resolve(cur.C, cur.Pm, cur.I, cur.n, prev.history(), cur.cam, cur.world, params=WIDE)
    seen = hit_mask(cur) & (cur.I[..., 1] == flat[0])
    assert (Tm[seen][:, 3] == cur.n).all() and (M[seen] == 0).all()
    still = frames_of(oracle, "cornell", None, 0, 2)
    Tm, M = T.resolve(still.C, still.Pm, still.I, still.n, prev.history(), still.cam, cur.world, params=WIDE)
    seen = hit_mask(still) & (still.I[..., 1] == flat[0])
    assert seen.sum() > 20
    assert (Tm[seen][:, 3] == still.n).all() and (M[seen] == 0).all()
    assert (Tm[hit_mask(still) & ~seen][:, 3] > still.n).mean() > 0.8
    # invertible transforms: D . W_cur = W_prev
    e1 = frames_of(oracle, "cornell", "E1-move-mesh-node", 0, 4)
    i = next(i for i in range(len(e1.world)) if e1.world[i].tobytes() != prev.world[i].tobytes())
    D, ok = T.motion_matrix(prev.world[i], e1.world[i])
    assert ok
    D4 = np.vstack([D.astype(np.float64), [0, 0, 0, 1]])
    Wp, Wc = (w.astype(np.float64).reshape(4, 4).T for w in (prev.world[i], e1.world[i]))
    assert np.abs(D4 @ Wc - Wp).max() <= 1e-4 * np.abs(Wp).max()


def test_point_behind_the_captured_camera_has_no_history(oracle):
    prev, cur = frames_of(oracle, "cornell", None, 0, 3), frames_of(oracle, "cornell", None, 0, 2)
    hist = prev.history()
    back = T.Camera(hist.cam.position, -hist.cam.right, hist.cam.up, -hist.cam.forward, hist.cam.tan_half, hist.cam.xmag, hist.cam.ymag, 0)
    hist = T.History(hist.Hc, hist.Hp, hist.Hi, back, hist.world)
    Tm, M = T.resolve(cur.C, cur.Pm, cur.I, cur.n, hist, cur.cam, cur.world, params=WIDE)
    assert hit_mask(cur).sum() > 1000
    assert (Tm[..., 3] == cur.n).all() and (M == 0).all()
    assert Tm[..., :3].tobytes() == cur.C[..., :3].tobytes()


def test_max_history_clamps(oracle):
    prev, cur = frames_of(oracle, "cornell", None, 0, 3), frames_of(oracle, "cornell", None, 0, 2)
    hist = prev.history()
    hist.Hc[..., 3] = 1000.0
    Tm, _ = T.resolve(cur.C, cur.Pm, cur.I, cur.n, hist, cur.cam, cur.world, params=T.Params(max_history=8.0, tol=0.2))
    took = Tm[..., 3] > cur.n
    assert took.sum() > 1000 and (Tm[took][:, 3] == 8.0 + cur.n).all()
    closed = ((prev.C[..., :3] * f32(8.0)).astype(f32) + (cur.C[..., :3] * f32(cur.n)).astype(f32)).astype(f32) / f32(8.0 + cur.n)
    assert Tm[took][:, :3].tobytes() == closed.astype(f32)[took].tobytes()
    free, _ = T.resolve(cur.C, cur.Pm, cur.I, cur.n, hist, cur.cam, cur.world, params=T.Params(max_history=2048.0, tol=0.2))
    assert (free[took][:, 3] == 1000.0 + cur.n).all()


def test_capture_without_samples_keeps_the_history(oracle):
    prev = frames_of(oracle, "cornell", None, 0, 3)
    hist = prev.history()
    assert T.capture(prev.C, prev.Pm, prev.I, 0, hist, prev.cam, prev.world) is hist
    first = T.capture(prev.C, prev.Pm, prev.I, prev.n, None, prev.cam, prev.world)
    assert first.Hc.tobytes() == hist.Hc.tobytes()  # no history before: T = (C, n)


# ---- CPU tier: parameters, header -----------------------------------------------------------------------------------------------------
NEW_FUNCTIONS = ["hala_temporal_default_params", "hala_rt_set_temporal", "hala_rt_temporal_capture", "hala_rt_temporal_resolve",
                 "hala_rt_read_temporal", "hala_rt_get_temporal_buffer", "hala_rt_denoise_temporal"]


def test_header_declares_and_library_exports_the_entry_points(halart):
    raw = open(os.path.join(ROOT, "include", "halart.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = C.CDLL(halart.LIB_PATH)
    for name in NEW_FUNCTIONS:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in A.EXPORTS, name
        assert hasattr(lib, name), name
        if name.startswith("hala_rt_"):
            m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int " + name + r"\(", raw, flags=re.S)
            assert m and "RENDER_SPEC 16" in m.group(1), f"{name} cites its section of the spec"


def test_temporal_params_layout_and_defaults(halart):
    assert C.sizeof(A.TemporalParams) == 32
    offsets = {f: getattr(A.TemporalParams, f).offset for f, _ in A.TemporalParams._fields_}
    assert offsets == {"max_history": 0, "tol": 4, "min_weight": 8, "reserved": 12}
    assert re.search(r"\}\s*hala_temporal_params;\s*/\*\s*32 B", open(os.path.join(ROOT, "include", "halart.h")).read())
    p = halart.temporal_default_params()
    d = T.Params()
    assert (p.max_history, p.tol, p.min_weight, list(p.reserved)) == (f32(d.max_history), f32(d.tol), f32(d.min_weight), [0] * 5)
    assert T.check_params(p.max_history, p.tol, p.min_weight) == ""


BAD_PARAMS = [("max_history", 0.5), ("max_history", math.nan), ("max_history", math.inf), ("max_history", -4.0), ("max_history", 2.0 ** 21),
              ("tol", 0.0), ("tol", -1.0), ("tol", math.nan), ("tol", 1.5), ("min_weight", 0.0), ("min_weight", 1.25), ("min_weight", math.nan)]


@pytest.mark.parametrize("field,value", BAD_PARAMS)
def test_invalid_params_are_refused_before_any_device_call(halart, field, value):
    lib = halart.load_library()
    p = halart.temporal_default_params(**{field: value})
    want = T.check_params(p.max_history, p.tol, p.min_weight)
    assert field in want
    assert lib.hala_rt_set_temporal(None, C.byref(p)) == 1  # validated before the renderer handle is looked at
    assert halart.last_error() == want


def test_reserved_words_and_null_handle_are_refused(halart):
    lib = halart.load_library()
    p = halart.temporal_default_params()
    p.reserved[3] = 1
    assert lib.hala_rt_set_temporal(None, C.byref(p)) == 1 and halart.last_error() == T.check_params(32, 0.05, 0.25, (0, 0, 0, 1, 0))
    p = halart.temporal_default_params()
    for call in (lambda: lib.hala_rt_set_temporal(None, C.byref(p)), lambda: lib.hala_rt_set_temporal(None, None),
                 lambda: lib.hala_rt_temporal_capture(None), lambda: lib.hala_rt_temporal_resolve(None, None),
                 lambda: lib.hala_rt_read_temporal(None, 0, None), lambda: lib.hala_rt_get_temporal_buffer(None, 0, None, None)):
        assert call() == 1 and "null" in halart.last_error()


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------------------
def make(halart, base, build=None, views=None):
    kw = base.kw
    r = halart.HalaRenderer("temporal", kw["width"], kw["height"], kw["max_depth"], kw["rr_depth"], *kw["tonemap"], 0)
    if build is not None:
        r.set_build_options(**build)
    if base.env is not None:
        r.set_envmap(base.env, kw["env_rotation"])
        r.set_env_intensity(kw["env_intensity"])
    r.set_exposure_value(kw["exposure"])
    r.set_scene(base.scene)
    r.commit()
    if views is not None:
        r.set_views(views)
    r.set_aovs(position=True, ids=True)
    return r


class Twin:
    """the renderer's temporal state, mirrored from its read-backs with the numpy twin"""

    def __init__(self, r, scene, cam=0, params=T.Params()):
        self.r, self.scene, self.cam, self.params, self.hist = r, scene, cam, params, None
        self.clear_marks()

    def clear_marks(self):
        self.im, self.mm = T.marks_of(self.scene, [])

    def mark(self, ops):
        im, mm = T.marks_of(self.scene, ops)
        self.im |= im
        self.mm |= mm

    def state(self):
        r = self.r
        world = np.array([list(m.transform) for m in r.packed_primitives()[0]], dtype=f32)
        return dict(C=r.read_image(0), Pm=r.read_image(4), I=r.read_ids(), n=int(r.statistics().total_frames), cam_cur=T.camera_of(r.packed_cameras()[self.cam]),
                    world_cur=world)

    def resolve(self):
        return T.resolve(hist=self.hist, inst_marked=self.im, mat_marked=self.mm, material_count=len(self.scene.materials), params=self.params,
                         **self.state())

    def capture(self):
        self.hist = T.capture(hist=self.hist, inst_marked=self.im, mat_marked=self.mm, material_count=len(self.scene.materials),
                              params=self.params, **self.state())
        self.clear_marks()


def assert_same(got, want, what):
    if got.tobytes() != want.tobytes():
        bad = np.any(got.reshape(-1, 4).view(np.uint32) != want.reshape(-1, 4).view(np.uint32), axis=-1)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} pixels differ, first at {np.nonzero(bad)[0][:5]}")


def check_resolve(r, twin, what):
    r.temporal_resolve()
    want_t, want_m = twin.resolve()
    assert_same(r.read_temporal(0), want_t, f"{what}: temporal")
    assert_same(r.read_temporal(1), want_m, f"{what}: motion")
    return want_t, want_m


def edit_round(r, twin, ops, render):
    """capture -> edit -> refit -> render, on the renderer and on the twin"""
    r.temporal_capture()
    twin.capture()
    E.apply_to_renderer(r, ops)
    twin.mark(ops)
    r.refit()
    render(r)


def gpu_cases():
    """scenes x edits of the issue, on both tree forms where the scene has a mesh that several nodes reference: cornell and random.
    textured (one blob, one ground plane, no shared mesh) has nothing to instance and runs on the one-level tree only."""
    out = []
    for b, edits in (("cornell", ("E1-move-mesh-node", "E3-move-camera-1", "E4-deform-shared", "E5-glass-to-diffuse", "E9-singular")),
                     ("random", ("E1-move-mesh-node", "E4-deform-shared")), ("textured", ("E1-move-mesh-node",))):
        forms = (False, True) if E.shared_mesh(base_of(b).scene) is not None else (False,)
        out += [(b, e, two) for e in edits for two in forms]
    return out


GPU_CASES = gpu_cases()


@gpu
@pytest.mark.parametrize("case", GPU_CASES, ids=lambda c: f"{c[0]}-{c[1]}-{'two_level' if c[2] else 'one_level'}")
def test_kernel_equals_the_twin_after_an_edit(halart, oracle, case):
    """5 frames, capture, the edit, refit, update_batch(4): both output images equal the twin's byte for byte, on both tree forms (E3 is
    seen through view {1}); a second resolve after one more update equals it again, and a capture + resolve with no edit too"""
    b, e, two_level = case
    base = base_of(b)
    cam = E.EDITS[e].camera
    fwd, _ = E.edit_ops(e, base.scene)
    r = make(halart, base, build=dict(instancing=True) if two_level else dict(instancing=False), views=[cam] if cam else None)
    try:
        assert (r.bvh_info().instance_ref_count > 0) == two_level
        r.set_temporal()
        twin = Twin(r, base.scene, cam)
        r.update_batch(5)
        check_resolve(r, twin, f"{case} before any capture")
        edit_round(r, twin, fwd, lambda r: r.update_batch(4))
        t, m = check_resolve(r, twin, f"{case} after the edit")
        n = 4
        assert (t[..., 3] > n).any(), "some pixels carry history"
        if e in ("E1-move-mesh-node", "E3-move-camera-1"):
            assert (np.abs(m[..., :2]).max(axis=-1) > 0.05).sum() > 20, "something moved"
        r.update()
        check_resolve(r, twin, f"{case} one update later")
    finally:
        r.close()


@gpu
def test_kernel_equals_the_twin_on_an_odd_frame_with_single_updates(halart):
    base = E.cornell(61, 37)
    fwd, _ = E.edit_ops("E1-move-mesh-node", base.scene)
    r = make(halart, base)
    try:
        r.set_temporal(max_history=6.0, tol=0.05, min_weight=0.5)
        twin = Twin(r, base.scene, params=T.Params(6.0, 0.05, 0.5))
        for _ in range(9):
            r.update(); r.render()
        edit_round(r, twin, fwd, lambda r: [r.update() for _ in range(3)])
        t, _ = check_resolve(r, twin, "61 x 37")
        assert (t[..., 3] == 6.0 + 3).any(), "max_history clamps the 9 captured samples"
    finally:
        r.close()


@gpu
def test_resolve_directly_behind_an_update(halart):
    """no wait between update() and the resolve: the resolve goes behind the open tail, whose k_resolve still folds the images it reads"""
    base = base_of("cornell")
    fwd, _ = E.edit_ops("E1-move-mesh-node", base.scene)
    r = make(halart, base)
    try:
        r.set_launch_timing_period(0)  # untimed updates: the ones that leave their tail open
        r.set_temporal()
        twin = Twin(r, base.scene)
        r.update_batch(3)
        edit_round(r, twin, fwd, lambda r: r.update_batch(2))
        check_resolve(r, twin, "first resolve (uploads the table)")
        for k in range(3):
            r.update()
            r.temporal_resolve()  # straight behind the update
            want_t, want_m = twin.resolve()  # (the read-backs in here wait)
            assert_same(r.read_temporal(0), want_t, f"tail overlap {k}: temporal")
            assert_same(r.read_temporal(1), want_m, f"tail overlap {k}: motion")
        r.update()
        r.temporal_capture()  # the same for a capture
        twin.capture()
        r.update()
        check_resolve(r, twin, "after a capture behind an update")
    finally:
        r.close()


@gpu
@pytest.mark.parametrize("two_level", [False, True])
def test_chain_of_three_captures(halart, two_level):
    """capture -> edit -> render three times over: each history is the resolve of the one before"""
    base = base_of("cornell")
    e1, e1_back = E.edit_ops("E1-move-mesh-node", base.scene)
    e5, _ = E.edit_ops("E5-glass-to-diffuse", base.scene)
    r = make(halart, base, build=dict(instancing=two_level))
    try:
        r.set_temporal()
        twin = Twin(r, base.scene)
        r.update_batch(6)
        lengths = []
        for k, ops in enumerate((e1, e1_back, e5)):
            edit_round(r, twin, ops, lambda r: r.update_batch(2))
            t, _ = check_resolve(r, twin, f"round {k}")
            lengths.append(float(t[..., 3].max()))
        assert lengths[0] == 6 + 2 and lengths[1] == 6 + 2 + 2 and lengths[2] == 6 + 2 + 2 + 2, lengths
        r.temporal_capture(); twin.capture()
        r.temporal_capture(); twin.capture()  # twice: the second folds the same samples again (RENDER_SPEC 16 "Capture")
        E.apply_to_renderer(r, e1); r.refit()
        r.temporal_capture(); twin.capture()  # n = 0: nothing happens
        r.update()
        check_resolve(r, twin, "after captures without frames")
    finally:
        r.close()


@gpu
def test_images_and_statistics_do_not_change_with_the_feature_on(halart):
    base = base_of("cornell")
    fwd, _ = E.edit_ops("E1-move-mesh-node", base.scene)
    got = []
    for on in (False, True):
        r = make(halart, base)
        try:
            if on:
                r.set_temporal()
            r.update_batch(3); r.update()
            if on:
                r.temporal_resolve(); r.temporal_capture()
            E.apply_to_renderer(r, fwd); r.refit()
            r.update_batch(2); r.update()
            if on:
                r.temporal_resolve(); r.denoise_temporal()
            st = r.statistics()
            got.append(([r.read_image(k).tobytes() for k in range(6)],
                        [getattr(st, f) for f in ("total_frames", "rays_total", "rays_closest_total", "rays_shadow_total", "rays_primary_total", "updates_rendered")]))
        finally:
            r.close()
    assert got[0][1] == got[1][1]
    for k in range(6):
        assert got[0][0][k] == got[1][0][k], f"image {k}"


@gpu
def test_denoise_temporal_equals_the_denoiser_twin(halart):
    base = base_of("cornell")
    fwd, _ = E.edit_ops("E1-move-mesh-node", base.scene)
    r = make(halart, base)
    try:
        r.set_temporal()
        with pytest.raises(halart.HalaRendererError, match="resolved"):
            r.denoise_temporal()
        r.update_batch(8)
        r.temporal_capture()
        E.apply_to_renderer(r, fwd); r.refit()
        r.update_batch(2)
        r.temporal_resolve()
        for p in (dict(), dict(iterations=3, sigma_color=0.2, demodulate=False)):
            ms = r.denoise_temporal(timed=True, **p)
            assert ms > 0
            d = H.denoise_default_params(**p)
            want = denoise_ref.denoise(r.read_temporal(0), r.read_image(1), r.read_image(2), iterations=d.iterations, sigma_color=d.sigma_color,
                                       sigma_albedo=d.sigma_albedo, normal_power=d.normal_power, demodulate=bool(d.demodulate))
            assert r.read_denoised().tobytes() == want.tobytes()
        ptr, nbytes = r.temporal_buffer(1)
        assert ptr and nbytes == base.kw["width"] * base.kw["height"] * 16
    finally:
        r.close()


@gpu
def test_refusals_leave_the_renderer_as_it_was(halart):
    base = base_of("cornell")
    Err = halart.HalaRendererError
    r = make(halart, base)
    try:
        for call in (r.temporal_capture, r.temporal_resolve, r.read_temporal):
            with pytest.raises(Err, match="off"):
                call()
        with pytest.raises(Err, match="tol"):
            r.set_temporal(tol=7.0)
        r.set_temporal()
        with pytest.raises(Err, match="no sample"):
            r.temporal_resolve()
        r.temporal_capture()  # no sample, no history: succeeds and changes nothing
        with pytest.raises(Err, match="resolved"):
            r.read_temporal()
        r.update_batch(2)
        before = [r.read_image(k).tobytes() for k in range(6)]
        # whichever is set second: several views, adaptive sampling, a shard
        with pytest.raises(Err, match="temporal"):
            r.set_views([0, 1])
        with pytest.raises(Err, match="temporal"):
            r.set_adaptive_sampling(0.05)
        with pytest.raises(Err, match="[Tt]emporal"):
            r.set_tile_shard(0, 2, 16)
        assert r.statistics().total_frames == 2 and [r.read_image(k).tobytes() for k in range(6)] == before
        r.temporal_resolve()
        first = r.read_temporal(0)
        assert first[..., :3].tobytes() == r.read_image(0)[..., :3].tobytes() and (first[..., 3] == 2).all()  # no history yet
        assert (r.read_temporal("motion") == 0).all()
        with pytest.raises(Err, match="selector"):
            r.read_temporal(2)
        # AOV bits 0 and 1 must both be on
        for pos, ids in ((True, False), (False, True), (False, False)):
            r.set_aovs(position=pos, ids=ids)
            r.update()
            with pytest.raises(Err, match="AOV"):
                r.temporal_resolve()
            with pytest.raises(Err, match="AOV"):
                r.temporal_capture()
        r.set_temporal(False)
        with pytest.raises(Err, match="off"):
            r.temporal_resolve()
        # the other order: the feature is refused on top of views / adaptive sampling / a shard
        r.set_aovs(True, True)
        r.set_views([0, 1])
        with pytest.raises(Err, match="views"):
            r.set_temporal()
        r.set_views([0])
        r.set_adaptive_sampling(0.05)
        with pytest.raises(Err, match="adaptive"):
            r.set_temporal()
        r.set_adaptive_sampling(None)
        r.set_aovs(False, False)
        r.set_tile_shard(0, 2, 16)
        with pytest.raises(Err, match="sharded"):
            r.set_temporal()
        r.set_tile_shard(0, 1, 32)
        r.set_aovs(True, True)
        r.set_temporal()
        r.update()
        r.temporal_resolve()
    finally:
        r.close()


@gpu
def test_history_is_dropped_by_commit_shard_and_aovs(halart):
    """(a renderer has no resize: its frame size is fixed at creation; set_tile_shard is the call that reallocates the frame)"""
    base = base_of("cornell")
    r = make(halart, base)
    try:
        r.set_temporal()

        def history_taken():
            r.update_batch(2)
            r.temporal_resolve()
            return bool((r.read_temporal(0)[..., 3] > 2).any())

        def capture_and_restart():
            r.update_batch(3)
            r.temporal_capture()
            r.reset_accumulation()

        capture_and_restart()
        assert history_taken(), "a plain restart keeps the history"
        for drop in (r.commit, lambda: r.set_tile_shard(0, 1, 32), lambda: (r.set_aovs(True, False), r.set_aovs(True, True)),
                     lambda: (r.set_scene(base.scene), r.commit()), lambda: (r.set_temporal(False), r.set_temporal())):
            r.reset_accumulation()
            capture_and_restart()
            drop()
            assert not history_taken()
    finally:
        r.close()


def g_space(x):
    x = np.asarray(x[..., :3], np.float64)
    lum = 0.212671 * x[..., 0] + 0.715160 * x[..., 1] + 0.072169 * x[..., 2]
    return x / (1.0 + lum)[..., None]


def quality_case(halart, hist_frames=64, new_frames=4, ref_frames=1024, **params):
    """cornell 48 x 36: hist_frames, capture, camera 0's node moves, new_frames, resolve.  -> MSE in g-space against ref_frames of the
    edited scene of: the accumulation, the temporal image, the blend without reprojection, denoise, denoise_temporal"""
    base = base_of("cornell")
    node = next(i for i, nd in enumerate(base.scene.nodes) if nd.camera_index == 0)
    move = np.asarray(base.scene.nodes[node].local_transform, f32) @ E._translate((0.04 * E._extent(base.scene), 0.0, 0.0)) @ E._rot(ry=0.05)
    r = make(halart, base)
    try:
        r.set_temporal(**params)
        p = halart.temporal_default_params(**params)
        twin = Twin(r, base.scene, params=T.Params(p.max_history, p.tol, p.min_weight))
        r.update_batch(hist_frames)
        r.temporal_capture(); twin.capture()
        r.update_node_transform(node, move); r.refit()
        r.update_batch(new_frames)
        r.temporal_resolve()
        temporal = r.read_temporal(0)
        st = twin.state()
        unprojected = T.History(twin.hist.Hc, twin.hist.Hp, twin.hist.Hi, st["cam_cur"], st["world_cur"])  # D = identity, the current camera
        plain, _ = T.resolve(hist=unprojected, params=twin.params, material_count=len(base.scene.materials), **st)
        accum = r.read_image(0)
        r.denoise(); dn = r.read_denoised()
        r.denoise_temporal(); dnt = r.read_denoised()
        r.update_batch(ref_frames - new_frames)
        ref = g_space(r.read_image(0))
    finally:
        r.close()
    mse = lambda x: float(np.mean((g_space(x) - ref) ** 2))  # noqa: E731
    return dict(accum=mse(accum), temporal=mse(temporal), unprojected=mse(plain), denoise=mse(dn), denoise_temporal=mse(dnt),
                carried=float((temporal[..., 3] > new_frames).mean()))


@gpu
def test_quality_after_a_camera_move(halart):
    """the three strict inequalities of the issue; DESIGN.md "Temporal reprojection" records the ratios"""
    q = quality_case(halart)
    print("quality:", q)
    assert q["temporal"] < q["accum"]
    assert q["temporal"] < q["unprojected"]
    assert q["denoise_temporal"] < q["denoise"]
