"""Occlusion batches (docs/RENDER_SPEC.md 4.10): hala_rt_occlusion against the numpy twin of tests/occlusion_ref.py, all 16 bytes of every
record and every mask word.

CPU tier: the ABI surface is there; the twin's occlusion bits come from the oracle's brute-force any-hit trace of the expanded batch; the
inputs are shown to be telling (shares of occluded rays, visibility 0 and 1, bent normals off the normal, translucent triangles that
matter); the twin is tied to float64 directions and a float64 Moeller-Trumbore over all triangles; a floor under a wall has the analytic
visibility 1/2; degenerate samples answer the invalid record; normals at the basis's singular end give finite directions.
GPU tier: every tree form (LDS-staged, large one-level, two-level) and the ALPHA variants with every builder and ray counts around the
mask word's size; the masks against the renderer's own any-hit batch; the Python forms, determinism and the global sample index; the
refusals; frames around a batch; refits.

Sample sets.  Per scene 257 samples (KINDS), shuffled so that every prefix mixes them: the first hits of the oracle's 16 x 16 camera rays
with the geometric normal (not normalised: the operator does that) turned towards the ray, bias = ray_eps and four kinds of reach; some of
them with a normal tilted 70 degrees off the surface's; the same hits with the normal turned away (the origin goes behind the surface);
exact vertices, with a triangle's normal; points 10^-3 triangle sizes in front of a triangle and facing it; the degenerate samples;
valid samples whose reach admits nothing; points at 10^2 and 10^4 scene diagonals.  N <= 64 runs all 257, N = 256 the first 64: the queue
then ends inside a wave and inside a mask word.  The conditions and the float64 comparison run on (257, N = 64) and (64, N = 256) of
every scene.

Float64, measured (CPU tier, GRAZING_SHARE below and RENDER_SPEC 4.10): of the 164 160 rays of those ten sets 389 answer differently, all
of them rays of the exact-vertex samples of the three box scenes (cornell 13 and 17, two_level 267 and 91, cornell_alpha 1 and 0): a
box's vertex moved by ray_eps along one face's normal still lies in the planes of the two adjacent faces, so whether those faces are hit
at t > 0 is decided by the last bit.  No ray of any other kind of sample differs, and none on the blob or the sheets.
"""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest

import closest_point_ref as CR
import deform_ref as DR
import hala_renderer_amd as H
import occlusion_ref as OR
import ray_conditioning as RC
import scene_edits as SE
from aov_ref import cross, dot, fma
from first_hit_ref import pcg
from hala_renderer_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = H._abi
f32, f64 = np.float32, np.float64
M32 = np.uint64(0xFFFFFFFF)
MISS = 0xFFFFFFFF
FLT_MAX = f32(3.402823466e38)
FUNCTIONS = ("hala_rt_occlusion", "hala_rt_occlusion_host")
BUILDERS = ("sah", "ploc", "lbvh")
RAY_COUNTS = (1, 31, 32, 33, 64, 256)
SEED = 7
# rays whose float64 outcome differs from the twin's, per set, as measured (module docstring); asserted at twice that
GRAZING_SHARE = {("cornell", 64): 13 / 16448, ("cornell", 256): 17 / 16384, ("blob", 64): 0.0, ("blob", 256): 0.0, ("sheets512", 64): 0.0,
                 ("sheets512", 256): 0.0, ("two_level", 64): 267 / 16448, ("two_level", 256): 91 / 16384, ("cornell_alpha", 64): 1 / 16448,
                 ("cornell_alpha", 256): 0.0}


def count_for(n_rays):
    return 257 if n_rays <= 64 else 64


def translucent_cornell(block_opacity=0.5):
    """the Cornell box with the blocks' material at opacity 0.5 (translucent) and the red wall's at 0 (invisible)"""
    s = scenes.cornell_box()
    s.materials[4].opacity = block_opacity
    s.materials[1].opacity = 0.0
    return s


def two_instances():
    from test_instance_levels import instance_scene
    return instance_scene(2, True)


SCENES = {  # name -> (scene, tree form)
    "cornell": (scenes.cornell_box, "staged"),
    "blob": (lambda: RC.blob_scene(3), "large"),
    "sheets512": (lambda: scenes.stacked_sheets(512), "large"),
    "two_level": (two_instances, "two_level"),
    "cornell_alpha": (translucent_cornell, "staged"),
}


def oracle_scene(oracle, scene, two_level):
    oracle.set_instancing(bool(two_level))
    try:
        return oracle.OracleScene(scene)
    finally:
        oracle.set_instancing(False)


def scene_diag(osc):
    mn, mx = osc.bounds()
    ext = (mx - mn).astype(f32)
    return f32(np.sqrt(dot(ext, ext)))


def ray_eps(osc):
    """RENDER_SPEC 3"""
    return f32(scene_diag(osc) * f32(1e-5))


def _unit(v):
    v = np.asarray(v, dtype=f64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def far_samples(osc, count, decade, rs):
    """points at 10^decade scene diagonals around the box, normals (not normalised) aimed at a point of the box, reach +inf"""
    mn, mx = (x.astype(f64) for x in osc.bounds())
    diag = float(scene_diag(osc))
    p = 0.5 * (mn + mx) + _unit(rs.normal(size=(count, 3))) * diag * 10.0 ** decade
    target = rs.uniform(mn, mx, (count, 3))
    s = np.zeros(count, dtype=A.OCCLUSION_SAMPLE_DTYPE)
    s["point"], s["normal"], s["bias"], s["reach"] = p.astype(f32), (target - p).astype(f32), 0.0, np.inf
    return s


KINDS = ("first hit", "tilted normal", "behind the surface", "vertex", "facing a triangle", "degenerate", "no reach", "far")


def surface_samples(scene, osc, seed):
    """the 257 samples of a scene (module docstring) and the index into KINDS of each"""
    rs = np.random.RandomState(seed)
    v0, e1, e2 = CR.scene_triangles(scene, osc)
    ng = cross(e1, e2).astype(f32)
    diag, eps = scene_diag(osc), ray_eps(osc)
    cam = osc.camera_rays(16, 16, 0)
    hits = osc.trace(cam, 0, brute=True)
    found = np.nonzero(hits["prim"] != MISS)[0]
    assert len(found) >= 16, "the camera sees the scene"

    def make(n):
        return np.zeros(n, dtype=A.OCCLUSION_SAMPLE_DTYPE)

    def first_hits(n, towards):
        k = found[rs.randint(0, len(found), n)]
        d, o, t = cam["direction"][k], cam["origin"][k], hits["t"][k]
        n_g = ng[hits["prim"][k]]
        facing = dot(n_g, d) < 0
        s = make(n)
        s["point"] = fma(d, t[:, None], o)
        s["normal"] = np.where((facing == towards)[:, None], n_g, -n_g)
        s["bias"] = eps
        return s

    a = first_hits(120, True)
    a["reach"] = np.array([np.inf, FLT_MAX, f32(0.3) * diag, f32(0.05) * diag], f32)[np.arange(120) % 4]
    # 20 of them with a normal tilted 70 degrees off the surface's (a shading normal that disagrees with the geometry): the surface itself
    # hides part of the hemisphere and the bent normal leans away from it
    tilt = a["normal"][100:].astype(f64)
    side = np.cross(tilt, rs.normal(size=tilt.shape))
    a["normal"][100:] = (np.cos(np.radians(70.0)) * _unit(tilt) + np.sin(np.radians(70.0)) * _unit(side)).astype(f32)
    a["reach"][100:] = np.inf
    b = first_hits(40, False)
    b["reach"] = np.inf
    c = make(40)
    k = rs.randint(0, len(v0), 40)
    corner = rs.randint(0, 3, 40)
    c["point"] = np.where((corner == 0)[:, None], v0[k], np.where((corner == 1)[:, None], (v0[k] + e1[k]).astype(f32), (v0[k] + e2[k]).astype(f32)))
    c["normal"] = ng[k] * np.where(rs.randint(0, 2, 40) == 0, f32(1.0), f32(-1.0))[:, None]
    c["bias"], c["reach"] = eps, np.inf
    d_ = make(16)  # in front of a triangle's centroid, 10^-3 of its size away, facing it
    big = np.argsort(-dot(ng, ng))[: max(len(v0) // 2, 1)]
    k = big[rs.randint(0, len(big), 16)]
    size = np.sqrt(np.sqrt(dot(ng[k], ng[k]).astype(f64)))
    centre = v0[k].astype(f64) + (e1[k].astype(f64) + e2[k].astype(f64)) / 3.0
    d_["point"] = (centre + _unit(ng[k]) * (1e-3 * size)[:, None]).astype(f32)
    d_["normal"], d_["bias"], d_["reach"] = -ng[k], 0.0, np.inf
    e = degenerate_samples(first_hits(21, True))
    g = first_hits(6, True)
    g["reach"] = np.array([np.nan, 0.0, -1.0, -np.inf, -0.0, np.nan], f32)
    f = np.concatenate([far_samples(osc, 7, 2, rs), far_samples(osc, 7, 4, rs)])
    out = np.concatenate([a, b, c, d_, e, g, f])
    kinds = np.repeat(np.arange(len(KINDS)), [100, 20, 40, 40, 16, 21, 6, 14])
    assert len(out) == len(kinds) == 257
    order = rs.permutation(len(out))
    return out[order], kinds[order]


def degenerate_samples(valid):
    """21 valid samples made invalid, three of each kind: a zero, a NaN, an infinite and an overflowing normal; a NaN and an infinite point; a
    non-finite bias"""
    s = valid.copy()
    assert len(s) == 21
    for k in range(3):
        s["normal"][k] = (0.0, 0.0, -0.0)
        s["normal"][3 + k][k] = np.nan
        s["normal"][6 + k][k] = (np.inf, -np.inf, np.inf)[k]
        s["normal"][9 + k] = (3e19, 3e19, 3e19)  # finite, but nn overflows to +inf
        s["point"][12 + k][k] = np.nan
        s["point"][15 + k][k] = (-np.inf, np.inf, np.inf)[k]
        s["bias"][18 + k] = (np.nan, np.inf, -np.inf)[k]
    return s


class Reference:
    pass


_SCENE_REF, _REF = {}, {}


def scene_ref(oracle, name):
    """scene, oracle scene, its triangles and the 257 samples: once per scene"""
    if name not in _SCENE_REF:
        ref = Reference()
        ref.scene = SCENES[name][0]()
        ref.osc = oracle_scene(oracle, ref.scene, SCENES[name][1] == "two_level")
        ref.samples, ref.kinds = surface_samples(ref.scene, ref.osc, 500 + list(SCENES).index(name))
        _SCENE_REF[name] = ref
    return _SCENE_REF[name]


def twin_answer(osc, samples, n_rays, seed, first=0):
    """(records, masks, occlusion bits) of the twin, the bits from the oracle's brute-force any-hit trace of the expanded batch"""
    rays, _ = OR.expand(samples, n_rays, seed, first)
    occluded = (osc.trace(rays, 1, brute=True)["t"] > 0).reshape(len(samples), n_rays)
    rec, masks = OR.reduce(samples, n_rays, seed, occluded, first)
    return rec, masks, occluded


def reference(oracle, name, n_rays):
    """the twin's answer for (scene, N): computed once, shared by every test and left unchanged"""
    if (name, n_rays) not in _REF:
        base = scene_ref(oracle, name)
        ref = Reference()
        ref.scene, ref.osc = base.scene, base.osc
        ref.samples, ref.kinds = base.samples[: count_for(n_rays)], base.kinds[: count_for(n_rays)]
        ref.rec, ref.masks, ref.occluded = twin_answer(ref.osc, ref.samples, n_rays, SEED)
        _REF[(name, n_rays)] = ref
    return _REF[(name, n_rays)]


CONDITION_SETS = [(name, n) for name in SCENES for n in (64, 256)]


def unit_normals(samples):
    with np.errstate(all="ignore"):
        return _unit(samples["normal"].astype(f64))


def check_conditions(oracle, name, n_rays):
    """what a set must show before a comparison on it means something"""
    ref = reference(oracle, name, n_rays)
    ok = ref.rec["visibility"] >= 0
    share = float(ref.occluded[ok].mean())
    vis = ref.rec["visibility"][ok]
    partly = ok & (ref.rec["visibility"] > 0)
    off = (ref.rec["bent"][partly].astype(f64) * unit_normals(ref.samples[partly])).sum(axis=1)
    out = dict(occluded=share, fully_occluded=int((vis == 0).sum()), fully_clear=int((vis == 1).sum()), bent_off_normal=int((off < 0.95).sum()),
               invalid=int((~ok).sum()))
    assert 0.10 <= share <= 0.90, (name, n_rays, out)
    assert out["fully_occluded"] >= 1 and out["fully_clear"] >= 1 and out["bent_off_normal"] >= 1 and out["invalid"] >= 3, (name, n_rays, out)
    return out


# ---- CPU tier ------------------------------------------------------------------------------------------------------------------------
def test_abi_surface(halart):
    """the header, the export list, the Python declarations and the library name the functions, the two records and the limit"""
    header = open(os.path.join(ROOT, "include", "halart.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    rust = open(os.path.join(ROOT, "rust", "hala-renderer-halart", "src", "lib.rs")).read()
    lib = C.CDLL(halart.LIB_PATH)
    for fn in FUNCTIONS:
        assert re.search(rf"\bint {fn}\s*\(", code), fn
        assert fn in A.EXPORTS and fn in A.PROTOTYPES, fn
        assert f"fn {fn}(" in rust, fn
        assert hasattr(lib, fn), fn
    assert "pub struct hala_occlusion_sample" in rust and "pub struct hala_occlusion " in rust and "pub const HALA_MAX_OCCLUSION_RAYS: u32 = 256;" in rust
    assert re.search(r"typedef struct hala_occlusion_sample \{\s*float point\[3\];\s*float bias;\s*float normal\[3\];\s*float reach;\s*\} hala_occlusion_sample;", code)
    assert re.search(r"typedef struct hala_occlusion \{\s*float visibility;\s*float bent\[3\];\s*\} hala_occlusion;", code)
    assert re.search(r"#define HALA_MAX_OCCLUSION_RAYS 256\b", code) and A.MAX_OCCLUSION_RAYS == 256
    assert C.sizeof(A.OcclusionSample) == 32 and A.OCCLUSION_SAMPLE_DTYPE.itemsize == 32
    assert C.sizeof(A.Occlusion) == 16 and A.OCCLUSION_DTYPE.itemsize == 16
    assert [f[0] for f in A.OcclusionSample._fields_] == list(A.OCCLUSION_SAMPLE_DTYPE.names)
    assert [f[0] for f in A.Occlusion._fields_] == list(A.OCCLUSION_DTYPE.names)
    assert [A.OCCLUSION_SAMPLE_DTYPE.fields[n][1] for n in ("point", "bias", "normal", "reach")] == [0, 12, 16, 28]
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*#define HALA_MAX_OCCLUSION_RAYS", header, flags=re.S)
    assert m and "RENDER_SPEC 4.10" in m.group(1) and "Not built" in m.group(1), "cites its section of the spec and names what is not built"
    assert callable(halart.HalaRenderer.occlusion)
    spec = open(os.path.join(ROOT, "docs", "RENDER_SPEC.md")).read()
    assert "### 4.10 Occlusion batches (no reference equivalent)" in spec


def test_pcg_inverse_and_equivalent_seed():
    for x in (0, 1, 0x12345678, 0xFFFFFFFF, 0x80000000, 747796405):
        assert int(pcg(np.uint64(OR.pcg_inverse(x)))) == x
    for seed, offset in ((0, 1), (7, 64), (0xDEADBEEF, 1000)):
        other = OR.equivalent_seed(seed, offset)
        assert np.array_equal(OR.streams(0, 16, other), OR.streams(offset, 16, seed))


@pytest.mark.parametrize("name,n_rays", CONDITION_SETS)
def test_the_inputs_are_telling(oracle, name, n_rays):
    print(name, n_rays, check_conditions(oracle, name, n_rays))


def test_translucent_triangles_matter(oracle):
    """in the translucent scene at least 32 rays change their outcome when the translucent triangles become opaque, and as many when they
    are removed (opacity 0: invisible to any-hit rays)"""
    for n_rays in (64, 256):
        ref = reference(oracle, "cornell_alpha", n_rays)
        rays, _ = OR.expand(ref.samples, n_rays, SEED)
        for opacity, what in ((1.0, "opaque"), (0.0, "removed")):
            other = oracle.OracleScene(translucent_cornell(opacity))
            changed = int(((other.trace(rays, 1, brute=True)["t"] > 0).reshape(ref.occluded.shape) != ref.occluded).sum())
            print(f"cornell_alpha N = {n_rays}: {changed} rays change when the translucent triangles are {what}")
            assert changed >= 32, (n_rays, what, changed)


def triangle_opacity(scene):
    """opacity of every triangle's material, global-id order (RENDER_SPEC 3: nodes in order, primitives in order)"""
    out = []
    for nd in scene.nodes:
        if nd.mesh_index != A.INVALID_INDEX:
            for pr in scene.meshes[nd.mesh_index].primitives:
                out.append(np.full(len(pr.indices) // 3, scene.materials[pr.material_index].opacity, dtype=f32))
    return np.concatenate(out)


def occluded64(scene, osc, samples, n_rays, seed):
    """float64 directions, a float64 Moeller-Trumbore over all triangles (the float32 records of the flattened scene) and the any-hit rule
    of RENDER_SPEC 7.1d for untextured materials: [count, N] bool"""
    o, d, ok = OR.expand64(samples, n_rays, seed)
    v0, e1, e2 = (x.astype(f64) for x in CR.scene_triangles(scene, osc))
    opacity = triangle_opacity(scene)
    assert len(opacity) == len(v0)
    reach = samples["reach"].astype(f64)
    reach = np.where(np.isnan(reach), -1.0, reach)
    key = pcg((np.arange(len(samples) * n_rays, dtype=np.uint64) ^ np.uint64(0x5BD1E995)) & M32).reshape(len(samples), n_rays)
    ids = np.arange(len(v0), dtype=np.uint64)
    translucent = (opacity > 0) & (opacity < 1)
    out = np.zeros((len(samples), n_rays), dtype=bool)
    step = max(1, 400000 // max(len(v0) * n_rays, 1))
    with np.errstate(all="ignore"):
        for lo in range(0, len(samples), step):
            sl = slice(lo, lo + step)
            dd = d[sl, :, None, :]                              # [s, N, 1, 3]
            p = np.cross(dd, e2[None, None])                     # [s, N, T, 3]
            det = (e1[None, None] * p).sum(-1)
            inv = 1.0 / det
            tv = (o[sl, None, None, :] - v0[None, None])          # [s, 1, T, 3]
            u = (tv * p).sum(-1) * inv
            q = np.cross(tv, e1[None, None])                     # [s, 1, T, 3]
            v = (dd * q).sum(-1) * inv
            t = np.broadcast_to((e2[None, None] * q).sum(-1), det.shape) * inv
            hit = (det != 0) & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (t > 0) & (t < reach[sl, None, None])
            blocks = np.broadcast_to((opacity > 0)[None, None, :], hit.shape)
            if translucent.any():
                draw = pcg((key[sl, :, None] + ids[None, None, :] * np.uint64(0x9E3779B1)) & M32)
                passes = ((draw >> np.uint64(8)).astype(f64) * 2.0 ** -24).astype(f32) >= opacity[None, None, :]
                blocks = blocks & ~(translucent[None, None, :] & passes)
            out[sl] = (hit & blocks).any(axis=-1)
    return out & ok[:, None]


@pytest.mark.parametrize("name,n_rays", CONDITION_SETS)
def test_twin_against_float64(oracle, name, n_rays):
    """the rays whose float64 outcome differs from the twin's are the grazing ones: their share per set, at most twice what was measured;
    a sample's visibility differs from its float64 value by no more than its own count of such rays over N"""
    ref = reference(oracle, name, n_rays)
    want = occluded64(ref.scene, ref.osc, ref.samples, n_rays, SEED)
    differ = want != ref.occluded
    share = float(differ.mean())
    by_kind = {KINDS[k]: int(differ[ref.kinds == k].sum()) for k in range(len(KINDS)) if differ[ref.kinds == k].any()}
    print(f"{name} N = {n_rays}: {int(differ.sum())} of {differ.size} rays differ from float64 ({share:.2e}) {by_kind}")
    assert share <= 2.0 * GRAZING_SHARE[(name, n_rays)], (name, n_rays, share)
    ok = ref.rec["visibility"] >= 0
    vis64 = (~want).sum(axis=1) / float(n_rays)
    assert (np.abs(ref.rec["visibility"].astype(f64) - vis64)[ok] <= differ.sum(axis=1)[ok] / float(n_rays) + 2.0 ** -24).all()


def _quad_prim(p0, p1, p2, p3):
    p = scenes._merge_quads([(p0, p1, p2, p3)])
    p.material_index = 0
    return p


def test_analytic_floor_under_a_wall(oracle):
    """256 samples on a floor, 0.01 from a wall of half-width and height 100 at a right angle, normal up, N = 256: the wall hides the
    half of the hemisphere behind it, so the mean visibility is 0.5 +- 0.011 (5 sigma of 65 536 Bernoulli draws is 0.0098; what escapes over
    or around the finite wall is below 0.001)"""
    s = H.HalaScene()
    s.materials = [H.HalaMaterial(type=0, base_color=(0.7, 0.7, 0.7))]
    floor = _quad_prim((0, 0, 100), (100, 0, 100), (100, 0, -100), (0, 0, -100))
    wall = _quad_prim((0, 0, -100), (0, 100, -100), (0, 100, 100), (0, 0, 100))
    s.meshes = [H.HalaMesh([floor]), H.HalaMesh([wall])]
    s.nodes = [H.HalaNode(name="floor", mesh_index=0), H.HalaNode(name="wall", mesh_index=1)]
    osc = oracle.OracleScene(s)
    samples = np.zeros(256, dtype=A.OCCLUSION_SAMPLE_DTYPE)
    samples["point"] = np.stack([np.full(256, 0.01), np.zeros(256), np.linspace(-1.0, 1.0, 256)], axis=1).astype(f32)
    samples["normal"], samples["bias"], samples["reach"] = (0.0, 1.0, 0.0), ray_eps(osc), np.inf
    rec, masks, occluded = twin_answer(osc, samples, 256, 3)
    mean = float(rec["visibility"].astype(f64).mean())
    print(f"mean visibility {mean:.5f}")
    assert abs(mean - 0.5) <= 0.011
    # the bent normal leans away from the wall
    assert (rec["bent"][:, 0] > 0.2).all() and (rec["bent"][:, 1] > 0.5).all()
    assert np.array_equal(OR.bits_of(masks, 256), occluded)


def test_degenerate_samples_answer_the_invalid_record(oracle):
    ref = scene_ref(oracle, "cornell")
    good = ref.samples[ref.samples["reach"] == np.inf][:21]
    good = good[OR.valid_flags(good)[0]]
    good = np.concatenate([good] * 21)[:21]
    bad = degenerate_samples(good)
    mixed = np.empty(42, dtype=A.OCCLUSION_SAMPLE_DTYPE)
    mixed[0::2], mixed[1::2] = bad, good
    for n_rays in (1, 33, 64):
        rec, masks, _ = twin_answer(ref.osc, mixed, n_rays, SEED)
        rays, ok = OR.expand(mixed, n_rays, SEED)
        assert not ok[0::2].any() and ok[1::2].all()
        assert rec[0::2].tobytes() == np.array([OR.INVALID] * 21, dtype=A.OCCLUSION_DTYPE).tobytes()
        assert not masks[0::2].any()
        assert (rec["visibility"][1::2] >= 0).all()
        assert np.isfinite(rays["origin"]).all() and np.isfinite(rays["direction"]).all()


def test_normals_at_the_singular_end_of_the_basis():
    """(0, 0, +-1) and (0, 0, -1 + 2^-24): the branchless basis divides by sign + n.z, which stays away from 0"""
    s = np.zeros(4, dtype=A.OCCLUSION_SAMPLE_DTYPE)
    s["normal"] = [(0, 0, 1), (0, 0, -1), (0, 0, -1 + 2.0 ** -24), (-0.0, 0.0, -1)]
    s["bias"], s["reach"] = 0.25, np.inf
    rays, ok = OR.expand(s, 256, SEED)
    assert ok.all() and np.isfinite(rays["direction"]).all() and np.isfinite(rays["origin"]).all()
    d = rays["direction"].reshape(4, 256, 3).astype(f64)
    assert (np.abs(np.linalg.norm(d, axis=2) - 1.0) < 1e-6).all()
    assert ((d * unit_normals(s)[:, None, :]).sum(axis=2) >= 0).all(), "every direction lies in the normal's hemisphere"
    o64, d64, _ = OR.expand64(s, 256, SEED)
    assert np.abs(d - d64).max() < 1e-6


# ---- GPU tier ------------------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def renderers(halart, oracle):
    """one committed renderer per (scene, builder), closed when the module is done"""
    from test_gpu_parity import make_renderer
    made = {}

    def get(name, builder=None):
        if (name, builder) not in made:
            build = dict(builder=builder, instancing=True) if SCENES[name][1] == "two_level" else dict(builder=builder)
            made[(name, builder)] = make_renderer(halart, scene_ref(oracle, name).scene, 16, 16, build=build)
            assert_form(made[(name, builder)], SCENES[name][1])
        return made[(name, builder)]
    yield get
    for r in made.values():
        r.close()


def assert_form(r, form):
    i = r.bvh_info()
    assert (i.instance_ref_count > 0) == (form == "two_level"), form
    assert (i.lds_node_count > 0) == (form == "staged"), form


def assert_equals_twin(got, ref_rec, ref_masks, samples, what):
    rec, masks = got
    if rec.tobytes() != ref_rec.tobytes() or masks.tobytes() != ref_masks.tobytes():
        bad = np.nonzero((rec.view(np.uint32).reshape(len(rec), 4) != ref_rec.view(np.uint32).reshape(len(rec), 4)).any(axis=1) |
                         (masks != ref_masks).any(axis=1))[0]
        i = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {len(rec)} samples differ; first sample {i} {samples[i]}: got {rec[i]} {masks[i]} "
                             f"want {ref_rec[i]} {ref_masks[i]}")


@gpu
@pytest.mark.parametrize("n_rays", RAY_COUNTS)
@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("name", list(SCENES))
def test_records_and_masks_equal_the_twin(halart, oracle, renderers, name, builder, n_rays):
    if n_rays in (64, 256):
        check_conditions(oracle, name, n_rays)
    ref = reference(oracle, name, n_rays)
    r = renderers(name, builder)
    got = r.occlusion(ref.samples, rays=n_rays, seed=SEED, want_masks=True)
    assert got[1].shape == (count_for(n_rays), (n_rays + 31) // 32)
    assert_equals_twin(got, ref.rec, ref.masks, ref.samples, f"{name} {builder} N = {n_rays}")


@gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_masks_equal_the_renderers_own_any_hit_batch(halart, oracle, renderers, name):
    """ray (i, j) is entry i * N + j of the expanded batch in mode 1 of hala_rt_trace_rays, on the same renderer"""
    for n_rays in (33, 64):
        ref = reference(oracle, name, n_rays)
        r = renderers(name)
        rays, ok = OR.expand(ref.samples, n_rays, SEED)
        own = (r.trace_rays_host(rays, 1)["t"] > 0).reshape(len(ref.samples), n_rays)
        _, masks = r.occlusion(ref.samples, rays=n_rays, seed=SEED, want_masks=True)
        assert np.array_equal(OR.bits_of(masks, n_rays), own), (name, n_rays)
        if n_rays & 31:
            assert not (masks[:, -1] >> np.uint32(n_rays & 31)).any(), "bits >= N are 0"


@gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_far_samples(halart, oracle, renderers, name):
    """64 points at 10^2 and 64 at 10^4 scene diagonals, normals aimed at the scene, reach +inf: the far-origin rule of RENDER_SPEC 4.2
    runs in the lanes; records and masks equal the twin, whose bits come from the oracle's own re-basing"""
    base = scene_ref(oracle, name)
    rs = np.random.RandomState(77)
    samples = np.concatenate([far_samples(base.osc, 64, 2, rs), far_samples(base.osc, 64, 4, rs)])
    rec, masks, _ = twin_answer(base.osc, samples, 64, SEED)
    got = renderers(name).occlusion(samples, rays=64, seed=SEED, want_masks=True)
    assert_equals_twin(got, rec, masks, samples, f"far samples, {name}")


@gpu
@pytest.mark.parametrize("name", ["cornell", "blob"])
def test_forms_determinism_and_the_global_sample_index(halart, oracle, renderers, name):
    import torch
    n_rays = 33
    ref = reference(oracle, name, n_rays)
    r = renderers(name)
    n, w = len(ref.samples), 2
    first = r.occlusion(ref.samples, rays=n_rays, seed=SEED, want_masks=True)
    second = r.occlusion(ref.samples, rays=n_rays, seed=SEED, want_masks=True)
    assert first[0].tobytes() == second[0].tobytes() == ref.rec.tobytes() and first[1].tobytes() == second[1].tobytes() == ref.masks.tobytes()
    # points + normals with one bias and per-sample reach: the same samples
    plain = r.occlusion(ref.samples["point"], ref.samples["normal"], rays=n_rays, reach=ref.samples["reach"], bias=ref.samples["bias"], seed=SEED)
    assert plain.tobytes() == ref.rec.tobytes()
    # the device form on a second stream, with the caller's masks and with the renderer's own
    d_s = torch.from_numpy(ref.samples.view(np.uint8).copy()).cuda()
    d_out = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    d_masks = torch.full((n * w,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    r.occlusion(d_s, rays=n_rays, seed=SEED, out=d_out, out_masks=d_masks, stream=side.cuda_stream)
    side.synchronize()
    assert d_out.cpu().numpy().tobytes() == ref.rec.tobytes() and d_masks.cpu().numpy().tobytes() == ref.masks.tobytes()
    d_out.zero_()
    torch.cuda.synchronize()
    r.occlusion(d_s.data_ptr(), rays=n_rays, seed=SEED, out=d_out.data_ptr(), count=n)  # raw pointers, no masks, the renderer's stream
    r.wait_idle()
    assert d_out.cpu().numpy().tobytes() == ref.rec.tobytes()
    # another seed, another answer; the equivalent seed and a sample offset, the same one: i is the global sample index
    other = r.occlusion(ref.samples, rays=n_rays, seed=SEED + 1)
    assert other.tobytes() != ref.rec.tobytes()
    offset = 40
    tail = r.occlusion(ref.samples[offset:], rays=n_rays, seed=OR.equivalent_seed(SEED, offset))
    assert tail.tobytes() == ref.rec[offset:].tobytes()


@gpu
def test_count_zero_and_refusals(halart, oracle, renderers):
    """count == 0 is a no-op; rays outside 1..256, a null sample or output pointer, an uncommitted renderer and count * rays >= 2^32 raise
    with their message and leave prefilled buffers as they were and the renderer usable"""
    import torch
    ref = reference(oracle, "cornell", 32)
    r = renderers("cornell")
    n = 64
    d_s = torch.from_numpy(ref.samples[:n].view(np.uint8).copy()).cuda()
    d_out = torch.full((n * 16,), 0xAB, dtype=torch.uint8, device="cuda")
    d_masks = torch.full((n * 8 * 4,), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    fresh = halart.HalaRenderer("uncommitted", 16, 16, 5, 3, False, False, False, 0)
    s_, o_, m_ = d_s.data_ptr(), d_out.data_ptr(), d_masks.data_ptr()
    for who, args, match in ((r, (s_, o_, m_, n, 0), "1..256"), (r, (s_, o_, m_, n, 257), "1..256"), (r, (0, o_, m_, n, 32), "null"),
                             (r, (s_, 0, m_, n, 32), "null"), (fresh, (s_, o_, m_, n, 32), "acceleration structure"),
                             (r, (s_, o_, m_, 1 << 24, 256), "too large"), (r, (s_, o_, 0, 0xFFFFFFFF, 2), "too large")):
        with pytest.raises(halart.HalaRendererError, match=match):
            who._check(who._lib.hala_rt_occlusion(who._h, C.c_void_p(args[0]), C.c_void_p(args[1]), C.c_void_p(args[2]), C.c_uint32(args[3]),
                                                  C.c_uint32(args[4]), C.c_uint32(SEED), None))
    with pytest.raises(halart.HalaRendererError, match="1..256"):
        r.occlusion(ref.samples[:n], rays=300)
    with pytest.raises(halart.HalaRendererError, match="acceleration structure"):
        fresh.occlusion(ref.samples[:n], rays=32)
    r.occlusion(d_s, rays=32, out=d_out, out_masks=d_masks, count=0)
    empty = r.occlusion(np.zeros((0, 3), f32), np.zeros((0, 3), f32), rays=32, want_masks=True)
    assert len(empty[0]) == 0 and empty[1].shape == (0, 1)
    r.wait_idle()
    torch.cuda.synchronize()
    assert bool((d_out == 0xAB).all()) and bool((d_masks == 0xCD).all())
    fresh.close()
    got = r.occlusion(ref.samples, rays=32, seed=SEED, want_masks=True)  # still usable
    assert_equals_twin(got, ref.rec, ref.masks, ref.samples, "after the refusals")


@gpu
@pytest.mark.parametrize("name", ["cornell", "blob"])
def test_frames_around_a_batch_are_unchanged(halart, oracle, name):
    """update, batch, update: the batch shares the renderer's scratch; images 0-3 are those of a run without the batch, bit for bit"""
    from test_gpu_parity import make_renderer
    ref = reference(oracle, name, 64)
    images = []
    for with_batch in (False, True):
        r = make_renderer(halart, ref.scene, 32, 32)
        r.update(); r.render()
        if with_batch:
            assert_equals_twin(r.occlusion(ref.samples, rays=64, seed=SEED, want_masks=True), ref.rec, ref.masks, ref.samples, f"between frames, {name}")
        r.update(); r.render()
        images.append([r.read_image(which).tobytes() for which in range(4)])
        r.close()
    assert images[0] == images[1]


def edited_answer(oracle, scene, seed, n_rays=64):
    osc = oracle.OracleScene(scene)
    samples, _ = surface_samples(scene, osc, seed)
    rec, masks, occluded = twin_answer(osc, samples, n_rays, SEED)
    share = occluded[rec["visibility"] >= 0].mean()
    assert 0.10 <= share <= 0.90, share
    return samples, rec, masks


@gpu
def test_after_a_node_refit(halart, oracle):
    """update_node_transform + refit on two flattened blobs: the answers are the twin's on the edited scene"""
    from test_closest_points import two_blobs
    from test_gpu_parity import make_renderer
    s = two_blobs()
    r = make_renderer(halart, s, 16, 16, build=dict(instancing=False))
    assert r.bvh_info().instance_ref_count == 0
    m = np.eye(4, dtype=f32); m[:3, :3] *= f32(0.75); m[:3, 3] = (1.5, 0.25, -0.5)  # into the other blob
    ops = [("node", 0, m)]
    before = r.occlusion(surface_samples(s, oracle.OracleScene(s), 61)[0], rays=64, seed=SEED)
    SE.apply_to_renderer(r, ops)
    r.refit()
    samples, rec, masks = edited_answer(oracle, SE.apply_to_scene(s, ops), 61)
    assert before.tobytes() != rec.tobytes()
    assert_equals_twin(r.occlusion(samples, rays=64, seed=SEED, want_masks=True), rec, masks, samples, "node refit")
    r.close()


@gpu
def test_after_a_deformer_refit(halart, oracle):
    """a posed morph target + refit on the blob: the answers are the twin's on the posed vertices (deform_ref's)"""
    from test_gpu_parity import make_renderer
    s = RC.blob_scene(3)
    r = make_renderer(halart, s, 16, 16)
    rest = s.meshes[0].primitives[0].vertices
    pos = np.asarray(rest["position"], dtype=f32)
    delta = (pos * (0.3 * np.sin(5.0 * pos[:, 1:2]))).astype(f32)
    r.set_deformer(0, 0, targets=delta[None])
    r.update_deformer(0, 0, morph_weights=[0.7])
    r.refit()
    posed = DR.deform(rest, targets=delta[None], morph_weights=[0.7])
    assert r.read_vertices(0, 0)["position"].tobytes() == posed["position"].tobytes()
    samples, rec, masks = edited_answer(oracle, SE.apply_to_scene(s, [("vertices", 0, 0, posed)]), 71)
    assert_equals_twin(r.occlusion(samples, rays=64, seed=SEED, want_masks=True), rec, masks, samples, "deformer refit")
    r.close()
