"""Transfer bakes (docs/RENDER_SPEC.md 4.13): hala_rt_bake_transfer against the numpy twin of tests/bake_transfer_ref.py, every byte of
every record and texel record.

The scene is test_bake_atlas.carpets(): the Cornell box (instances 0-5) with the bumpy 8 x 8 carpet (instance 6, y ~ 2) as receiver and
the mirrored 4 x 4 carpet (instance 7, y = 60) above it.  SETS are (receiver flags, front, back, targets):
  A  the cage 200 above the carpet, 50 below, every other instance: the mirrored carpet, the blocks and the box are hit
  B  a cage 30 above it that never ends, the box and the blocks only: the mirrored carpet sits in between and is not seen
  C  the blocks alone: most texels miss
  D  the floor alone with tmax = 201, which cuts through the carpet's bumps: hits and misses side by side, at t close to tmax
  E  the flipped normal from 5 below the carpet: the floor first, where the unfiltered ray would meet the carpet itself
  F  four targets that are no neighbours in instance order: four id ranges, the table in memory and its bisection
  G  the cage 100 000 above: every origin is far (RENDER_SPEC 4.2), t comes back as t' + ts
The carpet fills its whole map, so ownerless texels and the dilation are tested on `gutter`, the same scene with the carpet's chart shrunk
to the middle half of the map.  The maps are test_bake's: one texel, one block, full blocks, partial blocks, a map one block high.

CPU tier: the ABI surface; the sets are telling; twin consistency (default targets, permutations, height); the twin against float64.
GPU tier: every set on every map with margin 0 and 3; the gutter map with margins 0, 3, 16; staged and large trees by every builder; the
composition bake_samples -> rays -> trace_rays_multi(k = 16) -> host filter; target lists; translucent materials; determinism, frames
around a transfer, a refit of the target; the refusals; the Python forms and the stream order."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bake_ref as BR
import bake_transfer_ref as TR
import hala_renderer_amd as H
from hala_renderer_amd import scenes
import scene_edits as SE
import test_bake as TB
import test_bake_atlas as TA
from test_bake import MISS, same_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = H._abi
f32, f64 = np.float32, np.float64
FUNCTIONS = ("hala_rt_bake_transfer", "hala_rt_bake_transfer_host")
INF = float("inf")
SETS = {"A": (1, 200.0, 50.0, None), "B": (1, 30.0, INF, (0, 1, 2, 3, 4, 5)), "C": (1, 200.0, INF, (4, 5)), "D": (1, 200.0, 1.0, (0,)), "E": (3, 5.0, INF, None),
        "F": (1, 200.0, 50.0, (7, 2, 4, 0)), "G": (1, 1.0e5, INF, None)}
MAPS = TB.MAPS
NAME, RECEIVER = TA.NAME, 6
BLOB = (1, 0.5, 0.5, None)  # under the blob: half a unit above the chart to half a unit below it
# measured here (test_the_twin_against_float64 prints them): per set, over the 64 x 64 and 67 x 33 maps, the texels whose triangle differs
# from the float64 answer and the largest |t32 - t64| in ulp32 of front + back where that is finite, else of the scene's diagonal
FLOAT64 = {"A": (0, 12.887), "B": (0, 3.865), "C": (0, 7.485), "D": (0, 2.985), "E": (0, 0.101), "F": (0, 3.066), "G": (0, 3.595)}


def gutter_carpets():
    return TB.in_cornell(TB.chart(8, TB.gutter_uv), extra=TB.chart(4))


def blob():
    return TB.in_blob(TB.chart(16))


def one_instance():
    """the Cornell box's camera and light around its short block alone"""
    s = scenes.cornell_box()
    s.meshes = [H.HalaMesh([s.meshes[1].primitives[0]])]
    s.nodes = [H.HalaNode(name="only", mesh_index=0)] + [nd for nd in s.nodes if nd.mesh_index == A.INVALID_INDEX]
    return s


SCENES = {NAME: TA.carpets, "transfer_gutter": gutter_carpets, "blob": blob}
_TWIN, _CASE = {}, {}


def twin_of(oracle, name):
    if name not in _TWIN:
        base = TB.scene_ref(oracle, name, SCENES[name])
        _TWIN[name] = TR.Twin(base.twin, base.osc)
    return _TWIN[name]


class Case:
    pass


def case_ref(oracle, name, receiver, w, h, params):
    """samples, texel records, rays, hits and undilated records of one call: computed once, shared and left unchanged"""
    key = (name, receiver, w, h, params)
    if key not in _CASE:
        flags, front, back, targets = params
        twin = twin_of(oracle, name)
        c = Case()
        c.twin, c.receiver, c.w, c.h, c.params = twin, receiver, w, h, params
        c.samples, c.texels = twin.base.samples(receiver, w, h, flags=flags)
        c.rays, c.valid = twin.rays(c.samples, front, back)
        c.mask = twin.target_mask(receiver, targets)
        c.hits = twin.first(c.rays, c.valid, c.mask)
        c.rec = twin.records(c.hits, front)
        c.owned = c.texels["prim"] != MISS
        _CASE[key] = c
    return _CASE[key]


def instance_of(twin, prim):
    return np.searchsorted(twin.base.first, prim, side="right") - 1


def hits_by_instance(c):
    return np.bincount(instance_of(c.twin, c.hits.prim[c.hits.found]), minlength=c.twin.instances)


# ---- CPU tier ------------------------------------------------------------------------------------------------------------------------
def test_abi_surface(halart):
    """the header, the export list, the Python declarations, the Rust binding and the built library name the two functions and the two
    records; the spec, the design notes and the integration guide have their sections"""
    header = open(os.path.join(ROOT, "include", "halart.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    rust = open(os.path.join(ROOT, "rust", "hala-renderer-halart", "src", "lib.rs")).read()
    lib = C.CDLL(halart.LIB_PATH)
    for fn in FUNCTIONS:
        assert re.search(rf"\bint {fn}\s*\(", code), fn
        assert fn in A.EXPORTS and fn in A.PROTOTYPES, fn
        assert f"fn {fn}(" in rust, fn
        assert hasattr(lib, fn), fn
    assert "pub struct hala_bake_transfer_desc" in rust and "pub struct hala_bake_transfer_hit" in rust and "pub fn bake_transfer(" in rust
    assert re.search(r"typedef struct hala_bake_transfer_desc \{\s*float front, back;\s*uint32_t flags;\s*uint32_t target_count;\s*\} hala_bake_transfer_desc;", code)
    assert re.search(r"typedef struct hala_bake_transfer_hit \{\s*float t, u, v;\s*uint32_t prim;\s*float normal\[3\];\s*float height;\s*\} hala_bake_transfer_hit;", code)
    assert C.sizeof(A.BakeTransferDesc) == 16 and C.sizeof(A.BakeTransferHit) == 32 and A.BAKE_TRANSFER_HIT_DTYPE.itemsize == 32
    assert [(f[0], getattr(A.BakeTransferDesc, f[0]).offset) for f in A.BakeTransferDesc._fields_] == [("front", 0), ("back", 4), ("flags", 8), ("target_count", 12)]
    names = ["t", "u", "v", "prim", "normal", "height"]
    assert [f[0] for f in A.BakeTransferHit._fields_] == names == list(A.BAKE_TRANSFER_HIT_DTYPE.names)
    assert [A.BAKE_TRANSFER_HIT_DTYPE.fields[n][1] for n in names] == [getattr(A.BakeTransferHit, n).offset for n in names] == [0, 4, 8, 12, 16, 28]
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*typedef struct hala_bake_transfer_desc", header, flags=re.S)
    assert m and "RENDER_SPEC 4.13" in m.group(1) and "Not built" in m.group(1), "cites its section of the spec and names what is not built"
    for word in ("tangent-space", "atlas form", "instance masks", "supersampling", "two-level"):
        assert word in m.group(1), word
    assert callable(halart.HalaRenderer.bake_transfer)
    spec = open(os.path.join(ROOT, "docs", "RENDER_SPEC.md")).read()
    assert "### 4.13 Transfer bakes (no reference equivalent)" in spec
    assert re.search(r"^## 33\.", open(os.path.join(ROOT, "DESIGN.md")).read(), flags=re.M)
    assert re.search(r"^## 6r\.", open(os.path.join(ROOT, "INTEGRATION.md")).read(), flags=re.M)
    assert "bake_transfer_timing.py" in open(os.path.join(ROOT, "README.md")).read()


def test_dilate_copies_rows_of_any_record(oracle):
    """bake_ref.dilate is written for the 16-B occlusion records: it copies whole rows of the 32-B records too"""
    c = case_ref(oracle, "transfer_gutter", RECEIVER, 67, 33, SETS["A"])
    assert 0.1 < c.owned.mean() < 0.5
    rec, texels = BR.dilate(c.rec, c.texels, 67, 33, 3)
    filled = (texels["source"] != MISS) & ~c.owned
    assert filled.sum() > 100 and rec[filled].tobytes() == c.rec[texels["source"][filled]].tobytes()
    assert (rec["t"][filled] > 0).sum() > 100 and (texels["prim"][filled] == MISS).all() and not texels["u"][filled].any()
    same_bytes(rec[~filled], c.rec[~filled], "the others are as they were")


@pytest.mark.parametrize("size", [(64, 64), (67, 33)])
def test_the_sets_are_telling(oracle, size):
    w, h = size
    case = {k: case_ref(oracle, NAME, RECEIVER, w, h, SETS[k]) for k in SETS}
    every = np.ones(case["A"].twin.instances, bool)
    changed = {k: int((c.twin.first(c.rays, c.valid, every).prim != c.hits.prim).sum()) for k, c in case.items() if k in "BE"}
    for c in case.values():
        assert c.owned.all() and c.valid.all(), "the carpet fills its map"
    a = hits_by_instance(case["A"])
    assert (a >= 10).sum() >= 3 and case["A"].hits.found.all(), a
    assert (~case["B"].hits.found).sum() >= 1 and changed["B"] >= 1000
    cc = case["C"].hits.found
    assert (~cc).sum() > cc.sum() >= 1
    assert 0.1 < case["D"].hits.found.mean() < 0.9
    e = hits_by_instance(case["E"])
    assert (e > 0).sum() >= 2 and changed["E"] >= 100, e
    assert (hits_by_instance(case["F"])[[0, 2, 4, 7]] > 0).sum() >= 3 and case["F"].mask.nonzero()[0].tolist() == [0, 2, 4, 7], "four id ranges"
    g = case["G"].hits
    assert g.far.all() and g.found.all() and (g.ts > 9.0e4).all(), "every origin of G is far and re-based"


@pytest.mark.parametrize("size", [(8, 8), (128, 3)])
def test_the_small_maps_are_telling(oracle, size):
    """C hits at least once from 8 x 8 up (and still misses more often than it hits), D stays between 10 % and 90 %"""
    c = case_ref(oracle, NAME, RECEIVER, size[0], size[1], SETS["C"]).hits.found
    d = case_ref(oracle, NAME, RECEIVER, size[0], size[1], SETS["D"]).hits.found
    assert (~c).sum() > c.sum() >= 1
    assert 0.1 < d.mean() < 0.9


def test_the_blob_set_hits_and_misses(oracle):
    for w, h in ((16, 16), (67, 33)):
        base = TB.scene_ref(oracle, "blob", blob)
        c = case_ref(oracle, "blob", base.instance, w, h, BLOB)
        assert c.valid.all() and 0.1 < c.hits.found.mean() < 0.9


def test_twin_consistency(oracle):
    """default targets = the explicit list of all others; a permuted list gives the same bytes; height == front - t bit for bit; the
    normal is a unit vector and is not turned to the ray"""
    w, h = 67, 33
    twin = twin_of(oracle, NAME)
    for k in ("A", "E"):
        c = case_ref(oracle, NAME, RECEIVER, w, h, SETS[k])
        flags, front, back, _ = SETS[k]
        explicit = twin.transfer(RECEIVER, w, h, flags, front, back, (0, 1, 2, 3, 4, 5, 7))
        same_bytes(explicit[0], c.rec, f"{k}: explicit list")
        same_bytes(twin.transfer(RECEIVER, w, h, flags, front, back, (7, 3, 0, 5, 1, 4, 2))[0], c.rec, f"{k}: permuted list")
    for k, params in SETS.items():
        c = case_ref(oracle, NAME, RECEIVER, w, h, params)
        hit = c.hits.found
        assert (c.rec["height"][hit].view(np.uint32) == (f32(params[1]) - c.rec["t"][hit]).astype(f32).view(np.uint32)).all()
        assert np.allclose(np.linalg.norm(c.rec["normal"][hit].astype(f64), axis=1), 1.0, atol=1e-6)
        assert not c.rec[~hit]["normal"].any() and (c.rec["t"][~hit] == -1).all() and (c.rec["prim"][~hit] == MISS).all() and not c.rec["height"][~hit].any()
    along = {}
    for k in ("A", "E"):  # from above onto surfaces that face up; from below onto the floor, which faces up too
        c = case_ref(oracle, NAME, RECEIVER, w, h, SETS[k])
        along[k] = (c.rec["normal"].astype(f64) * c.rays["direction"].astype(f64)).sum(axis=1)[c.hits.found]
    assert (along["A"] < -0.5).sum() > 100 and (along["E"] > 0.5).sum() > 100, "normals against and with the ray: they are the target's own"


@pytest.mark.parametrize("name", list(SETS))
def test_the_twin_against_float64(oracle, name):
    """the same rays and the same filtered minimum in float64 on the float32 records; the bounds are twice what was measured"""
    flags, front, back, targets = SETS[name]
    diff = 0
    worst = 0.0
    for w, h in ((64, 64), (67, 33)):
        c = case_ref(oracle, NAME, RECEIVER, w, h, SETS[name])
        t64, p64 = TR.first64(c.twin, c.rays, c.valid, c.mask)
        diff += int((p64 != c.hits.prim).sum())
        both = c.hits.found & (p64 == c.hits.prim)
        scale = f32(front) + f32(back) if np.isfinite(back) else c.twin.diag
        worst = max(worst, float(np.abs(c.hits.t[both].astype(f64) - t64[both]).max() / np.spacing(f32(scale))))
    print(f"set {name}: {diff} texels differ in prim, |t32 - t64| <= {worst:.3f} ulp32")
    assert diff <= 2 * FLOAT64[name][0] and worst <= 2.0 * FLOAT64[name][1]


# ---- GPU tier ------------------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def renderers(halart, oracle):
    """one committed renderer per (scene, builder), closed when the module is done"""
    from test_gpu_parity import make_renderer
    made = {}

    def get(name, builder=None):
        if (name, builder) not in made:
            made[(name, builder)] = make_renderer(halart, TB.scene_ref(oracle, name, SCENES[name]).scene, 16, 16, build=dict(builder=builder))
            assert made[(name, builder)].bvh_info().instance_ref_count == 0
        return made[(name, builder)]
    yield get
    for r in made.values():
        r.close()


def call(r, c, margin=0, targets="set"):
    flags, front, back, tg = c.params
    return r.bake_transfer(c.receiver, c.w, c.h, front, back, tg if targets == "set" else targets, margin=margin, **TB.FLAG_KW[flags])


def check(r, c, margin=0, what="", targets="set"):
    """records and texel records of one call against the twin, byte for byte"""
    want_r, want_t = BR.dilate(c.rec, c.texels, c.w, c.h, margin) if margin else (c.rec, c.texels)
    got_r, got_t = call(r, c, margin, targets)
    assert got_r.shape == got_t.shape == (c.h, c.w)
    same_bytes(got_r, want_r, f"records {c.w} x {c.h} margin {margin} {what}")
    same_bytes(got_t, want_t, f"texels {c.w} x {c.h} margin {margin} {what}")


@gpu
@pytest.mark.parametrize("size", MAPS)
@pytest.mark.parametrize("name", list(SETS))
def test_records_equal_the_twin(halart, oracle, renderers, name, size):
    r = renderers(NAME)
    assert r.bvh_info().lds_node_count > 0, "a one-level tree staged in LDS"
    c = case_ref(oracle, NAME, RECEIVER, size[0], size[1], SETS[name])
    for margin in (0, 3):
        check(r, c, margin, f"set {name}")


@gpu
@pytest.mark.parametrize("size", [(8, 8), (64, 64), (67, 33), (128, 3)])
def test_ownerless_texels_and_the_dilation(halart, oracle, renderers, size):
    """the chart in the middle half of the map: ownerless texels take no ray and get the miss record; margins 0, 3 and 16"""
    r = renderers("transfer_gutter")
    for name in ("A", "D"):
        c = case_ref(oracle, "transfer_gutter", RECEIVER, size[0], size[1], SETS[name])
        assert 0.05 < c.owned.mean() < 0.6 and c.hits.found.any() and (c.valid == c.owned).all()
        for margin in (0, 3, 16):
            check(r, c, margin, f"gutter, set {name}")


@gpu
@pytest.mark.parametrize("builder", TB.BUILDERS)
def test_trees_and_builders(halart, oracle, renderers, builder):
    """the staged Cornell tree and the large one-level tree under the blob, by every builder: the same bytes"""
    r = renderers(NAME, builder)
    assert r.bvh_info().lds_node_count > 0
    for name in ("A", "F"):
        check(r, case_ref(oracle, NAME, RECEIVER, 67, 33, SETS[name]), 0, f"set {name} {builder}")
    r = renderers("blob", builder)
    assert r.bvh_info().lds_node_count == 0 and r.bvh_info().instance_ref_count == 0
    base = TB.scene_ref(oracle, "blob", blob)
    for w, h in ((16, 16), (67, 33)):
        check(r, case_ref(oracle, "blob", base.instance, w, h, BLOB), 1, f"blob {builder}")
        check(r, case_ref(oracle, "blob", base.instance, w, h, BLOB), 0, f"blob {builder}, explicit", targets=(0,))


@gpu
@pytest.mark.parametrize("name", ["A", "D"])
def test_the_composition_on_the_gpu(halart, oracle, renderers, name):
    """bake_samples, the rays of 4.13 on the host, trace_rays_multi(k = 16), the host's filter by instance: the transfer's (t, u, v, prim),
    wherever the list was not exhausted before a target (at most 5 % of the texels may be left out)"""
    r = renderers(NAME)
    w, h = 67, 33
    c = case_ref(oracle, NAME, RECEIVER, w, h, SETS[name])
    flags, front, back, _ = c.params
    samples, _ = r.bake_samples(RECEIVER, w, h, bias=0.0, **TB.FLAG_KW[flags])
    rays, valid = c.twin.rays(samples.reshape(-1), front, back)
    assert valid.all()
    lists, counts = r.trace_rays_multi_host(rays, 16)
    admitted = (lists["prim"] != MISS) & c.mask[instance_of(c.twin, np.where(lists["prim"] != MISS, lists["prim"], 0))]
    first = np.argmax(admitted, axis=1)
    found = admitted.any(axis=1)
    decided = found | (counts < 16)  # a list that is not full and names no target: a miss
    assert (~decided).mean() <= 0.05
    want = np.zeros(w * h, dtype=A.HIT_DTYPE)
    want["t"], want["prim"] = -1.0, MISS
    want[found] = lists[np.arange(w * h)[found], first[found]]
    got = call(r, c)[0].reshape(-1)
    head = np.zeros(w * h, dtype=A.HIT_DTYPE)
    for f in ("t", "u", "v", "prim"):
        head[f] = got[f]
    same_bytes(head[decided], want[decided], f"set {name}")
    assert found.sum() > 100


@gpu
def test_target_lists(halart, oracle, renderers):
    """target_count == 0 is the explicit list of all other instances; the order of a list does not show"""
    r = renderers(NAME)
    for name in ("A", "E"):
        c = case_ref(oracle, NAME, RECEIVER, 67, 33, SETS[name])
        check(r, c, 0, f"set {name}, explicit", targets=(0, 1, 2, 3, 4, 5, 7))
        check(r, c, 0, f"set {name}, permuted", targets=(7, 3, 0, 5, 1, 4, 2))
        check(r, c, 0, f"set {name}, empty list", targets=())
    c = case_ref(oracle, NAME, RECEIVER, 67, 33, SETS["F"])
    check(r, c, 0, "set F, sorted", targets=(0, 2, 4, 7))
    c = case_ref(oracle, NAME, RECEIVER, 67, 33, SETS["B"])
    check(r, c, 0, "set B, permuted", targets=(5, 0, 3, 1, 4, 2))


@gpu
def test_materials_play_no_part(halart, oracle, renderers):
    """translucent blocks and an invisible wall: the bytes of the opaque scene"""
    from test_gpu_parity import make_renderer
    s, _ = TA.translucent_carpets()
    r = make_renderer(halart, s, 16, 16)
    for name in ("A", "B", "C"):
        check(r, case_ref(oracle, NAME, RECEIVER, 67, 33, SETS[name]), 0, f"set {name}, translucent")
    r.close()


@gpu
def test_two_calls_give_the_same_bytes(halart, oracle, renderers):
    """another transfer, a bake and an atlas in between reuse the renderer's buffers"""
    r = renderers(NAME)
    c = case_ref(oracle, NAME, RECEIVER, 67, 33, SETS["F"])
    first = call(r, c, 3)
    call(r, case_ref(oracle, NAME, RECEIVER, 128, 3, SETS["B"]))
    r.bake_occlusion(7, 96, 40, 33, 11)
    second = call(r, c, 3)
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()


@gpu
def test_frames_around_a_transfer_are_unchanged(halart, oracle):
    """update, transfer, update: the transfer shares the renderer's scratch; images 0-3 are those of a run without it, bit for bit"""
    from test_gpu_parity import make_renderer
    base = TB.scene_ref(oracle, NAME, TA.carpets)
    images = []
    for with_transfer in (False, True):
        r = make_renderer(halart, base.scene, 32, 32)
        r.update(); r.render()
        if with_transfer:
            check(r, case_ref(oracle, NAME, RECEIVER, 67, 33, SETS["F"]), 3, "between frames")
        r.update(); r.render()
        images.append([r.read_image(which).tobytes() for which in range(4)])
        r.close()
    assert images[0] == images[1]


@gpu
def test_after_moving_the_target_node_and_a_refit(halart, oracle):
    """the mirrored carpet lowered, turned and scaled, then refit: the records equal a twin of the edited scene"""
    from test_gpu_parity import make_renderer
    s, _ = TA.carpets()
    r = make_renderer(halart, s, 16, 16, build=dict(instancing=False))
    k = [i for i, nd in enumerate(s.nodes) if nd.name == "mirrored carpet"][0]
    m = (TB.carpet_transform().astype(f64) @ SE._rot(ry=0.5, rx=0.2).astype(f64) @ np.diag([-0.8, 1.5, 1.1, 1.0]))
    m[:3, 3] = (300.0, 120.0, 250.0)
    ops = [("node", k, m.astype(f32))]
    w, h = 67, 33
    flags, front, back, targets = SETS["A"]
    before = r.bake_transfer(RECEIVER, w, h, front, back, targets, **TB.FLAG_KW[flags])
    same_bytes(before[0], case_ref(oracle, NAME, RECEIVER, w, h, SETS["A"]).rec, "before the edit")
    SE.apply_to_renderer(r, ops)
    r.refit()
    edited = SE.apply_to_scene(s, ops)
    osc = oracle.OracleScene(edited)
    want_r, want_t = TR.Twin(BR.Twin(edited, osc), osc).transfer(RECEIVER, w, h, flags, front, back, targets)
    assert want_r.tobytes() != before[0].reshape(-1).tobytes() and (want_r["prim"] >= 160).sum() > 100
    got_r, got_t = r.bake_transfer(RECEIVER, w, h, front, back, targets, **TB.FLAG_KW[flags])
    same_bytes(got_r, want_r, "records after the refit")
    same_bytes(got_t, want_t, "texels after the refit")
    r.close()


@gpu
def test_refusals(halart, oracle):
    """every refusal raises with its message, leaves last_error's owner, the prefilled output buffers and the next frame as they were"""
    import torch
    from test_gpu_parity import make_renderer
    from test_instance_levels import instance_scene
    base = TB.scene_ref(oracle, NAME, TA.carpets)
    plain = make_renderer(halart, base.scene, 32, 32)
    plain.update(); plain.render(); plain.update(); plain.render()
    want_images = [plain.read_image(which).tobytes() for which in range(4)]
    plain.close()
    r = make_renderer(halart, base.scene, 32, 32)
    r.update(); r.render()
    n = 16 * 16
    d_o = torch.full((n * 32,), 0xAB, dtype=torch.uint8, device="cuda")
    d_t = torch.full((n * 16,), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    fresh = halart.HalaRenderer("uncommitted", 16, 16, 5, 3, False, False, False, 0)
    alone = make_renderer(halart, one_instance(), 16, 16)
    oracle.set_instancing(True)
    try:
        two = make_renderer(halart, instance_scene(2, True), 16, 16, build=dict(instancing=True))
    finally:
        oracle.set_instancing(False)
    assert two.bvh_info().instance_ref_count > 0

    def desc(**kw):
        d = dict(instance=RECEIVER, width=16, height=16, flags=1, bias=0.0, reach=INF, margin=0)
        d.update(kw)
        return A.BakeDesc(d["instance"], d["width"], d["height"], d["flags"], d["bias"], d["reach"], d["margin"])

    def tdesc(front=200.0, back=50.0, flags=0, target_count=0):
        return A.BakeTransferDesc(front, back, flags, target_count)

    keep = []

    def ids(*t):
        keep.append(np.array(t, dtype=np.uint32))
        return keep[-1]

    def device_call(who, d, t, targets=None, out=d_o.data_ptr()):
        return who._lib.hala_rt_bake_transfer(who._h, C.byref(d) if d is not None else None, C.byref(t) if t is not None else None,
                                              C.c_void_p(targets.ctypes.data) if targets is not None else None, C.c_void_p(out), C.c_void_p(d_t.data_ptr()), None)
    h_o, h_t = np.full(n, 0xAB, dtype=np.uint8).repeat(32), np.full(n, 0xCD, dtype=np.uint8).repeat(16)

    def host_call(who, d, t, targets=None, out=None):
        out = h_o.ctypes.data if out is None else out
        return who._lib.hala_rt_bake_transfer_host(who._h, C.byref(d) if d is not None else None, C.byref(t) if t is not None else None,
                                                   C.c_void_p(targets.ctypes.data) if targets is not None else None, C.c_void_p(out), C.c_void_p(h_t.ctypes.data))
    cases = [(r, None, tdesc(), {}, "description is null"), (r, desc(), tdesc(), dict(out=0), "output is null"), (fresh, desc(), tdesc(), {}, "acceleration structure"),
             (two, desc(instance=0), tdesc(), {}, "two-level"), (r, desc(instance=8), tdesc(), {}, "instance is out of range"),
             (r, desc(width=0), tdesc(), {}, "dimensions"), (r, desc(height=4097), tdesc(), {}, "dimensions"), (r, desc(margin=17), tdesc(), {}, "margin"),
             (r, desc(flags=4), tdesc(), {}, "Unknown bake flags"), (r, desc(bias=np.nan), tdesc(), {}, "bias"), (r, desc(bias=np.inf), tdesc(), {}, "bias"),
             (r, desc(), None, {}, "transfer description is null"), (r, desc(), tdesc(flags=1), {}, "transfer flags"),
             (r, desc(), tdesc(front=np.nan), {}, "front distance"), (r, desc(), tdesc(front=np.inf), {}, "front distance"),
             (r, desc(), tdesc(front=-1.0), {}, "front distance"), (r, desc(), tdesc(back=np.nan), {}, "back distance"),
             (r, desc(), tdesc(back=-0.5), {}, "back distance"), (r, desc(), tdesc(back=-np.inf), {}, "back distance"),
             (r, desc(), tdesc(target_count=9), dict(targets=ids(0, 1, 2, 3, 4, 5, 7, 0, 1)), "target count"),
             (r, desc(), tdesc(target_count=2), {}, "target list is null"),
             (r, desc(), tdesc(target_count=2), dict(targets=ids(0, 8)), "out of range"),
             (r, desc(), tdesc(target_count=2), dict(targets=ids(0xFFFFFFFF, 1)), "out of range"),
             (r, desc(), tdesc(target_count=3), dict(targets=ids(4, 5, 4)), "named twice"),
             (r, desc(), tdesc(target_count=2), dict(targets=ids(7, 6)), "receiver"),
             (alone, desc(instance=0), tdesc(), {}, "no targets")]
    for who, d, t, kw, match in cases:
        for form in (device_call, host_call):
            with pytest.raises(halart.HalaRendererError, match=match):
                who._check(form(who, d, t, **kw))
    with pytest.raises(halart.HalaRendererError, match="margin"):
        r.bake_transfer(RECEIVER, 16, 16, 10.0, margin=20)
    with pytest.raises(halart.HalaRendererError, match="two-level"):
        two.bake_transfer(0, 8, 8, 1.0)
    with pytest.raises(halart.HalaRendererError, match="receiver"):
        r.bake_transfer(RECEIVER, 8, 8, 1.0, targets=[RECEIVER])
    r.wait_idle()
    torch.cuda.synchronize()
    assert bool((d_o == 0xAB).all()) and bool((d_t == 0xCD).all()) and (h_o == 0xAB).all() and (h_t == 0xCD).all()
    fresh.close(); two.close(); alone.close()
    r.update(); r.render()
    assert [r.read_image(which).tobytes() for which in range(4)] == want_images
    check(r, case_ref(oracle, NAME, RECEIVER, 8, 8, SETS["A"]), 0, "after the refusals")  # still usable
    r.close()


@gpu
def test_python_forms_and_stream_order(halart, oracle, renderers):
    """(H, W) shapes and dtypes; back=None is front; device tensors for the outputs on a second stream, with and without texel records;
    a transfer on a side stream right behind an occlusion bake on the renderer's stream (both use the rasteriser's scratch and the sample
    buffer): each gives the bytes of the call made alone"""
    import torch
    w, h = 67, 33
    r = renderers("transfer_gutter")
    c = case_ref(oracle, "transfer_gutter", RECEIVER, w, h, SETS["A"])
    want_r, want_t = BR.dilate(c.rec, c.texels, w, h, 3)
    rec, texels = r.bake_transfer(RECEIVER, w, h, 200.0, 50.0, margin=3, shading_normal=True)
    assert rec.shape == texels.shape == (h, w) and rec.dtype == A.BAKE_TRANSFER_HIT_DTYPE and texels.dtype == A.BAKE_TEXEL_DTYPE
    same_bytes(rec, want_r, "host form")
    same = case_ref(oracle, "transfer_gutter", RECEIVER, w, h, (1, 30.0, 30.0, None))
    same_bytes(r.bake_transfer(RECEIVER, w, h, 30.0, shading_normal=True)[0], same.rec, "back=None is front")
    n = w * h
    d_o = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    d_t = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    d_ao = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    alone_ao = r.bake_occlusion(7, w, h, 33, 11, margin=2)[0]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    assert r.bake_occlusion(7, w, h, 33, 11, margin=2, out=d_ao) is None  # the renderer's stream; no synchronisation before the next call
    assert r.bake_transfer(RECEIVER, w, h, 200.0, 50.0, margin=3, shading_normal=True, out=d_o, out_texels=d_t, stream=side.cuda_stream) is None
    torch.cuda.synchronize()
    assert d_ao.cpu().numpy().tobytes() == alone_ao.tobytes(), "the bake ahead of the transfer"
    assert d_o.cpu().numpy().tobytes() == want_r.tobytes() and d_t.cpu().numpy().tobytes() == want_t.tobytes(), "the transfer behind it"
    d_o.zero_()
    torch.cuda.synchronize()
    r.bake_transfer(RECEIVER, w, h, 200.0, 50.0, margin=3, shading_normal=True, out=d_o.data_ptr())  # raw pointer, no texel records
    r.wait_idle()
    assert d_o.cpu().numpy().tobytes() == want_r.tobytes()
    with pytest.raises(ValueError, match="too small"):
        r.bake_transfer(RECEIVER, w, h, 1.0, out=d_o[:64])
    with pytest.raises(ValueError, match="too small"):
        r.bake_transfer(RECEIVER, w, h, 1.0, out=d_o, out_texels=d_t[:64])
