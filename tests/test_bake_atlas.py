"""Bake atlases (docs/RENDER_SPEC.md 4.12): hala_rt_bake_atlas_samples and hala_rt_bake_atlas_occlusion against the numpy twin of
tests/bake_atlas_ref.py, every byte of every sample, texel record and occlusion record.

The scene is test_bake's Cornell box with two carpets (instance 6: an 8 x 8 grid; instance 7: a 4 x 4 grid under a mirrored node) and the
layout puts three instances into one map: 6 at scale (0.5, 0.5) offset (0, 0), 7 at (0.25, 0.5) offset (0.625, 0.25) and instance 0 (the
box's quads over the unit square) at (0.375, 0.25) offset (0.125, 0.625).  The sizes are the smallest that have empty, full and partial
8 x 8 blocks, widths that are no multiple of 8 or 64, a map one block high and a map of one texel; OWNED below is what the twin gives
there, asserted on the CPU and again on what the GPU returns.

CPU tier: the ABI surface; the twin is telling (the table, the identity chart is the 4.11 map, an overlap goes to the lower id, a mirrored
chart, a zero scale and an off-map offset, per-chart flags).
GPU tier: the layout on every size with mixed flags and N = 1, 33, 64, 256; bake_atlas_occlusion against occlusion(bake_atlas_samples)
and the twin's dilation — the listed pass against the unlisted one; all empty, all owned, clipped and overlapping charts; the identity
chart against bake_occlusion; a translucent and an invisible material on a staged and on a large tree (the any-hit key is the texel's:
a key taken from the list position shows here, a stream taken from it shows in every test); every builder; determinism, frames around
a bake, a refit; the refusals; the Python forms."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bake_atlas_ref as AR
import bake_ref as BR
import hala_renderer_amd as H
import scene_edits as SE
import test_bake as TB
from test_bake import BIAS, MISS, REACH, SEED, same_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = H._abi
f32, f64 = np.float32, np.float64
FUNCTIONS = ("hala_rt_bake_atlas_samples", "hala_rt_bake_atlas_samples_host", "hala_rt_bake_atlas_occlusion", "hala_rt_bake_atlas_occlusion_host")
SIZES = ((1, 1), (8, 8), (64, 64), (67, 33), (96, 40), (128, 3))
RAYS = {(1, 1): 256, (8, 8): 256, (64, 64): 33, (67, 33): 64, (96, 40): 1, (128, 3): 33}
# (instance, scale, offset, flags): the shading normal on the first carpet, the flipped triangle normal on the mirrored one, the triangle's on the box
LAYOUT = ((6, (0.5, 0.5), (0.0, 0.0), 1), (7, (0.25, 0.5), (0.625, 0.25), 2), (0, (0.375, 0.25), (0.125, 0.625), 0))
PLAIN = tuple((i, s, o, 0) for i, s, o, _ in LAYOUT)
# map -> (owned texels, (empty, full, partial) 8 x 8 blocks or None)
OWNED = {(64, 64): (1920, (34, 30, 0)), (67, 33): (1075, (17, 10, 18)), (96, 40): (1800, (20, 14, 26)), (128, 3): (208, (4, 0, 12)), (8, 8): (30, None),
         (1, 1): (1, None)}
IDENTITY = ((6, (1.0, 1.0), (0.0, 0.0), 0),)
OVERLAP = ((6, (0.5, 0.5), (0.1, 0.1), 0), (7, (0.5, 0.5), (0.3, 0.3), 0))
MIRRORED = ((6, (-0.5, 0.5), (0.75, 0.25), 0),)
OFF_MAP = ((6, (0.5, 0.5), (2.0, 2.0), 0), (7, (0.25, 0.25), (-1.0, 0.25), 1))
CLIPPED = ((6, (1.5, 1.5), (-0.25, 0.3), 1),)
NAME = "atlas_carpets"


def carpets():
    return TB.in_cornell(TB.chart(8), extra=TB.chart(4))


def translucent_carpets():
    """the blocks' material translucent (opacity 0.5) and the red wall's invisible (0), as in test_occlusion.translucent_cornell"""
    s, inst = carpets()
    s.materials[4].opacity = 0.5
    s.materials[1].opacity = 0.0
    return s, inst


def translucent_blob():
    """the chart under the blob (a large one-level tree) with the blob translucent: the chart gets an opaque material of its own"""
    s, inst = TB.in_blob(TB.chart(16))
    blob_material = s.meshes[0].primitives[0].material_index
    s.materials.append(H.HalaMaterial(type=0, base_color=(0.7, 0.7, 0.7)))
    s.meshes[-1].primitives[0].material_index = len(s.materials) - 1
    s.materials[blob_material].opacity = 0.5
    return s, inst


_ATLAS, _REC = {}, {}


def atlas_ref(oracle, name, charts, w, h, make=carpets):
    """(atlas twin, samples, texels) of a layout on a map: computed once, shared and left unchanged"""
    key = (name, charts, w, h)
    if key not in _ATLAS:
        base = TB.scene_ref(oracle, name, make)
        atlas = AR.Atlas(base.twin, charts)
        _ATLAS[key] = (atlas,) + atlas.samples(w, h, bias=BIAS, reach=REACH)
    return _ATLAS[key]


def records_ref(oracle, name, charts, w, h, n_rays, make=carpets):
    """the undilated occlusion records of the atlas' samples, sample i being texel i: once"""
    key = (name, charts, w, h, n_rays)
    if key not in _REC:
        _, samples, _ = atlas_ref(oracle, name, charts, w, h, make)
        _REC[key] = TB.trace_twin(TB.scene_ref(oracle, name, make).osc, samples, n_rays, SEED)
    return _REC[key]


def blocks_of(owned, w, h):
    """(empty, full, partial) 8 x 8 blocks of an ownership map; a block cut by the map's edge is never full"""
    ob = owned.reshape(h, w)
    e = f = p = 0
    for y in range(0, h, 8):
        for x in range(0, w, 8):
            b = ob[y:y + 8, x:x + 8]
            if not b.any():
                e += 1
            elif b.all() and b.size == 64:
                f += 1
            else:
                p += 1
    return e, f, p


def instance_of(twin, prim):
    return np.searchsorted(twin.first, prim, side="right") - 1


# ---- CPU tier ------------------------------------------------------------------------------------------------------------------------
def test_abi_surface(halart):
    """the header, the export list, the Python declarations, the Rust binding and the built library name the four functions and the two
    records; the spec has its section; the 4.11 lists no longer call compaction not built"""
    header = open(os.path.join(ROOT, "include", "halart.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    rust = open(os.path.join(ROOT, "rust", "hala-renderer-halart", "src", "lib.rs")).read()
    lib = C.CDLL(halart.LIB_PATH)
    for fn in FUNCTIONS:
        assert re.search(rf"\bint {fn}\s*\(", code), fn
        assert fn in A.EXPORTS and fn in A.PROTOTYPES, fn
        assert f"fn {fn}(" in rust, fn
        assert hasattr(lib, fn), fn
    assert "pub struct hala_bake_chart" in rust and "pub struct hala_bake_atlas_desc" in rust
    assert re.search(r"typedef struct hala_bake_chart \{\s*uint32_t instance;\s*uint32_t flags;\s*float scale\[2\];\s*float offset\[2\];\s*\} hala_bake_chart;", code)
    assert re.search(r"typedef struct hala_bake_atlas_desc \{\s*uint32_t width, height;\s*float bias, reach;\s*uint32_t margin;\s*uint32_t chart_count;\s*\} "
                     r"hala_bake_atlas_desc;", code)
    assert C.sizeof(A.BakeChart) == 24 and C.sizeof(A.BakeAtlasDesc) == 24 and A.BAKE_CHART_DTYPE.itemsize == 24
    assert [f[0] for f in A.BakeChart._fields_] == ["instance", "flags", "scale", "offset"] == list(A.BAKE_CHART_DTYPE.names)
    assert [A.BAKE_CHART_DTYPE.fields[n][1] for n in A.BAKE_CHART_DTYPE.names] == [getattr(A.BakeChart, n).offset for n in A.BAKE_CHART_DTYPE.names]
    assert [f[0] for f in A.BakeAtlasDesc._fields_] == ["width", "height", "bias", "reach", "margin", "chart_count"]
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*typedef struct hala_bake_chart", header, flags=re.S)
    assert m and "RENDER_SPEC 4.12" in m.group(1) and "Not built" in m.group(1), "cites its section of the spec and names what is not built"
    assert callable(halart.HalaRenderer.bake_atlas_samples) and callable(halart.HalaRenderer.bake_atlas_occlusion)
    spec = open(os.path.join(ROOT, "docs", "RENDER_SPEC.md")).read()
    assert "### 4.12 Bake atlases (no reference equivalent)" in spec
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "compaction of empty texels" not in header and "compaction of empty texels" not in spec.split("### 4.12")[0].split("### 4.11")[1]
    assert re.search(r"^## 31\.", design, flags=re.M)


@pytest.mark.parametrize("size", SIZES)
def test_the_layout_owns_what_the_table_says(oracle, size):
    """owned texels and empty / full / partial blocks of the layout on every size; all three instances own texels from 8 x 8 up"""
    w, h = size
    atlas, samples, texels = atlas_ref(oracle, NAME, LAYOUT, w, h)
    owned = texels["prim"] != MISS
    want, blocks = OWNED[size]
    assert int(owned.sum()) == want
    if blocks is not None:
        assert blocks_of(owned, w, h) == blocks
    if w * h > 1:
        assert set(instance_of(atlas, texels["prim"][owned]).tolist()) == {0, 6, 7}
    assert not samples[~owned].view(np.uint8).any() and (texels["source"][owned] == np.nonzero(owned)[0]).all()


@pytest.mark.parametrize("size", TB.MAPS)
def test_the_identity_chart_is_the_bake_map(oracle, size):
    """scale (1, 1), offset (0, 0): owners, samples and texel records of RENDER_SPEC 4.11 (the carpet's UVs hold no negative zero)"""
    w, h = size
    base = TB.scene_ref(oracle, NAME, carpets)
    assert not np.signbit(base.twin.uv[base.twin.first[6]:base.twin.first[7]][base.twin.uv[base.twin.first[6]:base.twin.first[7]] == 0]).any()
    for flags in (0, 3):
        atlas = AR.Atlas(base.twin, ((6, (1.0, 1.0), (0.0, 0.0), flags),))
        owner = atlas.owners(w, h)
        assert np.array_equal(owner, base.twin.owners(6, w, h))
        got = atlas.samples(w, h, bias=BIAS, reach=REACH, owner=owner)
        want = base.twin.samples(6, w, h, flags=flags, bias=BIAS, reach=REACH, owner=owner)
        same_bytes(got[0], want[0], f"samples {size} flags {flags}")
        same_bytes(got[1], want[1], f"texels {size} flags {flags}")


def test_overlap_mirror_zero_scale_and_off_map(oracle):
    """two charts that overlap: 1024 and 663 texels, the lower instance (the lower ids) wins, and instance 7 alone owns 1024; a mirrored
    chart owns its full 1024 with area < 0; a zero scale and offsets off the map own nothing"""
    base = TB.scene_ref(oracle, NAME, carpets)
    atlas, _, texels = atlas_ref(oracle, NAME, OVERLAP, 64, 64)
    owned = texels["prim"] != MISS
    assert np.bincount(instance_of(atlas, texels["prim"][owned]), minlength=8).tolist() == [0, 0, 0, 0, 0, 0, 1024, 663]
    alone = AR.Atlas(base.twin, OVERLAP[1:]).owners(64, 64)
    assert int((alone != MISS).sum()) == 1024
    both = owned & (alone != MISS) & (instance_of(atlas, np.where(owned, texels["prim"], 0)) == 6)
    assert int(both.sum()) == 1024 - 663, "the texels both cover go to instance 6"
    mirrored = AR.Atlas(base.twin, MIRRORED)
    owner = mirrored.owners(64, 64)
    assert int((owner != MISS).sum()) == 1024
    area = mirrored.at_owner(owner, 64, 64)[0]
    assert (area[owner != MISS] < 0).all()
    for charts in (OFF_MAP, ((6, (0.0, 0.5), (0.5, 0.25), 0),), ((6, (0.5, 0.0), (0.25, 0.5), 0), (7, (0.0, 0.0), (0.5, 0.5), 0))):
        assert (AR.Atlas(base.twin, charts).owners(67, 33) == MISS).all(), charts


def test_per_chart_flags_change_their_own_chart_only(oracle):
    """the layout with mixed flags against the layout with none: points, texel records and the box's normals are the same bytes, the first
    carpet's normals are unit shading normals, the mirrored carpet's are the triangle normals negated"""
    atlas, mixed, texels = atlas_ref(oracle, NAME, LAYOUT, 67, 33)
    _, plain, texels0 = atlas_ref(oracle, NAME, PLAIN, 67, 33)
    assert texels.tobytes() == texels0.tobytes() and mixed["point"].tobytes() == plain["point"].tobytes()
    owned = texels["prim"] != MISS
    inst = np.where(owned, instance_of(atlas, np.where(owned, texels["prim"], 0)), -1)
    assert mixed["normal"][inst == 0].tobytes() == plain["normal"][inst == 0].tobytes()
    assert np.array_equal(mixed["normal"][inst == 7], -plain["normal"][inst == 7]) and (inst == 7).sum() > 50
    n6 = mixed["normal"][inst == 6]
    assert np.allclose(np.linalg.norm(n6.astype(f64), axis=1), 1.0, atol=1e-6) and (np.abs(n6 - plain["normal"][inst == 6]).max(axis=1) > 1e-3).all()


# ---- GPU tier ------------------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def renderer(halart, oracle):
    """the committed carpets scene, shared by the tests that do not edit it"""
    from test_gpu_parity import make_renderer
    r = make_renderer(halart, TB.scene_ref(oracle, NAME, carpets).scene, 16, 16)
    assert r.bvh_info().instance_ref_count == 0 and r.bvh_info().lds_node_count > 0, "a one-level tree staged in LDS"
    yield r
    r.close()


def check_atlas(oracle, r, name, charts, w, h, n_rays, margin=0, make=carpets, what=""):
    """samples, texel records and (n_rays > 0) occlusion records of one atlas against the twin, byte for byte"""
    atlas, samples, texels = atlas_ref(oracle, name, charts, w, h, make)
    table = atlas.table()
    got_s, got_t = r.bake_atlas_samples(table, w, h, bias=BIAS, reach=REACH)
    assert got_s.shape == got_t.shape == (h, w)
    same_bytes(got_s, samples, f"samples {name} {w} x {h} {what}")
    same_bytes(got_t, texels, f"texels {name} {w} x {h} {what}")
    if n_rays:
        rec = records_ref(oracle, name, charts, w, h, n_rays, make)
        want_r, want_t = BR.dilate(rec, texels, w, h, margin) if margin else (rec, texels)
        got_r, got_t = r.bake_atlas_occlusion(table, w, h, n_rays, SEED, margin=margin, bias=BIAS, reach=REACH)
        same_bytes(got_r, want_r, f"records {name} {w} x {h} N = {n_rays} margin {margin} {what}")
        same_bytes(got_t, want_t, f"texels of the records {name} {w} x {h} margin {margin} {what}")
    return samples, texels


@gpu
@pytest.mark.parametrize("size", SIZES)
def test_the_layout_equals_the_twin(halart, oracle, renderer, size):
    """three instances with mixed flags in one map, every size, N = 1, 33, 64 or 256: empty, full and partial blocks in the list"""
    w, h = size
    _, texels = check_atlas(oracle, renderer, NAME, LAYOUT, w, h, RAYS[size])
    assert int((texels["prim"] != MISS).sum()) == OWNED[size][0]
    rec = records_ref(oracle, NAME, LAYOUT, w, h, RAYS[size])
    assert ((rec["visibility"] >= 0) == (texels["prim"] != MISS)).all()


def test_list_positions_are_not_texel_indices(oracle):
    """what the GPU tests rest on: on the 67 x 33 layout nearly no owned texel sits at a list position equal to its index (in row-major or
    in block-major order), so a stream or a key taken from the position cannot give the texel's record by accident"""
    _, samples, texels = atlas_ref(oracle, NAME, LAYOUT, 67, 33)
    owned = texels["prim"] != MISS
    row_major = np.nonzero(owned)[0]
    assert (row_major != np.arange(len(row_major))).mean() > 0.9
    y, x = np.divmod(row_major, 67)
    block_major = row_major[np.lexsort((x & 7, y & 7, x >> 3, y >> 3))]
    assert (block_major != np.arange(len(block_major))).mean() > 0.9


@gpu
def test_atlas_occlusion_is_samples_then_occlusion_then_dilation(halart, oracle, renderer):
    """on one renderer: the listed pass against the unlisted one.  Margin 0 equals occlusion(bake_atlas_samples(...)) byte for byte, margins
    1 and 16 the twin's dilation of that over the whole atlas"""
    w, h = 67, 33
    atlas, want_s, want_t = atlas_ref(oracle, NAME, LAYOUT, w, h)
    table = atlas.table()
    samples, texels = renderer.bake_atlas_samples(table, w, h, bias=BIAS, reach=REACH)
    same_bytes(samples, want_s, "samples")
    for n_rays in (33, 64):
        own = renderer.occlusion(samples.reshape(-1), rays=n_rays, seed=SEED)
        for margin in (0, 1, 16):
            want_r, want_tex = BR.dilate(own, texels.reshape(-1), w, h, margin)
            got_r, got_t = renderer.bake_atlas_occlusion(table, w, h, n_rays, SEED, margin=margin, bias=BIAS, reach=REACH)
            same_bytes(got_r, want_r, f"N = {n_rays} margin {margin}")
            same_bytes(got_t, want_tex, f"texels, N = {n_rays} margin {margin}")
            if margin == 0:
                empty = texels["prim"].reshape(-1) == MISS
                assert 0.3 < empty.mean() < 0.7 and (got_r["visibility"].reshape(-1)[empty] == -1).all()
            else:
                assert ((want_tex["source"] != MISS) & (texels["prim"].reshape(-1) == MISS)).any()


@gpu
@pytest.mark.parametrize("case", ["empty", "full", "clipped", "overlap", "mirrored"])
def test_extremes(halart, oracle, renderer, case):
    """every chart off the map: every record is (-1, 0, 0, 0), texel records (0, 0, ~0, ~0), also with a margin (a list of no entries); one
    chart that fills the map: every block full but the cut ones; one clipped by the map's edge; overlapping charts; a mirrored one"""
    w, h = 67, 33
    charts = dict(empty=OFF_MAP, full=((7, (1.0, 1.0), (0.0, 0.0), 2),), clipped=CLIPPED, overlap=OVERLAP, mirrored=MIRRORED)[case]
    _, texels = check_atlas(oracle, renderer, NAME, charts, w, h, 33, margin=3 if case in ("empty", "clipped") else 0, what=case)
    owned = texels["prim"] != MISS
    if case == "empty":
        assert not owned.any()
        rec, tex = renderer.bake_atlas_occlusion(AR.Atlas(TB.scene_ref(oracle, NAME).twin, charts).table(), w, h, 256, SEED, margin=16)
        assert (rec["visibility"] == -1).all() and not rec["bent"].any() and (tex["prim"] == MISS).all() and (tex["source"] == MISS).all()
    elif case == "full":
        assert owned.all()
    else:
        assert 0.1 < owned.mean() < 0.9


@gpu
@pytest.mark.parametrize("size", [(64, 64), (67, 33)])
def test_the_identity_chart_equals_bake_occlusion(halart, oracle, renderer, size):
    """one chart, scale (1, 1), offset (0, 0): the bytes of hala_rt_bake_occlusion of that instance, which runs the unlisted pass"""
    w, h = size
    for inst, kw, flags in ((6, dict(shading_normal=True), 1), (0, {}, 0)):
        table = np.array([(inst, flags, (1.0, 1.0), (0.0, 0.0))], dtype=A.BAKE_CHART_DTYPE)
        want = renderer.bake_occlusion(inst, w, h, 33, SEED, margin=3, bias=BIAS, reach=REACH, **kw)
        got = renderer.bake_atlas_occlusion(table, w, h, 33, SEED, margin=3, bias=BIAS, reach=REACH)
        same_bytes(got[0], want[0], f"records, instance {inst}")
        same_bytes(got[1], want[1], f"texels, instance {inst}")
        assert (want[1]["prim"] != MISS).all()


@gpu
def test_translucent_and_invisible_materials(halart, oracle):
    """the ALPHA instantiations: a translucent triangle stops a ray by a draw from the ray's any-hit key, pcg((i * N + j) ^ ...) of texel i,
    so a key taken from the list position changes records here; on the staged Cornell tree and on the large tree under the blob"""
    from test_gpu_parity import make_renderer
    for name, make, charts, staged in (("atlas_alpha", translucent_carpets, LAYOUT, True),
                                       ("atlas_alpha_blob", translucent_blob, None, False)):
        base = TB.scene_ref(oracle, name, make)
        if charts is None:
            charts = ((base.instance, (0.5, 0.75), (0.25, 0.125), 1),)
        r = make_renderer(halart, base.scene, 16, 16)
        assert (r.bvh_info().lds_node_count > 0) == staged and r.bvh_info().instance_ref_count == 0
        w, h, n_rays = (67, 33, 64) if staged else (40, 24, 33)
        check_atlas(oracle, r, name, charts, w, h, n_rays, make=make, what=name)
        rec = records_ref(oracle, name, charts, w, h, n_rays, make)
        part = (rec["visibility"] > 0) & (rec["visibility"] < 1)
        assert part.sum() >= 32, "texels that see part of the sky"
        r.close()
    # the translucent triangles matter: the same atlas with them opaque gives other records
    opaque = records_ref(oracle, NAME, LAYOUT, 67, 33, 64)
    assert (records_ref(oracle, "atlas_alpha", LAYOUT, 67, 33, 64, translucent_carpets)["visibility"] != opaque["visibility"]).sum() >= 32


@gpu
@pytest.mark.parametrize("builder", TB.BUILDERS)
def test_trees_and_builders(halart, oracle, builder):
    """the staged Cornell tree and the large one-level tree under the blob, by every builder: the same bytes"""
    from test_gpu_parity import make_renderer
    r = make_renderer(halart, TB.scene_ref(oracle, NAME, carpets).scene, 16, 16, build=dict(builder=builder))
    check_atlas(oracle, r, NAME, LAYOUT, 67, 33, 64, what=builder)
    r.close()
    make = lambda: TB.in_blob(TB.chart(16))  # noqa: E731
    base = TB.scene_ref(oracle, "atlas_blob", make)
    charts = ((base.instance, (0.5, 0.75), (0.25, 0.125), 1),)
    r = make_renderer(halart, base.scene, 16, 16, build=dict(builder=builder))
    assert r.bvh_info().lds_node_count == 0 and r.bvh_info().instance_ref_count == 0
    check_atlas(oracle, r, "atlas_blob", charts, 40, 24, 33, margin=1, make=make, what=f"blob {builder}")
    rec = records_ref(oracle, "atlas_blob", charts, 40, 24, 33, make)
    assert 0.02 < (rec["visibility"] == 0).mean() < 0.9, "part of the chart lies inside the blob"
    r.close()


@gpu
def test_two_calls_give_the_same_bytes(halart, oracle, renderer):
    """the list is block-major and its offsets a prefix sum: nothing depends on the order of the atomics; another atlas and a plain bake in
    between reuse the renderer's buffers"""
    table = AR.Atlas(TB.scene_ref(oracle, NAME).twin, OVERLAP).table()
    first = renderer.bake_atlas_occlusion(table, 67, 33, 33, SEED, margin=3, bias=BIAS, reach=REACH)
    renderer.bake_atlas_occlusion(AR.Atlas(TB.scene_ref(oracle, NAME).twin, LAYOUT).table(), 128, 3, 64, SEED)
    renderer.bake_occlusion(6, 96, 40, 33, SEED)
    second = renderer.bake_atlas_occlusion(table, 67, 33, 33, SEED, margin=3, bias=BIAS, reach=REACH)
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
    third = renderer.bake_atlas_occlusion(table, 67, 33, 33, SEED + 1, margin=3, bias=BIAS, reach=REACH)
    assert third[0].tobytes() != first[0].tobytes() and third[1].tobytes() == first[1].tobytes()


@gpu
def test_frames_around_an_atlas_bake_are_unchanged(halart, oracle):
    """update, bake, update: the bake shares the renderer's scratch; images 0-3 are those of a run without it, bit for bit"""
    from test_gpu_parity import make_renderer
    base = TB.scene_ref(oracle, NAME, carpets)
    images = []
    for with_bake in (False, True):
        r = make_renderer(halart, base.scene, 32, 32)
        r.update(); r.render()
        if with_bake:
            check_atlas(oracle, r, NAME, LAYOUT, 67, 33, 64, what="between frames")
        r.update(); r.render()
        images.append([r.read_image(which).tobytes() for which in range(4)])
        r.close()
    assert images[0] == images[1]


@gpu
def test_after_moving_a_charted_node_and_a_refit(halart, oracle):
    """the first carpet lifted, turned and scaled, then refit: the atlas equals the twin of the edited scene"""
    from test_gpu_parity import make_renderer
    s, _ = carpets()
    r = make_renderer(halart, s, 16, 16, build=dict(instancing=False))
    k = [i for i, nd in enumerate(s.nodes) if nd.name == "carpet"][0]
    m = (TB.carpet_transform().astype(f64) @ SE._rot(ry=0.5, rx=0.2).astype(f64) @ np.diag([0.8, 1.5, 1.1, 1.0]))
    m[:3, 3] = (300.0, 120.0, 250.0)
    ops = [("node", k, m.astype(f32))]
    w, h = 67, 33
    table = AR.Atlas(TB.scene_ref(oracle, NAME, carpets).twin, LAYOUT).table()
    before = r.bake_atlas_occlusion(table, w, h, 33, SEED, bias=BIAS, reach=REACH)
    SE.apply_to_renderer(r, ops)
    r.refit()
    edited = SE.apply_to_scene(s, ops)
    osc = oracle.OracleScene(edited)
    samples, texels = AR.Atlas(BR.Twin(edited, osc), LAYOUT).samples(w, h, bias=BIAS, reach=REACH)
    rec = TB.trace_twin(osc, samples, 33, SEED)
    assert rec.tobytes() != before[0].reshape(-1).tobytes()
    got_s, _ = r.bake_atlas_samples(table, w, h, bias=BIAS, reach=REACH)
    same_bytes(got_s, samples, "samples after the refit")
    got_r, got_t = r.bake_atlas_occlusion(table, w, h, 33, SEED, bias=BIAS, reach=REACH)
    same_bytes(got_r, rec, "records after the refit")
    same_bytes(got_t, texels, "texels after the refit")
    r.close()


@gpu
def test_refusals(halart, oracle):
    """every refusal raises with its message, leaves prefilled output buffers as they were and the next frame as it would have been"""
    import torch
    from test_gpu_parity import make_renderer
    from test_instance_levels import instance_scene
    base = TB.scene_ref(oracle, NAME, carpets)
    plain = make_renderer(halart, base.scene, 32, 32)
    plain.update(); plain.render(); plain.update(); plain.render()
    want_images = [plain.read_image(which).tobytes() for which in range(4)]
    plain.close()
    r = make_renderer(halart, base.scene, 32, 32)
    r.update(); r.render()
    n = 16 * 16
    d_s = torch.full((n * 32,), 0xAB, dtype=torch.uint8, device="cuda")
    d_o = torch.full((n * 16,), 0xAB, dtype=torch.uint8, device="cuda")
    d_t = torch.full((n * 16,), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    fresh = halart.HalaRenderer("uncommitted", 16, 16, 5, 3, False, False, False, 0)
    oracle.set_instancing(True)
    try:
        two = make_renderer(halart, instance_scene(2, True), 16, 16, build=dict(instancing=True))
    finally:
        oracle.set_instancing(False)
    assert two.bvh_info().instance_ref_count > 0

    def desc(**kw):
        d = dict(width=16, height=16, bias=BIAS, reach=REACH, margin=0, chart_count=2)
        d.update(kw)
        return A.BakeAtlasDesc(d["width"], d["height"], d["bias"], d["reach"], d["margin"], d["chart_count"])

    def table(*rows):
        t = np.zeros(max(len(rows), 1), dtype=A.BAKE_CHART_DTYPE)
        for k, row in enumerate(rows):
            t[k] = row
        return t
    good = table((6, 1, (0.5, 0.5), (0.0, 0.0)), (7, 0, (0.5, 0.5), (0.5, 0.5)))
    keep = [good]

    def samples_call(who, d, t, out=d_s.data_ptr()):
        return who._lib.hala_rt_bake_atlas_samples(who._h, C.byref(d) if d is not None else None, C.c_void_p(t.ctypes.data) if t is not None else None,
                                                   C.c_void_p(out), C.c_void_p(d_t.data_ptr()), None)

    def occlusion_call(who, d, t, rays=16, out=d_o.data_ptr()):
        return who._lib.hala_rt_bake_atlas_occlusion(who._h, C.byref(d) if d is not None else None, C.c_void_p(t.ctypes.data) if t is not None else None,
                                                     C.c_uint32(rays), C.c_uint32(SEED), C.c_void_p(out), C.c_void_p(d_t.data_ptr()), None)

    def bad(row, other=(7, 0, (0.5, 0.5), (0.5, 0.5))):
        keep.append(table(row, other))
        return keep[-1]
    nine = table(*[(i % 8, 0, (0.1, 0.1), (0.1 * i, 0.0)) for i in range(9)])
    common = [(r, None, good, {}, "description is null"), (r, desc(), None, {}, "chart table is null"), (r, desc(), good, dict(out=0), "output is null"),
              (fresh, desc(), good, {}, "acceleration structure"), (two, desc(chart_count=1), good, {}, "two-level"),
              (r, desc(chart_count=0), good, {}, "chart count"), (r, desc(chart_count=9), nine, {}, "chart count"),
              (r, desc(), bad((8, 0, (0.5, 0.5), (0.0, 0.0))), {}, "instance is out of range"),
              (r, desc(), bad((0xFFFFFFFF, 0, (0.5, 0.5), (0.0, 0.0))), {}, "instance is out of range"),
              (r, desc(), bad((7, 0, (0.5, 0.5), (0.0, 0.0))), {}, "two charts"),
              (r, desc(), bad((6, 4, (0.5, 0.5), (0.0, 0.0))), {}, "flags"), (r, desc(), bad((6, 0x80000001, (0.5, 0.5), (0.0, 0.0))), {}, "flags"),
              (r, desc(), bad((6, 0, (np.nan, 0.5), (0.0, 0.0))), {}, "scale and offset"), (r, desc(), bad((6, 0, (0.5, np.inf), (0.0, 0.0))), {}, "scale and offset"),
              (r, desc(), bad((6, 0, (0.5, 0.5), (0.0, np.nan))), {}, "scale and offset"), (r, desc(), bad((6, 0, (0.5, 0.5), (-np.inf, 0.0))), {}, "scale and offset"),
              (r, desc(width=0), good, {}, "dimensions"), (r, desc(height=0), good, {}, "dimensions"), (r, desc(width=4097), good, {}, "dimensions"),
              (r, desc(height=4097), good, {}, "dimensions"), (r, desc(margin=17), good, {}, "margin"), (r, desc(bias=np.nan), good, {}, "bias"),
              (r, desc(bias=np.inf), good, {}, "bias")]
    for who, d, t, kw, match in common:
        for call in (samples_call, occlusion_call):
            with pytest.raises(halart.HalaRendererError, match=match):
                who._check(call(who, d, t, **kw))
    for d, rays, match in ((desc(), 0, "1..256"), (desc(), 257, "1..256"), (desc(width=4096, height=4096), 256, "too large")):
        with pytest.raises(halart.HalaRendererError, match=match):
            r._check(occlusion_call(r, d, good, rays))
    with pytest.raises(halart.HalaRendererError, match="margin"):
        r.bake_atlas_occlusion(good, 16, 16, 16, margin=20)
    with pytest.raises(halart.HalaRendererError, match="two-level"):
        two.bake_atlas_samples([(0, (1, 1), (0, 0))], 8, 8)
    r.wait_idle()
    torch.cuda.synchronize()
    assert bool((d_s == 0xAB).all()) and bool((d_o == 0xAB).all()) and bool((d_t == 0xCD).all())
    fresh.close(); two.close()
    r.update(); r.render()
    assert [r.read_image(which).tobytes() for which in range(4)] == want_images
    check_atlas(oracle, r, NAME, LAYOUT, 8, 8, 256, what="after the refusals")  # still usable
    r.close()


@gpu
def test_python_forms(halart, oracle, renderer):
    """(H, W) shapes; charts as a sequence of tuples; bias=None is the scene's ray_eps; device tensors for the outputs on a second stream,
    with and without texel records"""
    import torch
    w, h = 67, 33
    r = renderer
    atlas, want_s, want_t = atlas_ref(oracle, NAME, LAYOUT, w, h)
    rows = [(i, s, o, bool(fl & 1), bool(fl & 2)) for i, s, o, fl in LAYOUT]
    assert r._bake_charts(rows).tobytes() == atlas.table().tobytes() and r._bake_charts([(6, (1, 1), (0, 0))])["flags"][0] == 0
    samples, texels = r.bake_atlas_samples(rows, w, h)
    assert samples.shape == texels.shape == (h, w) and samples.dtype == A.OCCLUSION_SAMPLE_DTYPE and texels.dtype == A.BAKE_TEXEL_DTYPE
    owned = texels["prim"] != MISS
    assert (samples["bias"][owned] == r.ray_eps()).all() and (samples["reach"][owned] == np.inf).all()
    same_bytes(texels, want_t, "texels, tuples")
    want_r = records_ref(oracle, NAME, LAYOUT, w, h, 64)
    n = w * h
    d_s = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    d_o = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    d_t = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    assert r.bake_atlas_samples(rows, w, h, bias=BIAS, reach=REACH, out=d_s, out_texels=d_t, stream=side.cuda_stream) is None
    side.synchronize()
    assert d_s.cpu().numpy().tobytes() == want_s.tobytes() and d_t.cpu().numpy().tobytes() == want_t.tobytes()
    d_t.zero_()
    torch.cuda.synchronize()
    assert r.bake_atlas_occlusion(rows, w, h, 64, SEED, bias=BIAS, reach=REACH, out=d_o, out_texels=d_t, stream=side.cuda_stream) is None
    side.synchronize()
    assert d_o.cpu().numpy().tobytes() == want_r.tobytes() and d_t.cpu().numpy().tobytes() == want_t.tobytes()
    r.bake_atlas_occlusion(rows, w, h, 64, SEED, bias=BIAS, reach=REACH, out=d_t.data_ptr())  # raw pointer, no texel records
    r.wait_idle()
    assert d_t.cpu().numpy().tobytes() == want_r.tobytes()
    with pytest.raises(ValueError, match="too small"):
        r.bake_atlas_occlusion(rows, w, h, 33, out=d_o[:64])
    with pytest.raises(ValueError, match="too small"):
        r.bake_atlas_samples(rows, w, h, out=d_s, out_texels=d_t[:64])
