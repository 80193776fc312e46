"""Bake maps (docs/RENDER_SPEC.md 4.11): hala_rt_bake_samples and hala_rt_bake_occlusion against the numpy twin of tests/bake_ref.py, every
byte of every sample, texel record and occlusion record.

CPU tier: the ABI surface is there; the twin's coverage is shown to be telling (texel centres exactly on shared edges go to the lower id,
a chart's closed interior has no unowned texel on any map, mirrored or not, degenerate and NaN UVs own nothing, overlapping charts give
the lower id, a chart larger than the map is clipped, a smaller one leaves a gutter); the dilation against a plain per-texel search on a
map with two islands (ties, texels out of reach, the borders); the coverage rule against float64 edge values; the twin's occlusion on a
floor under the open sky (1), under a lid (0) and at the foot of a wall (1/2).
GPU tier: every map size of the issue for every chart, both normals and the flip, ray counts 1, 33, 64 and 256, a staged and a large
tree, every builder, an instance behind others under a rotated and under a mirrored node; needles and huge UVs, and long slivers whose
tips the rounded rule overshoots (the rasteriser's box must allow for all of them); bake_occlusion against occlusion(bake_samples)
on the same renderer; the margins; determinism; frames around a bake; a refit; the refusals; the Python forms.

The baked chart lies in the Cornell box as a bumpy carpet two units above the floor, rotated, through the feet of both blocks: texels inside
a block see nothing, texels beside one see part of the sky.  The occlusion bits of the twin come from the oracle's brute-force any-hit
trace of the rays expanded from the twin's samples (occlusion_ref), as in tests/test_occlusion.py.

The issue names "the all-zero-UV Cornell box" as the all-empty case; scenes.cornell_box() gives every quad the UVs of the unit square,
so that case is built here as it is described: the Cornell box with its texture coordinates set to zero.  The box as it comes is one more
overlapping case (three quads of instance 0 on one square: the floor's two triangles own the map).

Float64, measured (CPU tier, FLOAT64_DIFFER below and RENDER_SPEC 4.11): on the 45 maps of the float64 test (7 x 5, 64 x 64, 67 x 33 of grids
1, 4 and 64; plain, mirrored, clipped, gutter and sheared charts; 95 130 texels) the owner of one texel differs, on the 64 x 64 map of the
sheared 4 x 4 grid: float32 gives it to triangle 12, float64 to none, and the float64 edge value that decides it is 0.5 ulp32 of the larger
of the two products it is the difference of.  No texel of an axis-aligned chart differs.
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import bake_ref as BR
import hala_renderer_amd as H
import occlusion_ref as OR
import ray_conditioning as RC
import scene_edits as SE
from hala_renderer_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = H._abi
f32, f64 = np.float32, np.float64
MISS = 0xFFFFFFFF
FUNCTIONS = ("hala_rt_bake_samples", "hala_rt_bake_samples_host", "hala_rt_bake_occlusion", "hala_rt_bake_occlusion_host")
BUILDERS = ("sah", "ploc", "lbvh")
MAPS = ((1, 1), (8, 8), (64, 64), (67, 33), (128, 3))
RAY_COUNTS = (1, 33, 64)
SEED = 11
BIAS = 0.05  # five times the Cornell box's ray_eps
REACH = 150.0  # below the blocks' tops and the ceiling: the carpet's texels see all, part or nothing of what lies within it


# ---- charts and scenes ---------------------------------------------------------------------------------------------------------------
def chart(n, uv_map=None, lift=0.0, bumps=0.08):
    """scenes._grid_mesh(n, n): one chart with UVs in [0, 1]^2 over [-1, 1]^2 of the plane y = lift, geometric normal +y, with low bumps (so
    that vertex normals differ from the triangles'); uv_map: what to do to the UVs afterwards"""
    p = scenes._grid_mesh(n, n, lambda u, v: np.stack([2.0 * u - 1.0, lift + bumps * np.sin(5.0 * u) * np.cos(4.0 * v), 1.0 - 2.0 * v], 1))
    if uv_map is not None:
        p.vertices["tex_coord"] = np.asarray(uv_map(p.vertices["tex_coord"].astype(f64)), dtype=f32)
    p.material_index = 0
    return p


def merged(a, b):
    """two primitives as one: b's triangles follow a's"""
    v = np.concatenate([a.vertices, b.vertices])
    i = np.concatenate([a.indices, b.indices + np.uint32(len(a.vertices))]).astype(np.uint32)
    return H.HalaPrimitive(indices=i, vertices=v, material_index=a.material_index)


def mirror_u(uv):
    return np.stack([1.0 - uv[:, 0], uv[:, 1]], 1)


def clip_uv(uv):
    return 2.0 * uv - 0.5


def gutter_uv(uv):
    return 0.25 + 0.5 * uv


def shear_uv(uv):
    """a rotated, sheared chart inside the map: edges in general position"""
    return np.stack([0.15 + 0.55 * uv[:, 0] + 0.2 * uv[:, 1], 0.1 + 0.25 * uv[:, 0] + 0.6 * uv[:, 1]], 1)


def carpet_transform():
    c, s = math.cos(0.4), math.sin(0.4)
    m = np.eye(4)
    m[:3, :3] = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) @ np.diag([230.0, 40.0, 200.0])
    m[:3, 3] = (278.0, 2.0, 280.0)
    return m.astype(f32)


def in_cornell(prim, transform=None, extra=None):
    """(scene, instance): the Cornell box with `prim` as a carpet (the last instance but for `extra`, a second carpet under a mirrored node)"""
    s = scenes.cornell_box()
    s.meshes.append(H.HalaMesh([prim]))
    s.nodes.append(H.HalaNode(name="carpet", mesh_index=len(s.meshes) - 1, local_transform=carpet_transform() if transform is None else transform))
    if extra is not None:
        m = carpet_transform().astype(f64) @ np.diag([-1.0, 1.0, 1.0, 1.0])
        m[1, 3] = 60.0
        s.meshes.append(H.HalaMesh([extra]))
        s.nodes.append(H.HalaNode(name="mirrored carpet", mesh_index=len(s.meshes) - 1, local_transform=m.astype(f32)))
    return s, 6


def zero_uv_cornell():
    s = scenes.cornell_box()
    for m in s.meshes:
        for p in m.primitives:
            p.vertices["tex_coord"] = 0.0
    return s, 0


def in_blob(prim):
    """the chart under the blob of ray_conditioning.blob_scene(3): a large one-level tree"""
    s = RC.blob_scene(3)
    pos = np.concatenate([p.vertices["position"] for m in s.meshes for p in m.primitives]).astype(f64)
    lo, hi = pos.min(0), pos.max(0)
    m = np.eye(4)
    m[:3, :3] = np.diag([0.9 * (hi[0] - lo[0]), 0.3 * (hi[1] - lo[1]), 0.9 * (hi[2] - lo[2])])
    m[:3, 3] = (0.5 * (lo[0] + hi[0]), lo[1] + 0.2 * (hi[1] - lo[1]), 0.5 * (lo[2] + hi[2]))  # through the blob's lower part
    prim.material_index = s.meshes[0].primitives[0].material_index
    s.meshes.append(H.HalaMesh([prim]))
    s.nodes.append(H.HalaNode(name="chart", mesh_index=len(s.meshes) - 1, local_transform=m.astype(f32)))
    inst = sum(len(s.meshes[nd.mesh_index].primitives) for nd in s.nodes[:-1] if nd.mesh_index != A.INVALID_INDEX)
    return s, inst


def extreme_chart():
    """triangles whose UVs are needles (an angle of 1e-8 and of 1e-7 of a radian: texel centres beyond their tips can pass the rounded
    test), a sliver of 1e-3, one with coordinates of 10^6 (6.4 * 10^7 texels) that crosses the map, one far off the map, an exact line and
    a plain one; every triangle has its own three vertices on the carpet.  The huge one comes last: the others show through it."""
    uvs = [[(0.05, 0.05), (0.95, 0.05 + 1e-8), (0.95, 0.05)],
           [(0.1, 0.1), (0.9, 0.9), (0.9 + 1e-7, 0.9 - 1e-7)],
           [(0.1, 0.5), (0.9, 0.5), (0.9, 0.5008)],
           [(1e5, 1e5), (1e5 + 1.0, 1e5), (1e5, 1e5 + 1.0)],
           [(0.2, 0.2), (0.4, 0.4), (0.6, 0.6)],
           [(0.8, 0.1), (0.95, 0.1), (0.8, 0.25)],
           [(-1e6, 0.3), (1e6, 0.31), (0.5, 1e6)]]
    rs = np.random.RandomState(3)
    pos = np.stack([rs.uniform(-1, 1, 21), rs.uniform(0.0, 0.3, 21), rs.uniform(-1, 1, 21)], 1)
    v = scenes._vertices(pos, np.tile([0.0, 1.0, 0.0], (21, 1)), np.array(uvs, dtype=f64).reshape(21, 2))
    return H.HalaPrimitive(indices=np.arange(21, dtype=np.uint32), vertices=v, material_index=0)


# long slivers along the diagonal whose short edge lies 10 to 40 maps off the map and whose tip lies on it: the diagonal runs through texel
# centres, and the rounded rule of RENDER_SPEC 4.11 accepts centres up to 24 texels beyond the tip (found by search; the twin shows it below)
SLIVERS = {128: [[(0.4502132028215444, 0.4502132028215444), (-18.390265196735257, -18.390265196735257), (-18.390265196735257, -18.390421875640822)],
                 [(0.3813995435791039, 0.3813995435791039), (-35.59732327548661, -35.59732327548661), (-35.59732327548661, -35.59782579521699)],
                 [(0.6022805061070414, 0.6022805061070414), (-27.48085592898619, -27.48085592898619), (-27.48085592898619, -27.48310726584286)]],
           64: [[(0.34295369456993374, 0.34295369456993374), (-33.83877388601513, -33.83877388601513), (-33.83877388601513, -33.83909988571452)],
                [(0.5590298258046388, 0.5590298258046388), (-32.03148932325273, -32.03148932325273), (-32.03148932325273, -32.03181026339645)]],
           67: [[(0.63990989824366, 0.63990989824366), (-30.188223078932378, -30.188223078932378), (-30.188223078932378, -30.18862636840104)],
                [(0.3333344798783755, 0.3333344798783755), (-39.2684203891447, -39.2684203891447), (-39.2684203891447, -39.26872920016881)]]}


def sliver_chart(size):
    """the slivers of one map size, each with its own vertices on the carpet, and after them a plain triangle"""
    uvs = SLIVERS[size] + [[(0.8, 0.1), (0.95, 0.1), (0.8, 0.25)]]
    n = 3 * len(uvs)
    rs = np.random.RandomState(size)
    pos = np.stack([rs.uniform(-1, 1, n), rs.uniform(0.0, 0.3, n), rs.uniform(-1, 1, n)], 1)
    v = scenes._vertices(pos, np.tile([0.0, 1.0, 0.0], (n, 1)), np.array(uvs, dtype=f64).reshape(n, 2))
    return H.HalaPrimitive(indices=np.arange(n, dtype=np.uint32), vertices=v, material_index=0)


def beyond_the_corners(twin, instance, w, h):
    """owned texels whose centre lies more than half a texel outside the box of their owner's UV corners"""
    owner = twin.owners(instance, w, h)
    idx = np.nonzero(owner != MISS)[0]
    t = (twin.uv[owner[idx]] * np.array([w, h], f32)).astype(f32)
    px, py = (z[idx] for z in BR.centres(w, h))
    return int(((px > t[:, :, 0].max(axis=1) + 0.5) | (py > t[:, :, 1].max(axis=1) + 0.5) | (px < t[:, :, 0].min(axis=1) - 0.5) |
                (py < t[:, :, 1].min(axis=1) - 0.5)).sum())


@pytest.mark.parametrize("size", list(SLIVERS))
def test_the_rounded_rule_owns_texels_beyond_a_slivers_tip(oracle, size):
    """what the GPU case below rests on: on these maps the twin gives at least ten texels to slivers whose corners' box they lie outside of"""
    twin = plain_twin(oracle, sliver_chart(size))
    assert beyond_the_corners(twin, 0, size, size) >= 10


SCENES = {  # name -> () -> (scene, baked instance)
    "quad": lambda: in_cornell(chart(1)),
    "grid64": lambda: in_cornell(chart(64)),
    "mirrored": lambda: in_cornell(chart(8, mirror_u)),
    "clipped": lambda: in_cornell(chart(8, clip_uv)),
    "overlap": lambda: in_cornell(merged(chart(4), chart(4, lift=0.5))),
    "cornell_zero_uv": zero_uv_cornell,
}


class Reference:
    pass


_SCENE, _MAP, _OCC = {}, {}, {}


def scene_ref(oracle, name, make=None):
    """scene, oracle scene and twin: once per scene"""
    if name not in _SCENE:
        ref = Reference()
        ref.scene, ref.instance = (make or SCENES[name])()
        ref.osc = oracle.OracleScene(ref.scene)
        ref.twin = BR.Twin(ref.scene, ref.osc)
        _SCENE[name] = ref
    return _SCENE[name]


def map_ref(oracle, name, w, h, flags=0, instance=None):
    """the twin's samples and texel records of a map: computed once, shared by every test and left unchanged"""
    key = (name, w, h, flags, instance)
    if key not in _MAP:
        base = scene_ref(oracle, name)
        inst = base.instance if instance is None else instance
        okey = (name, w, h, "owner", inst)
        if okey not in _MAP:
            _MAP[okey] = base.twin.owners(inst, w, h)
        _MAP[key] = base.twin.samples(inst, w, h, flags=flags, bias=BIAS, reach=REACH, owner=_MAP[okey])
    return _MAP[key]


def trace_twin(osc, samples, n_rays, seed):
    """occlusion_ref's records of a sample buffer, the bits from the oracle's brute-force any-hit trace of the expanded batch"""
    rays, _ = OR.expand(samples, n_rays, seed)
    occluded = (osc.trace(rays, 1, brute=True)["t"] > 0).reshape(len(samples), n_rays)
    return OR.reduce(samples, n_rays, seed, occluded)[0]


def occlusion_ref(oracle, name, w, h, n_rays, flags=0, instance=None):
    """the undilated records of a map's samples: once"""
    key = (name, w, h, n_rays, flags, instance)
    if key not in _OCC:
        samples, _ = map_ref(oracle, name, w, h, flags, instance)
        _OCC[key] = trace_twin(scene_ref(oracle, name).osc, samples, n_rays, SEED)
    return _OCC[key]


def same_bytes(got, want, what):
    got, want = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        words = got.dtype.itemsize // 4
        bad = np.nonzero((got.view(np.uint32).reshape(-1, words) != want.view(np.uint32).reshape(-1, words)).any(axis=1))[0]
        i = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} records differ; first {i}: got {got[i]} want {want[i]}")


# ---- CPU tier ------------------------------------------------------------------------------------------------------------------------
def test_abi_surface(halart):
    """the header, the export list, the Python declarations, the Rust binding and the built library name the four functions, the two
    records and the limits"""
    header = open(os.path.join(ROOT, "include", "halart.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    rust = open(os.path.join(ROOT, "rust", "hala-renderer-halart", "src", "lib.rs")).read()
    lib = C.CDLL(halart.LIB_PATH)
    for fn in FUNCTIONS:
        assert re.search(rf"\bint {fn}\s*\(", code), fn
        assert fn in A.EXPORTS and fn in A.PROTOTYPES, fn
        assert f"fn {fn}(" in rust, fn
        assert hasattr(lib, fn), fn
    assert "pub struct hala_bake_desc" in rust and "pub struct hala_bake_texel" in rust
    for name, value in (("HALA_MAX_BAKE_DIM", 4096), ("HALA_MAX_BAKE_MARGIN", 16), ("HALA_BAKE_SHADING_NORMAL", 1), ("HALA_BAKE_FLIP_NORMAL", 2)):
        assert re.search(rf"#define {name} {value}u?\b", code), name
        assert f"pub const {name}: u32 = {value};" in rust, name
    assert (A.MAX_BAKE_DIM, A.MAX_BAKE_MARGIN, A.BAKE_SHADING_NORMAL, A.BAKE_FLIP_NORMAL) == (4096, 16, 1, 2)
    assert re.search(r"typedef struct hala_bake_texel \{\s*float u, v;\s*uint32_t prim;\s*uint32_t source;\s*\} hala_bake_texel;", code)
    assert re.search(r"typedef struct hala_bake_desc \{\s*uint32_t instance;\s*uint32_t width, height;\s*uint32_t flags;\s*float bias, reach;\s*"
                     r"uint32_t margin;\s*\} hala_bake_desc;", code)
    assert C.sizeof(A.BakeDesc) == 28 and C.sizeof(A.BakeTexel) == 16 and A.BAKE_TEXEL_DTYPE.itemsize == 16
    assert [f[0] for f in A.BakeDesc._fields_] == ["instance", "width", "height", "flags", "bias", "reach", "margin"]
    assert [f[0] for f in A.BakeTexel._fields_] == list(A.BAKE_TEXEL_DTYPE.names)
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*#define HALA_MAX_BAKE_DIM", header, flags=re.S)
    assert m and "RENDER_SPEC 4.11" in m.group(1) and "Not built" in m.group(1), "cites its section of the spec and names what is not built"
    assert callable(halart.HalaRenderer.bake_samples) and callable(halart.HalaRenderer.bake_occlusion)
    spec = open(os.path.join(ROOT, "docs", "RENDER_SPEC.md")).read()
    assert "### 4.11 Bake maps (no reference equivalent)" in spec
    assert "baking into a primitive's vertices or texture in one call" not in header + spec


def plain_scene(prim):
    s = H.HalaScene()
    s.materials = [H.HalaMaterial(type=0, base_color=(0.7, 0.7, 0.7))]
    prim.material_index = 0
    s.meshes = [H.HalaMesh([prim])]
    s.nodes = [H.HalaNode(name="chart", mesh_index=0)]
    return s


def plain_twin(oracle, prim):
    s = plain_scene(prim)
    return BR.Twin(s, oracle.OracleScene(s))


def covering(twin, w, h):
    """[T, P] bool: the twin's coverage of every triangle of instance 0 at every texel"""
    ids = np.arange(int(twin.first[0]), int(twin.first[1]))
    px, py = BR.centres(w, h)
    area, w0, w1, w2 = twin.edge_values(ids, w, h, px, py)
    return BR.covers(area[:, None], w0, w1, w2)


def test_centres_on_shared_edges_go_to_the_lower_id(oracle):
    """_grid_mesh(4, 4) on a 6 x 6 map: the grid lines lie at U = 1.5 k, so the texels of columns and rows 1 and 4 have their centres exactly
    on edges shared by two triangles (four at the crossings, six with the diagonals); each is covered by all of them and owned by the lowest"""
    twin = plain_twin(oracle, chart(4, bumps=0.0))
    cov = covering(twin, 6, 6)
    owner = twin.owners(0, 6, 6).reshape(6, 6)
    count = cov.sum(axis=0).reshape(6, 6)
    on_line = np.zeros((6, 6), bool)
    on_line[[1, 4], :] = True
    on_line[:, [1, 4]] = True
    assert (count[on_line] >= 2).all() and (count[~on_line] >= 1).all()
    assert (count[np.ix_([1, 4], [1, 4])] >= 4).all(), "the crossings"
    lowest = np.where(cov, np.arange(cov.shape[0])[:, None], MISS).min(axis=0).reshape(6, 6)
    assert np.array_equal(owner, lowest)
    both = cov.sum(axis=0) >= 2
    second = np.sort(np.where(cov, np.arange(cov.shape[0])[:, None], MISS), axis=0)[1].reshape(-1)
    assert (second[both] > owner.reshape(-1)[both]).all()


@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("n", [1, 4, 64])
@pytest.mark.parametrize("size", [(7, 5), (64, 64), (67, 33)])
def test_a_charts_closed_interior_is_owned(oracle, size, n, mirrored):
    """a chart that fills [0, 1]^2 owns every texel of every map (no centre is dropped between two triangles), with area > 0 and, mirrored,
    with area < 0; the owners are triangles whose float64 closed triangle contains the centre up to rounding"""
    w, h = size
    twin = plain_twin(oracle, chart(n, mirror_u if mirrored else None))
    owner = twin.owners(0, w, h)
    assert (owner != MISS).all(), (size, n, int((owner == MISS).sum()))
    area, w0, w1, w2 = twin.at_owner(owner, w, h, f64)
    assert ((area < 0) if mirrored else (area > 0)).all()
    sgn = np.sign(area)
    assert (np.minimum(np.minimum(w0, w1), w2) * sgn >= -1e-4 * np.abs(area)).all()


def test_most_triangles_of_a_fine_grid_own_nothing(oracle):
    twin = plain_twin(oracle, chart(64))
    owner = twin.owners(0, 16, 16)
    assert (owner != MISS).all()
    assert len(np.unique(owner)) <= 256 < 8192 // 16


def test_degenerate_and_nan_uvs_own_nothing(oracle):
    """a chart whose triangles are a point, a line, and NaN in one coordinate of one corner: nothing is owned; beside a good triangle only
    that one owns"""
    for kind in ("point", "line", "nan", "inf"):
        p = chart(2, bumps=0.0)
        uv = p.vertices["tex_coord"]
        if kind == "point":
            uv[:] = 0.5
        elif kind == "line":
            uv[:, 1] = uv[:, 0]
        elif kind == "nan":
            uv[:, 0] = np.where(np.arange(len(uv)) % 2 == 0, np.nan, uv[:, 0])
        else:
            uv[:, 1] = np.where(np.arange(len(uv)) % 2 == 0, np.inf, uv[:, 1])
        twin = plain_twin(oracle, p)
        owner = twin.owners(0, 9, 7)
        if kind == "inf":  # an infinite corner gives NaN or infinite edge values: whatever is owned has a valid record or none
            samples, texels = twin.samples(0, 9, 7)
            assert ((texels["prim"] == MISS) == (owner == MISS)).all()
        else:
            assert (owner == MISS).all(), kind
    good = merged(chart(1, lambda uv: np.full_like(uv, 0.25), bumps=0.0), chart(1, bumps=0.0))
    owner = plain_twin(oracle, good).owners(0, 5, 5)
    assert set(np.unique(owner)) == {2, 3}


def test_zero_uv_cornell_box_is_empty_and_the_box_as_it_comes_overlaps(oracle):
    base = scene_ref(oracle, "cornell_zero_uv")
    for inst in range(6):
        samples, texels = base.twin.samples(inst, 8, 8)
        assert (texels["prim"] == MISS).all() and not samples.view(np.uint8).any()
    s = scenes.cornell_box()
    twin = BR.Twin(s, oracle.OracleScene(s))
    owner = twin.owners(0, 8, 8)  # three quads on one square: the floor's triangles, 0 and 1
    assert set(np.unique(owner)) == {0, 1}


def test_overlapping_charts_give_the_lower_id(oracle):
    twin = plain_twin(oracle, merged(chart(4), chart(4, lift=0.5)))
    owner = twin.owners(0, 13, 11)
    assert (owner < 32).all() and len(np.unique(owner)) > 8
    assert covering(twin, 13, 11)[32:].any(axis=0).all(), "the second chart covers every texel too"


def test_a_chart_larger_than_the_map_is_clipped_and_a_smaller_one_leaves_a_gutter(oracle):
    for w, h in ((8, 8), (67, 33)):
        big = plain_twin(oracle, chart(8, clip_uv))
        owner = big.owners(0, w, h)
        assert (owner != MISS).all()
        _, texels = big.samples(0, w, h)
        # the map is the middle half of the chart: the sample points span half of the chart's [-1, 1]
        pts = big.samples(0, w, h)[0]["point"]
        assert -0.5 <= pts[:, 0].min() < -0.4 and 0.4 < pts[:, 0].max() <= 0.5
        small = plain_twin(oracle, chart(8, gutter_uv))
        owned = (small.owners(0, w, h) != MISS).reshape(h, w)
        px, py = (x.reshape(h, w) for x in BR.centres(w, h, f64))
        inside = (px >= 0.25 * w) & (px <= 0.75 * w) & (py >= 0.25 * h) & (py <= 0.75 * h)
        assert np.array_equal(owned, inside)
        assert not owned[0].any() and not owned[:, 0].any() and not owned[-1].any() and not owned[:, -1].any()


def islands():
    """two islands, u in [0.25, 0.45] and [0.6, 0.75], v in [0.25, 0.75]: on a 20 x 20 map columns 5 .. 8 and 12 .. 14 of rows 5 .. 14"""
    a = chart(2, lambda uv: np.stack([0.25 + 0.2 * uv[:, 0], 0.25 + 0.5 * uv[:, 1]], 1), bumps=0.0)
    b = chart(2, lambda uv: np.stack([0.6 + 0.15 * uv[:, 0], 0.25 + 0.5 * uv[:, 1]], 1), bumps=0.0)
    return merged(a, b)


def slow_dilation(owned, margin):
    """RENDER_SPEC 4.11 texel by texel: (source [H, W] or MISS, ties: how many texels had two candidates at the least distance)"""
    h, w = owned.shape
    source = np.full((h, w), MISS, dtype=np.uint32)
    ties = 0
    for y in range(h):
        for x in range(w):
            if owned[y, x]:
                source[y, x] = y * w + x
                continue
            cand = sorted(((xx - x) ** 2 + (yy - y) ** 2, yy * w + xx) for yy in range(max(0, y - margin), min(h, y + margin + 1))
                          for xx in range(max(0, x - margin), min(w, x + margin + 1)) if owned[yy, xx])
            if cand:
                source[y, x] = cand[0][1]
                ties += len(cand) > 1 and cand[1][0] == cand[0][0]
    return source, ties


@pytest.mark.parametrize("margin", [0, 1, 3, 16])
def test_dilation(oracle, margin):
    """the twin's dilation on the islands map against a plain search: the gap's middle column is at equal distance from both islands and
    takes the left one (the lower index), margins 1 and 3 leave texels out of reach, 16 reaches every border"""
    w = h = 20
    twin = plain_twin(oracle, islands())
    samples, texels = twin.samples(0, w, h)
    owned = (texels["prim"] != MISS).reshape(h, w)
    assert owned[5:15, 5:9].all() and owned[5:15, 12:15].all() and owned.sum() == 70
    rec = np.zeros(w * h, dtype=A.OCCLUSION_DTYPE)
    rec["visibility"] = np.where(owned.reshape(-1), np.arange(w * h) / f32(w * h), f32(-1.0))  # a record that names its texel
    rec["bent"][:, 0] = np.arange(w * h)
    out, tex = BR.dilate(rec, texels, w, h, margin)
    source, ties = slow_dilation(owned, margin)
    assert np.array_equal(tex["source"].reshape(h, w), source)
    filled = source.reshape(-1) != MISS
    assert out[filled].tobytes() == rec[source.reshape(-1)[filled]].tobytes()
    assert out[~filled].tobytes() == rec[~filled].tobytes() and (out["visibility"][~filled] == -1).all()
    for name in ("u", "v", "prim"):
        assert np.array_equal(tex[name], texels[name]), "an ownerless texel keeps its ownerless (u, v, prim)"
    unreached = int((~filled).sum())
    if margin == 0:
        assert unreached == w * h - 70 and ties == 0
    else:
        # the gap's middle column is two texels from either island
        assert (ties >= 10 and source[10, 10] == 10 * w + 8) if margin >= 2 else (ties == 0 and source[10, 10] == MISS), "equal distance: the lower index"
        assert (unreached > 0) == (margin < 16)
        assert source[0, 0] == (5 * w + 5 if margin >= 5 else MISS) and (source[0, :] != MISS).all() == (margin == 16)


@pytest.mark.parametrize("margin", [0, 1, 3, 16])
def test_dilation_on_the_gutter_map(oracle, margin):
    """the chart inside [0.25, 0.75]^2 on a 24 x 24 map (rows and columns 6 .. 17 owned, a gutter six texels wide): against the plain
    search; margins 1 and 3 leave texels out of reach, 16 reaches every border; the corner texel (0, 0) takes (6, 6)"""
    w = h = 24
    twin = plain_twin(oracle, chart(8, gutter_uv, bumps=0.0))
    samples, texels = twin.samples(0, w, h)
    owned = (texels["prim"] != MISS).reshape(h, w)
    assert owned[6:18, 6:18].all() and owned.sum() == 144
    rec = np.zeros(w * h, dtype=A.OCCLUSION_DTYPE)
    rec["visibility"] = np.where(owned.reshape(-1), np.arange(w * h) / f32(w * h), f32(-1.0))
    out, tex = BR.dilate(rec, texels, w, h, margin)
    source, _ = slow_dilation(owned, margin)
    assert np.array_equal(tex["source"].reshape(h, w), source)
    filled = source.reshape(-1) != MISS
    assert out[filled].tobytes() == rec[source.reshape(-1)[filled]].tobytes() and out[~filled].tobytes() == rec[~filled].tobytes()
    assert int((~filled).sum()) == {0: 576 - 144, 1: 576 - 14 * 14, 3: 576 - 18 * 18, 16: 0}[margin]
    assert source[0, 0] == (6 * w + 6 if margin >= 6 else MISS) and source[10, 5] == (10 * w + 6 if margin >= 1 else MISS)


# texels whose owner differs between float32 and float64 edge values, per map (kind, grid, W, H), as measured (module docstring): maps not
# listed measured 0; asserted at twice that.  ULP_FACTOR: the largest distance of such a texel from deciding otherwise — the least |float64
# edge value| among the edges of its two owners, in ulp32 of the larger of the two products the value is the difference of.
FLOAT64_DIFFER = {("sheared", 4, 64, 64): 1}
ULP_FACTOR = 0.5
FLOAT64_KINDS = {"plain": None, "mirrored": mirror_u, "clipped": clip_uv, "gutter": gutter_uv, "sheared": shear_uv}
FLOAT64_MAPS = ((7, 5), (64, 64), (67, 33))


def nearest_edge_ulps(twin, o32, o64, i, w, h):
    """of texel i, whose owners differ: the least |float64 edge value| / ulp32(larger product) over the edges of both owners"""
    px, py = BR.centres(w, h, f64)
    ratios = []
    for o in (o32[i], o64[i]):
        if o == MISS:
            continue
        (ax, ay), (bx, by), (cx, cy) = twin.corners(np.array([o]), w, h, f64)
        for (qx, qy), (rx, ry) in (((bx, by), (cx, cy)), ((cx, cy), (ax, ay)), ((ax, ay), (bx, by))):
            p1, p2 = float(((rx - qx) * (py[i] - qy))[0]), float(((ry - qy) * (px[i] - qx))[0])
            ratios.append(abs(p1 - p2) / float(np.spacing(f32(max(abs(p1), abs(p2))))))
    return min(ratios)


@pytest.mark.parametrize("kind", list(FLOAT64_KINDS))
def test_coverage_against_float64(oracle, kind):
    """the same rule with float64 edge values on the float32 corners: per map, the owners differ in at most twice the measured number of
    texels, and only where a centre is within rounding of an edge: some float64 edge value of one of the two owners there is within a few
    ulp32 of the products it is the difference of"""
    worst = 0.0
    for n in (1, 4, 64):
        twin = plain_twin(oracle, chart(n, FLOAT64_KINDS[kind], bumps=0.0))
        for w, h in FLOAT64_MAPS:
            o32, o64 = twin.owners(0, w, h), twin.owners64(0, w, h)
            bad = np.nonzero(o32 != o64)[0]
            ulps = [nearest_edge_ulps(twin, o32, o64, i, w, h) for i in bad]
            print(f"{kind} grid {n} map {w} x {h}: {len(bad)} of {w * h} texels differ from float64 ({len(bad) / (w * h):.2e})", [round(u, 3) for u in ulps])
            assert len(bad) <= 2 * FLOAT64_DIFFER.get((kind, n, w, h), 0), (kind, n, w, h, len(bad))
            worst = max([worst] + ulps)
    assert worst <= 2.0 * ULP_FACTOR, (kind, worst)


def floor_scene(occluder=None):
    """a flat floor chart (x in [0, 2], z in [-1, 1], normal +y, u along z, v along x: row 0 is the row next to x = 0) and an occluder quad"""
    p = scenes._grid_mesh(4, 4, lambda u, v: np.stack([2.0 * v, 0.0 * u, 2.0 * u - 1.0], 1))
    s = plain_scene(p)
    if occluder is not None:
        q = scenes._merge_quads([occluder])
        q.material_index = 0
        s.meshes.append(H.HalaMesh([q]))
        s.nodes.append(H.HalaNode(name="occluder", mesh_index=1))
    return s


def test_analytic_open_sky_lid_and_wall(oracle):
    """the twin's occlusion of a floor chart: nothing above it, visibility 1 in every owned texel; a large lid within reach, 0; a wall
    of half-width and height 100 along x = 0, 1/2 along its foot: row 0 of a 64 x 4 map at N = 256 is 16 384 draws, 5 sigma = 0.0195, and what
    escapes over or around the wall from 0.25 away is below 0.001"""
    def bake(s, w, h, n_rays, reach):
        osc = oracle.OracleScene(s)
        twin = BR.Twin(s, osc)
        samples, texels = twin.samples(0, w, h, bias=1e-3, reach=reach)
        assert (texels["prim"] != MISS).all() and np.allclose(samples["normal"] / np.linalg.norm(samples["normal"], axis=1)[:, None], (0, 1, 0))
        return trace_twin(osc, samples, n_rays, 3).reshape(h, w)
    assert (bake(floor_scene(), 16, 16, 64, np.inf)["visibility"] == 1).all()
    # the flattest direction has sin(elevation) = sqrt(1 - u1) >= 2^-12: it meets a lid at height 0.5 within 2048 of its origin
    lid = ((-5000, 0.5, -5000), (5000, 0.5, -5000), (5000, 0.5, 5000), (-5000, 0.5, 5000))
    assert (bake(floor_scene(lid), 16, 16, 64, 1.0e4)["visibility"] == 0).all()
    assert (bake(floor_scene(lid), 16, 16, 64, 0.25)["visibility"] == 1).all(), "the lid out of reach"
    wall = ((0, 0, -100), (0, 100, -100), (0, 100, 100), (0, 0, 100))
    rec = bake(floor_scene(wall), 64, 4, 256, np.inf)
    foot = float(rec["visibility"][0].astype(f64).mean())
    print(f"mean visibility along the wall's foot {foot:.5f}")
    assert abs(foot - 0.5) <= 0.0205
    assert (rec["bent"][0, :, 0] > 0.2).all(), "the bent normal leans away from the wall"


# ---- GPU tier ------------------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu
FLAG_KW = {0: {}, 1: dict(shading_normal=True), 2: dict(flip=True), 3: dict(shading_normal=True, flip=True)}


@pytest.fixture(scope="module")
def renderers(halart, oracle):
    """one committed renderer per (scene, builder), closed when the module is done"""
    from test_gpu_parity import make_renderer
    made = {}

    def get(name, builder=None):
        if (name, builder) not in made:
            made[(name, builder)] = make_renderer(halart, scene_ref(oracle, name).scene, 16, 16, build=dict(builder=builder))
            assert made[(name, builder)].bvh_info().instance_ref_count == 0
        return made[(name, builder)]
    yield get
    for r in made.values():
        r.close()


def check_map(oracle, r, name, w, h, n_rays, flags=0, instance=None, what=""):
    """samples, texel records and (n_rays > 0) occlusion records of one map against the twin, byte for byte"""
    base = scene_ref(oracle, name)
    inst = base.instance if instance is None else instance
    samples, texels = map_ref(oracle, name, w, h, flags, instance)
    got_s, got_t = r.bake_samples(inst, w, h, bias=BIAS, reach=REACH, **FLAG_KW[flags])
    assert got_s.shape == got_t.shape == (h, w)
    same_bytes(got_s, samples, f"samples {name} {w} x {h} flags {flags} {what}")
    same_bytes(got_t, texels, f"texels {name} {w} x {h} flags {flags} {what}")
    if n_rays:
        rec = occlusion_ref(oracle, name, w, h, n_rays, flags, instance)
        got_r, got_t = r.bake_occlusion(inst, w, h, n_rays, SEED, bias=BIAS, reach=REACH, **FLAG_KW[flags])
        same_bytes(got_r, rec, f"records {name} {w} x {h} N = {n_rays} flags {flags} {what}")
        same_bytes(got_t, texels, f"texels of the records {name} {w} x {h} {what}")
    return samples, texels


@gpu
@pytest.mark.parametrize("size", MAPS)
@pytest.mark.parametrize("name", list(SCENES))
def test_maps_equal_the_twin(halart, oracle, renderers, name, size):
    """every map size for every chart: the samples with both normals and the flip, the occlusion records at one of N = 1, 33, 64 (each N
    meets every chart and every size somewhere)"""
    w, h = size
    k = list(SCENES).index(name) + MAPS.index(size)
    r = renderers(name)
    for flags in (1, 2, 3):
        check_map(oracle, r, name, w, h, 0, flags)
    samples, texels = check_map(oracle, r, name, w, h, RAY_COUNTS[k % 3], 0)
    owned = texels["prim"] != MISS
    if name == "cornell_zero_uv":
        assert not owned.any()
    elif name in ("quad", "grid64", "mirrored", "clipped", "overlap"):
        assert owned.all()


def test_the_inputs_are_telling(oracle):
    """on the 64 x 64 map of the fine grid the carpet's texels see all, part and nothing of the sky, and the shading normal differs from
    the triangle's"""
    rec = occlusion_ref(oracle, "grid64", 64, 64, 64)
    vis = rec["visibility"]
    assert (vis >= 0).all() and (vis == 0).sum() >= 64 and (vis == 1).sum() >= 32 and ((vis > 0) & (vis < 1)).sum() >= 256, np.histogram(vis, 4)
    g, _ = map_ref(oracle, "grid64", 64, 64, 0)
    s, _ = map_ref(oracle, "grid64", 64, 64, 1)
    unit = g["normal"] / np.linalg.norm(g["normal"], axis=1)[:, None]
    assert ((unit * s["normal"]).sum(axis=1) > 0.5).all() and (np.abs(unit - s["normal"]).max(axis=1) > 1e-5).sum() >= 1024


@gpu
@pytest.mark.parametrize("flags", [0, 1, 3])
def test_ray_counts_and_normal_modes(halart, oracle, renderers, flags):
    """N = 1, 33 and 64 on the 67 x 33 map of the fine grid with the triangle's normal, the shading normal and the flipped one (which sends
    every ray into the floor two units below: visibility 0 inside the box); one 16 x 16 map at N = 256"""
    r = renderers("grid64")
    for n_rays in RAY_COUNTS:
        check_map(oracle, r, "grid64", 67, 33, n_rays, flags)
    if flags == 3:
        assert (occlusion_ref(oracle, "grid64", 67, 33, 64, 3)["visibility"] == 0).mean() > 0.5  # (a fifth of the carpet lies outside the box)
    if flags == 0:
        check_map(oracle, r, "grid64", 16, 16, 256, 0)


@gpu
def test_an_instance_behind_others_and_a_mirrored_node(halart, oracle):
    """two carpets behind the six instances of the box, the second under a node with det < 0: the ids are global ones, the points and the
    shading normals go through each node's own transform"""
    from test_gpu_parity import make_renderer
    base = scene_ref(oracle, "two_carpets", lambda: in_cornell(chart(8), extra=chart(6)))
    first = base.twin.first
    assert len(first) == 9 and first[6] == 32 and first[7] == 32 + 128 and first[8] == first[7] + 72
    assert np.linalg.det(np.asarray(base.scene.nodes[-1].local_transform, f64)[:3, :3]) < 0
    r = make_renderer(halart, base.scene, 16, 16)
    for inst in (6, 7):
        for flags in (0, 1):
            samples, texels = check_map(oracle, r, "two_carpets", 33, 17, 33 if flags else 0, flags, instance=inst)
            assert (texels["prim"] >= first[inst]).all() and (texels["prim"] < first[inst + 1]).all()
    up = map_ref(oracle, "two_carpets", 33, 17, 1, 7)[0]["normal"][:, 1]
    geo = map_ref(oracle, "two_carpets", 33, 17, 0, 7)[0]["normal"][:, 1]
    assert (up > 0.5).all() and (geo < 0).all(), "the mirror turns the triangles' winding, the normal matrix keeps the vertex normals' side"
    r.close()


@gpu
@pytest.mark.parametrize("size", [(64, 64), (67, 33)])
def test_needles_and_huge_coordinates(halart, oracle, size):
    """the rasteriser's bounding box must not change the rounded rule: needles and triangles with huge coordinates are tested against every
    texel of the map, like the brute-force twin does with every triangle; the inputs show what they are meant to (the huge triangle and the
    plain ones own texels, the far one and the line own none)"""
    from test_gpu_parity import make_renderer
    w, h = size
    base = scene_ref(oracle, "extreme", lambda: in_cornell(extreme_chart()))
    first = int(base.twin.first[base.instance])
    owners = set(np.unique(map_ref(oracle, "extreme", w, h)[1]["prim"]).tolist()) - {MISS}
    assert {first + 5, first + 6} <= owners and not ({first + 3, first + 4} & owners), owners
    r = make_renderer(halart, base.scene, 16, 16)
    check_map(oracle, r, "extreme", w, h, 33, 0)
    check_map(oracle, r, "extreme", w, h, 0, 1)
    r.close()


@gpu
@pytest.mark.parametrize("size", list(SLIVERS))
def test_texels_beyond_a_slivers_tip(halart, oracle, size):
    """long slivers whose far end is off the map and whose line runs through texel centres: the texels the rounded rule gives them beyond
    their tip, outside their corners' box, are baked as the twin bakes them"""
    from test_gpu_parity import make_renderer
    name = f"slivers{size}"
    base = scene_ref(oracle, name, lambda: in_cornell(sliver_chart(size)))
    assert beyond_the_corners(base.twin, base.instance, size, size) >= 10
    r = make_renderer(halart, base.scene, 16, 16)
    check_map(oracle, r, name, size, size, 33, 0)
    check_map(oracle, r, name, size, size, 0, 3)
    r.close()


@gpu
def test_staged_and_large_trees(halart, oracle, renderers):
    """the quad in the Cornell box is a tree staged in LDS; the chart under the blob a large one-level tree"""
    from test_gpu_parity import make_renderer
    assert renderers("quad").bvh_info().lds_node_count > 0
    check_map(oracle, renderers("quad"), "quad", 67, 33, 64, 1, what="staged")
    base = scene_ref(oracle, "blob", lambda: in_blob(chart(16)))
    r = make_renderer(halart, base.scene, 16, 16)
    i = r.bvh_info()
    assert i.lds_node_count == 0 and i.instance_ref_count == 0
    samples, texels = map_ref(oracle, "blob", 64, 64, 1)
    rec = trace_twin(base.osc, samples, 33, SEED)
    assert 0.05 < (rec["visibility"] == 0).mean() < 0.9, "part of the chart lies inside the blob"
    got_r, got_t = r.bake_occlusion(base.instance, 64, 64, 33, SEED, shading_normal=True, bias=BIAS, reach=REACH)
    same_bytes(got_r, rec, "records under the blob")
    same_bytes(got_t, texels, "texels under the blob")
    r.close()


@gpu
@pytest.mark.parametrize("builder", BUILDERS)
def test_the_answer_does_not_depend_on_the_builder(halart, oracle, renderers, builder):
    check_map(oracle, renderers("grid64", builder), "grid64", 67, 33, 33, 1, what=builder)


@gpu
def test_bake_occlusion_is_samples_then_occlusion_then_dilation(halart, oracle, renderers):
    """on one renderer: margin 0 equals occlusion(bake_samples(...)) byte for byte; margins 1, 3 and 16 equal the twin's dilation of that, on
    the islands map (ties, texels out of reach, borders) and on the gutter map in the box"""
    from test_gpu_parity import make_renderer
    cases = [("islands", lambda: in_cornell(islands()), 20, 20), ("gutter", lambda: in_cornell(chart(8, gutter_uv)), 67, 33)]
    for name, make, w, h in cases:
        base = scene_ref(oracle, name, make)
        r = make_renderer(halart, base.scene, 16, 16)
        samples, texels = r.bake_samples(base.instance, w, h, bias=BIAS, reach=REACH)
        same_bytes(samples, map_ref(oracle, name, w, h)[0], f"samples {name}")
        own = r.occlusion(samples.reshape(-1), rays=33, seed=SEED)
        same_bytes(own, occlusion_ref(oracle, name, w, h, 33), f"occlusion of the samples {name}")
        rec0, tex0 = r.bake_occlusion(base.instance, w, h, 33, SEED, margin=0, bias=BIAS, reach=REACH)
        same_bytes(rec0, own, f"margin 0 {name}")
        same_bytes(tex0, texels, f"texels, margin 0 {name}")
        empty = texels["prim"].reshape(-1) == MISS
        assert 0.3 < empty.mean() < 0.9 and (rec0["visibility"].reshape(-1)[empty] == -1).all()
        for margin in (1, 3, 16):
            want_r, want_t = BR.dilate(own, texels.reshape(-1), w, h, margin)
            got_r, got_t = r.bake_occlusion(base.instance, w, h, 33, SEED, margin=margin, bias=BIAS, reach=REACH)
            same_bytes(got_r, want_r, f"margin {margin} {name}")
            same_bytes(got_t, want_t, f"texels, margin {margin} {name}")
            filled = (want_t["source"] != MISS) & empty
            assert filled.any() and ((want_t["source"] == MISS).any() == (margin < 16 or name == "gutter"))
        r.close()


@gpu
def test_two_calls_give_the_same_bytes(halart, oracle, renderers):
    """the owner map is a minimum over ids: the order of the atomics does not show (overlapping charts, where they contend)"""
    r = renderers("overlap")
    inst = scene_ref(oracle, "overlap").instance
    first = r.bake_occlusion(inst, 67, 33, 33, SEED, margin=3, shading_normal=True, bias=BIAS, reach=REACH)
    other = r.bake_samples(inst, 128, 3)  # another map in between: the renderer's buffers are reused
    second = r.bake_occlusion(inst, 67, 33, 33, SEED, margin=3, shading_normal=True, bias=BIAS, reach=REACH)
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
    assert other[0].shape == (3, 128)
    third = r.bake_occlusion(inst, 67, 33, 33, SEED + 1, margin=3, shading_normal=True, bias=BIAS, reach=REACH)
    assert third[0].tobytes() != first[0].tobytes() and third[1].tobytes() == first[1].tobytes()


@gpu
@pytest.mark.parametrize("name", ["quad", "grid64"])
def test_frames_around_a_bake_are_unchanged(halart, oracle, name):
    """update, bake, update: the bake shares the renderer's scratch; images 0-3 are those of a run without it, bit for bit"""
    from test_gpu_parity import make_renderer
    base = scene_ref(oracle, name)
    images = []
    for with_bake in (False, True):
        r = make_renderer(halart, base.scene, 32, 32)
        r.update(); r.render()
        if with_bake:
            check_map(oracle, r, name, 67, 33, 33, 0, what="between frames")
        r.update(); r.render()
        images.append([r.read_image(which).tobytes() for which in range(4)])
        r.close()
    assert images[0] == images[1]


@gpu
def test_after_moving_the_baked_node_and_a_refit(halart, oracle):
    """the carpet lifted, turned and scaled, then refit: the bake equals the twin of the edited scene"""
    from test_gpu_parity import make_renderer
    s, inst = in_cornell(chart(8))
    r = make_renderer(halart, s, 16, 16, build=dict(instancing=False))
    k = len(s.nodes) - 1
    assert s.nodes[k].name == "carpet"
    m = (carpet_transform().astype(f64) @ SE._rot(ry=0.5, rx=0.2).astype(f64) @ np.diag([0.8, 1.5, 1.1, 1.0]))
    m[:3, 3] = (300.0, 120.0, 250.0)
    ops = [("node", k, m.astype(f32))]
    before = r.bake_occlusion(inst, 33, 17, 33, SEED, shading_normal=True, bias=BIAS, reach=REACH)
    SE.apply_to_renderer(r, ops)
    r.refit()
    edited = SE.apply_to_scene(s, ops)
    osc = oracle.OracleScene(edited)
    samples, texels = BR.Twin(edited, osc).samples(inst, 33, 17, flags=1, bias=BIAS, reach=REACH)
    rec = trace_twin(osc, samples, 33, SEED)
    assert rec.tobytes() != before[0].reshape(-1).tobytes()
    got_s, got_t = r.bake_samples(inst, 33, 17, shading_normal=True, bias=BIAS, reach=REACH)
    same_bytes(got_s, samples, "samples after the refit")
    got_r, got_t = r.bake_occlusion(inst, 33, 17, 33, SEED, shading_normal=True, bias=BIAS, reach=REACH)
    same_bytes(got_r, rec, "records after the refit")
    same_bytes(got_t, texels, "texels after the refit")
    r.close()


@gpu
def test_refusals(halart, oracle, renderers):
    """every refusal raises with its message, leaves prefilled output buffers as they were and the next frame as it would have been"""
    import torch
    from test_gpu_parity import make_renderer
    from test_instance_levels import instance_scene
    base = scene_ref(oracle, "quad")
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
        d = dict(instance=base.instance, width=16, height=16, flags=0, bias=BIAS, reach=REACH, margin=0)
        d.update(kw)
        return A.BakeDesc(d["instance"], d["width"], d["height"], d["flags"], d["bias"], d["reach"], d["margin"])

    def samples_call(who, d, out=d_s.data_ptr()):
        return who._lib.hala_rt_bake_samples(who._h, C.byref(d) if d is not None else None, C.c_void_p(out), C.c_void_p(d_t.data_ptr()), None)

    def occlusion_call(who, d, rays=16, out=d_o.data_ptr()):
        return who._lib.hala_rt_bake_occlusion(who._h, C.byref(d) if d is not None else None, C.c_uint32(rays), C.c_uint32(SEED), C.c_void_p(out),
                                               C.c_void_p(d_t.data_ptr()), None)
    common = [(r, None, {}, "description is null"), (r, desc(), dict(out=0), "output is null"), (fresh, desc(), {}, "acceleration structure"),
              (two, desc(instance=0), {}, "two-level"), (r, desc(instance=7), {}, "instance is out of range"),
              (r, desc(instance=0xFFFFFFFF), {}, "instance is out of range"), (r, desc(width=0), {}, "dimensions"), (r, desc(height=0), {}, "dimensions"),
              (r, desc(width=4097), {}, "dimensions"), (r, desc(height=4097), {}, "dimensions"), (r, desc(margin=17), {}, "margin"),
              (r, desc(flags=4), {}, "flags"), (r, desc(flags=0x80000001), {}, "flags"), (r, desc(bias=np.nan), {}, "bias"), (r, desc(bias=np.inf), {}, "bias")]
    for who, d, kw, match in common:
        for call in (samples_call, occlusion_call):
            with pytest.raises(halart.HalaRendererError, match=match):
                who._check(call(who, d, **kw))
    for d, rays, match in ((desc(), 0, "1..256"), (desc(), 257, "1..256"), (desc(width=4096, height=4096), 256, "too large"),
                           (desc(width=4096, height=2048), 512, "1..256")):
        with pytest.raises(halart.HalaRendererError, match=match):
            r._check(occlusion_call(r, d, rays))
    with pytest.raises(halart.HalaRendererError, match="margin"):
        r.bake_occlusion(base.instance, 16, 16, 16, margin=20)
    with pytest.raises(halart.HalaRendererError, match="two-level"):
        two.bake_samples(0, 8, 8)
    r.wait_idle()
    torch.cuda.synchronize()
    assert bool((d_s == 0xAB).all()) and bool((d_o == 0xAB).all()) and bool((d_t == 0xCD).all())
    fresh.close(); two.close()
    r.update(); r.render()
    assert [r.read_image(which).tobytes() for which in range(4)] == want_images
    check_map(oracle, r, "quad", 16, 16, 16, 0, what="after the refusals")  # still usable
    r.close()


@gpu
def test_python_forms(halart, oracle, renderers):
    """(H, W) shapes; bias=None is the scene's ray_eps; device tensors for the outputs on a second stream, with and without texel records"""
    import torch
    name, w, h = "grid64", 67, 33
    base = scene_ref(oracle, name)
    r = renderers(name)
    samples, texels = r.bake_samples(base.instance, w, h)
    assert samples.shape == texels.shape == (h, w) and samples.dtype == A.OCCLUSION_SAMPLE_DTYPE and texels.dtype == A.BAKE_TEXEL_DTYPE
    assert (samples["bias"] == r.ray_eps()).all() and (samples["reach"] == np.inf).all()
    want_s, want_t = map_ref(oracle, name, w, h, 1)
    same_bytes(samples, base.twin.samples(base.instance, w, h, bias=r.ray_eps(), owner=_MAP[(name, w, h, "owner", base.instance)])[0], "bias=None")
    short = r.bake_samples(base.instance, w, h, reach=25.0, bias=BIAS)[0]
    assert (short["reach"] == f32(25.0)).all() and (short["bias"] == f32(BIAS)).all()
    want_r = occlusion_ref(oracle, name, w, h, 33, 1)
    n = w * h
    d_s = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    d_o = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    d_t = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    assert r.bake_samples(base.instance, w, h, shading_normal=True, bias=BIAS, reach=REACH, out=d_s, out_texels=d_t, stream=side.cuda_stream) is None
    side.synchronize()
    assert d_s.cpu().numpy().tobytes() == want_s.tobytes() and d_t.cpu().numpy().tobytes() == want_t.tobytes()
    d_t.zero_()
    torch.cuda.synchronize()
    assert r.bake_occlusion(base.instance, w, h, 33, SEED, shading_normal=True, bias=BIAS, reach=REACH, out=d_o, out_texels=d_t, stream=side.cuda_stream) is None
    side.synchronize()
    assert d_o.cpu().numpy().tobytes() == want_r.tobytes() and d_t.cpu().numpy().tobytes() == want_t.tobytes()
    # the occlusion kernels take the baked samples where they lie: no copy between the two calls
    d_o.zero_()
    torch.cuda.synchronize()
    r.occlusion(d_s, rays=33, seed=SEED, out=d_o)
    r.bake_occlusion(base.instance, w, h, 33, SEED, shading_normal=True, bias=BIAS, reach=REACH, out=d_t.data_ptr())  # raw pointer, no texel records
    r.wait_idle()
    assert d_o.cpu().numpy().tobytes() == want_r.tobytes() and d_t.cpu().numpy().tobytes() == want_r.tobytes()
    with pytest.raises(ValueError, match="too small"):
        r.bake_occlusion(base.instance, w, h, 33, out=d_o[:64])
    with pytest.raises(ValueError, match="too small"):
        r.bake_samples(base.instance, w, h, out=d_s, out_texels=d_t[:64])
