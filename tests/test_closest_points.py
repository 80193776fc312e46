"""Closest-point query batches (docs/RENDER_SPEC.md 4.8): hala_rt_closest_points against the numpy twin of tests/closest_point_ref.py,
all 32 bytes of every record.

CPU tier: the ABI surface is there; the twin is tied to a float64 evaluation of the same regions on every scene and query set used
below (no query left out); and the twin's own output shows what a comparison needs in order to mean something: every region, misses by
radius, ties decided by the triangle id, exact zeros.
GPU tier: both tree forms (LDS-staged, large one-level) with every builder, the limits, the refusals, the device-pointer form on a second
stream, determinism, the neighbours (frames around a batch), refits.

Margins of the float64 comparison, in units of ulp32(max(amax, max|p|)), the largest seen over all scenes and sets below: 2.29 for the
twin's distance against the float64 minimum (points on `stacked_sheets(512)`), 1.11 for the float64 distance to the twin's triangle
against that minimum (10^4 diagonals from `stacked_sheets(512)`); asserted at twice that, for platform differences in numpy's
summation order.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import closest_point_ref as CR
import hala_renderer_amd as H
import ray_conditioning as RC
from hala_renderer_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = H._abi
f32 = np.float32
FUNCTIONS = ("hala_rt_closest_points", "hala_rt_closest_points_host")
BUILDERS = ("sah", "ploc", "lbvh")
DISTANCE_MARGIN_ULP = 2 * 2.29   # the twin's distance against the float64 minimum
TRIANGLE_MARGIN_ULP = 2 * 1.11   # the float64 distance to the twin's triangle against the float64 minimum


def duplicated(scene):
    """every mesh node a second time: every answer becomes a tie between two ids"""
    nodes = []
    for nd in scene.nodes:
        nodes.append(nd)
        if nd.mesh_index != A.INVALID_INDEX:
            nodes.append(H.HalaNode(name=nd.name + "_again", parent=nd.parent, local_transform=np.array(nd.local_transform, dtype=f32), mesh_index=nd.mesh_index))
    assert all(nd.parent is None for nd in scene.nodes)
    scene.nodes = nodes
    return scene


def two_blobs():
    s = RC.blob_scene(3)
    m = np.eye(4, dtype=f32); m[:3, 3] = (3.0, 0.5, -1.0)
    s.nodes.insert(1, H.HalaNode(name="blob_b", mesh_index=0, local_transform=m))
    return s


SCENES = {  # name -> (scene, tree form)
    "cornell": (scenes.cornell_box, "staged"),
    "cornell_dup": (lambda: duplicated(scenes.cornell_box()), "staged"),
    "blob": (lambda: RC.blob_scene(3), "large"),
    "blob_dup": (lambda: duplicated(RC.blob_scene(3)), "large"),
    "sheets512": (lambda: scenes.stacked_sheets(512), "large"),
}

_REF = {}


class Reference:
    pass


def reference(oracle, name):
    """scene, triangles, queries (about 4 000: the six point sets, radii dealt out over them) and the twin's answer: computed once,
    shared by every test and left unchanged"""
    if name not in _REF:
        k = list(SCENES).index(name)
        ref = Reference()
        ref.scene = SCENES[name][0]()
        ref.tris = CR.scene_triangles(ref.scene, oracle.OracleScene(ref.scene))
        ref.points, ref.sets, ref.diag = CR.point_sets(*ref.tris, seed=100 + k)
        ref.queries = CR.with_radii(ref.points, ref.diag, seed=200 + k)
        ref.twin = CR.Twin(*ref.tris)
        ref.answer = ref.twin.answer(ref.queries)
        _REF[name] = ref
    return _REF[name]


_CONDITIONS = {}


def check_conditions(oracle):
    """what the twin's output over the query sets together must show before any result is compared"""
    if not _CONDITIONS:
        regions = np.zeros(7, np.int64); misses = ties = zeros = 0
        for name in SCENES:
            ans = reference(oracle, name).answer
            hit = ans.rec["prim"] != CR.MISS
            regions += np.bincount(ans.rec["region"][hit], minlength=7)
            misses += int(ans.by_radius.sum())
            ties += int((ans.ties & hit).sum())
            zeros += int((ans.rec["distance"][hit] == 0.0).sum())
        _CONDITIONS.update(regions=regions.tolist(), misses=misses, ties=ties, zeros=zeros)
    c = _CONDITIONS
    assert min(c["regions"]) >= 50 and c["misses"] >= 100 and c["ties"] >= 50 and c["zeros"] >= 50, c
    return c


# ---- CPU tier ------------------------------------------------------------------------------------------------------------------------
def test_abi_surface(halart):
    """the header, the export list, the Python and Rust declarations and the library name the functions and the two records"""
    header = open(os.path.join(ROOT, "include", "halart.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    rust = open(os.path.join(ROOT, "rust", "hala-renderer-halart", "src", "lib.rs")).read()
    lib = C.CDLL(halart.LIB_PATH)
    for fn in FUNCTIONS:
        assert re.search(rf"\bint {fn}\s*\(", code), fn
        assert fn in A.EXPORTS and fn in A.PROTOTYPES, fn
        assert f"fn {fn}(" in rust, fn
        assert hasattr(lib, fn), fn
    assert re.search(r"typedef struct hala_point_query \{\s*float point\[3\];\s*float radius;\s*\} hala_point_query;", code)
    assert re.search(r"typedef struct hala_closest_point \{\s*float distance;\s*float u;\s*float v;\s*uint32_t prim;\s*float point\[3\];\s*uint32_t region;\s*\} hala_closest_point;", code)
    assert C.sizeof(A.PointQuery) == 16 and A.POINT_QUERY_DTYPE.itemsize == 16
    assert C.sizeof(A.ClosestPoint) == 32 and A.CLOSEST_POINT_DTYPE.itemsize == 32
    assert [f[0] for f in A.ClosestPoint._fields_] == list(A.CLOSEST_POINT_DTYPE.names)
    assert "pub struct hala_point_query" in rust and "pub struct hala_closest_point" in rust
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*typedef struct hala_point_query", header, flags=re.S)
    assert m and "RENDER_SPEC 4.8" in m.group(1) and "Not built" in m.group(1), "cites its section of the spec and names what is not built"
    assert callable(halart.HalaRenderer.closest_points)
    spec = open(os.path.join(ROOT, "docs", "RENDER_SPEC.md")).read()
    assert "### 4.8 Closest-point queries (no reference equivalent)" in spec


def test_reference_shows_regions_misses_ties_and_zeros(oracle):
    print(check_conditions(oracle))


@pytest.mark.parametrize("name", list(SCENES))
def test_twin_against_float64(oracle, name):
    """every point of every set, without its radius: the twin's distance against the float64 minimum over all triangles, and the float64
    distance to the triangle the twin names against that minimum, in ulp32(max(amax, max|p|))"""
    ref = reference(oracle, name)
    ans = ref.answer
    assert (ans.free_prim != CR.MISS).all(), "without a limit every point has an answer"
    least, to_prim = ref.twin.float64(ref.queries, ans.free_prim)
    v0, e1, e2 = ref.tris
    amax = max(np.abs(v0).max(), np.abs((v0 + e1).astype(f32)).max(), np.abs((v0 + e2).astype(f32)).max())
    ulp = np.spacing(np.maximum(f32(amax), np.abs(ref.points).max(axis=1)).astype(f32)).astype(np.float64)
    dev_distance = np.abs(ans.free_distance.astype(np.float64) - least) / ulp
    dev_triangle = np.abs(to_prim - least) / ulp
    for k, rng in enumerate(ref.sets):
        print(f"{name} set {k}: distance {dev_distance[rng].max():.3f} ulp, triangle {dev_triangle[rng].max():.3f} ulp")
    assert dev_distance.max() <= DISTANCE_MARGIN_ULP, (name, dev_distance.max())
    assert dev_triangle.max() <= TRIANGLE_MARGIN_ULP, (name, dev_triangle.max())
    # a limited query answers like the unlimited one or not at all
    hit = ans.rec["prim"] != CR.MISS
    assert np.array_equal(ans.rec["prim"][hit], ans.free_prim[hit]) and np.array_equal(ans.rec["distance"][hit], ans.free_distance[hit])
    rad = ref.queries["radius"]
    assert not hit[~(rad >= 0)].any(), "a NaN or negative radius admits nothing"
    assert hit[np.isinf(rad) | (rad == f32(3.402823466e38))].all(), "+inf and FLT_MAX are no limit"


def test_twin_records(oracle):
    """the twin's bookkeeping on the duplicated Cornell box: every answer a tie that the lower id wins, miss records as the spec writes
    them, the reported point is fma(v, e2, fma(u, e1, v0)) of the named triangle and the region matches (u, v)"""
    ref = reference(oracle, "cornell_dup")
    rec, ans = ref.answer.rec, ref.answer
    hit = rec["prim"] != CR.MISS
    assert ans.ties[hit].all()
    miss = rec[~hit]
    assert len(miss) >= 100 and miss.tobytes() == np.array([(-1.0, 0.0, 0.0, CR.MISS, (0.0, 0.0, 0.0), 0)] * len(miss), dtype=A.CLOSEST_POINT_DTYPE).tobytes()
    u, v, region = rec["u"][hit], rec["v"][hit], rec["region"][hit]
    assert ((u == 0) & (v == 0))[region == 4].all() and ((u == 1) & (v == 0))[region == 5].all() and ((u == 0) & (v == 1))[region == 6].all()
    assert (v[region == 1] == 0).all() and (u[region == 2] == 0).all() and (u[region == 3] == (f32(1.0) - v[region == 3])).all()
    v0, e1, e2 = (x[rec["prim"][hit]] for x in ref.tris)
    q = CR.fma(v[:, None], e2, CR.fma(u[:, None], e1, v0))
    assert q.tobytes() == rec["point"][hit].tobytes()


# ---- GPU tier ------------------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def renderers(halart, oracle):
    """one committed renderer per (scene, builder), closed when the module is done"""
    from test_gpu_parity import make_renderer
    made = {}

    def get(name, builder=None):
        if (name, builder) not in made:
            made[(name, builder)] = make_renderer(halart, reference(oracle, name).scene, 16, 16, build=dict(builder=builder))
        return made[(name, builder)]
    yield get
    for r in made.values():
        r.close()


def assert_form(r, form):
    i = r.bvh_info()
    assert i.instance_ref_count == 0
    assert (i.lds_node_count > 0) == (form == "staged"), form


def assert_equals_twin(got, want, queries, what):
    if got.tobytes() != want.tobytes():
        bad = np.nonzero((got.view(np.uint32).reshape(len(got), 8) != want.view(np.uint32).reshape(len(want), 8)).any(axis=1))[0]
        i = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} records differ; first query {i} {queries[i]}: got {got[i]} want {want[i]}")


@gpu
@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("name", list(SCENES))
def test_answers_equal_the_twin(halart, oracle, renderers, name, builder):
    check_conditions(oracle)
    ref = reference(oracle, name)
    r = renderers(name, builder)
    assert_form(r, SCENES[name][1])
    got = r.closest_points(ref.queries)
    assert_equals_twin(got, ref.answer.rec, ref.queries, f"{name} {builder}")


@gpu
@pytest.mark.parametrize("name", ["cornell", "blob"])
def test_python_forms_and_determinism(halart, oracle, renderers, name):
    """points + one radius, points + a radius each, and the same batch twice: the same bytes"""
    ref = reference(oracle, name)
    r = renderers(name)
    want = ref.answer.rec
    first, second = r.closest_points(ref.queries), r.closest_points(ref.queries)
    assert first.tobytes() == second.tobytes() == want.tobytes()
    assert r.closest_points(ref.points, ref.queries["radius"]).tobytes() == want.tobytes()
    unlimited = r.closest_points(ref.points)
    assert np.array_equal(unlimited["prim"], ref.answer.free_prim) and np.array_equal(unlimited["distance"], ref.answer.free_distance)


@gpu
def test_count_zero_and_refusals(halart, oracle, renderers):
    """count == 0 is a no-op; a null batch, an uncommitted renderer and a two-level tree raise and leave a prefilled buffer as it was"""
    import torch
    from test_gpu_parity import make_renderer
    ref = reference(oracle, "cornell")
    r = renderers("cornell")
    n = 64
    d_q = torch.from_numpy(ref.queries[:n].view(np.uint8).copy()).cuda()
    d_out = torch.full((n * 32,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    fresh = halart.HalaRenderer("uncommitted", 16, 16, 5, 3, False, False, False, 0)
    instanced = make_renderer(halart, two_blobs(), 16, 16, build=dict(instancing=True))
    assert instanced.bvh_info().instance_ref_count > 0
    for who, args, match in ((r, (0, d_out.data_ptr(), n), "null"), (r, (d_q.data_ptr(), 0, n), "null"),
                             (fresh, (d_q.data_ptr(), d_out.data_ptr(), n), "acceleration structure"),
                             (instanced, (d_q.data_ptr(), d_out.data_ptr(), n), "two-level")):
        with pytest.raises(halart.HalaRendererError, match=match):
            who._check(who._lib.hala_rt_closest_points(who._h, C.c_void_p(args[0]), C.c_void_p(args[1]), C.c_uint32(args[2]), None))
    with pytest.raises(halart.HalaRendererError, match="two-level"):
        instanced.closest_points(ref.points[:n])
    with pytest.raises(halart.HalaRendererError, match="acceleration structure"):
        fresh.closest_points(ref.points[:n])
    r.closest_points(d_q, out=d_out, count=0)
    assert len(r.closest_points(np.zeros((0, 3), f32))) == 0
    r.wait_idle(); instanced.wait_idle()
    torch.cuda.synchronize()
    assert bool((d_out == 0xAB).all())
    fresh.close(); instanced.close()


@gpu
def test_device_pointer_form_on_a_second_stream(halart, oracle, renderers):
    import torch
    ref = reference(oracle, "blob")
    r = renderers("blob")
    d_q = torch.from_numpy(ref.queries.view(np.uint8).copy()).cuda()
    d_out = torch.zeros(len(ref.queries) * 32, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    r.closest_points(d_q, out=d_out, stream=side.cuda_stream)
    side.synchronize()
    assert d_out.cpu().numpy().tobytes() == ref.answer.rec.tobytes()
    d_out.zero_()
    torch.cuda.synchronize()
    r.closest_points(d_q.data_ptr(), out=d_out.data_ptr(), count=len(ref.queries))  # raw pointers, the renderer's stream
    r.wait_idle()
    assert d_out.cpu().numpy().tobytes() == ref.answer.rec.tobytes()


@gpu
@pytest.mark.parametrize("name", ["cornell", "blob"])
def test_frames_around_a_batch_are_unchanged(halart, oracle, name):
    """update, batch, update: the batch shares the renderer's scratch; images 0-3 are those of a run without the batch, bit for bit"""
    from test_gpu_parity import make_renderer
    ref = reference(oracle, name)
    images = []
    for with_batch in (False, True):
        r = make_renderer(halart, ref.scene, 32, 32)
        r.update(); r.render()
        if with_batch:
            assert_equals_twin(r.closest_points(ref.queries), ref.answer.rec, ref.queries, f"between frames, {name}")
        r.update(); r.render()
        images.append([r.read_image(which).tobytes() for which in range(4)])
        r.close()
    assert images[0] == images[1]


def edited_reference(r, seed):
    """the twin on the triangles the renderer holds after a refit (hala_rt_download_bvh), with queries made from them"""
    tris = CR.bvh_triangles(r.download_bvh()[1])
    points, _, diag = CR.point_sets(*tris, seed=seed, sizes=(300, 200, 300, 400, 100, 100))
    queries = CR.with_radii(points, diag, seed + 1)
    return tris, queries, CR.Twin(*tris).answer(queries)


@gpu
def test_after_a_node_refit(halart, oracle):
    """update_node_transform + refit on the flattened two_blobs: the answers are the twin's on the edited triangles"""
    from test_gpu_parity import make_renderer
    r = make_renderer(halart, two_blobs(), 16, 16, build=dict(instancing=False))
    assert r.bvh_info().instance_ref_count == 0
    before = CR.bvh_triangles(r.download_bvh()[1])
    m = np.eye(4, dtype=f32); m[:3, :3] *= f32(0.75); m[:3, 3] = (1.5, 0.25, -0.5)  # into the other blob
    r.update_node_transform(0, m)
    r.refit()
    tris, queries, ans = edited_reference(r, 31)
    assert not np.array_equal(tris[0], before[0]) and (ans.rec["prim"] != CR.MISS).sum() >= 500
    assert_equals_twin(r.closest_points(queries), ans.rec, queries, "node refit")
    r.close()


@gpu
def test_after_a_deformer_refit(halart, oracle):
    """a posed morph target + refit on the blob: the answers are the twin's on the posed triangles"""
    from test_gpu_parity import make_renderer
    s = RC.blob_scene(3)
    r = make_renderer(halart, s, 16, 16)
    before = CR.bvh_triangles(r.download_bvh()[1])
    pos = np.asarray(s.meshes[0].primitives[0].vertices["position"], dtype=f32)
    delta = (pos * (0.3 * np.sin(5.0 * pos[:, 1:2]))).astype(f32)
    r.set_deformer(0, 0, targets=delta[None])
    r.update_deformer(0, 0, morph_weights=[0.7])
    r.refit()
    tris, queries, ans = edited_reference(r, 41)
    assert not np.array_equal(tris[0], before[0]) and (ans.rec["prim"] != CR.MISS).sum() >= 500
    assert_equals_twin(r.closest_points(queries), ans.rec, queries, "deformer refit")
    r.close()
