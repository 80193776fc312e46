"""Signed distance grids (docs/RENDER_SPEC.md 4.9): hala_rt_distance_grid against the numpy twin of tests/distance_grid_ref.py, every
byte of every voxel.

CPU tier: the ABI surface is there; the twin's sign agrees with the float64 generalised winding number on the closed blobs; and the twin's
own output shows what a comparison needs in order to mean something: voxels inside, voxels the band answers, rows with 0, 2 and >= 4
crossings, a 70-voxel row with a crossing in every word of its bit array, distance ties.
GPU tier: both tree forms with every builder, methods 1, 2 and automatic, signed and unsigned, both bands; a grid too large for the twin
against hala_rt_closest_points and hala_rt_trace_rays_multi; the refusals; the device form on a second stream; the counting entry point
and which kernel an automatic grid runs; the neighbours (frames around a grid); refits.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import closest_point_ref as CR
import distance_grid_ref as DR
import hala_renderer_amd as H
import ray_conditioning as RC
from hala_renderer_amd import scenes
from test_closest_points import assert_form, duplicated, two_blobs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = H._abi
f32 = np.float32
FUNCTIONS = ("hala_rt_distance_grid", "hala_rt_distance_grid_host", "hala_rt_distance_grid_counted")
BUILDERS = ("sah", "ploc", "lbvh")
METHODS = (1, 2, None)

SCENES = {  # name -> (scene, tree form, closed surface)
    "cornell": (scenes.cornell_box, "staged", False),
    "blob2": (lambda: RC.blob_scene(2), "staged", True),
    "blob3": (lambda: RC.blob_scene(3), "large", True),
    "sheets512": (lambda: scenes.stacked_sheets(512), "large", False),
    "blob3_dup": (lambda: duplicated(RC.blob_scene(3)), "large", True),
}
SHAPES = ((13, 10, 7), (4, 4, 4), (1, 1, 1), (5, 1, 9), (70, 3, 2), (8, 2, 2))


def make_grids(mn, mx):
    """the six grids of a scene box: 1.3 boxes wide along their longest axis and centred, but (70, 3, 2), which starts 0.22 boxes before the
    box so that the box's far side falls into the third word of a row's bits, and (8, 2, 2), the far grid"""
    out = []
    for dims in SHAPES:
        if dims == (8, 2, 2):
            out.append(DR.far_grid(mn, mx, dims))
        else:
            out.append(DR.grid_over(mn, mx, dims, lead=0.22 if dims[0] == 70 else None))
    return out


def bands(grid):
    return (f32(np.inf), f32(2.0) * grid.spacing)


class Reference:
    pass


_REF = {}


def reference(oracle, name):
    """scene, triangles, twin, grids and the twin's answer for every grid and band: computed once, shared by every test, left unchanged"""
    if name not in _REF:
        ref = Reference()
        ref.scene = SCENES[name][0]()
        osc = oracle.OracleScene(ref.scene)
        ref.tris = CR.scene_triangles(ref.scene, osc)
        ref.mn, ref.mx = (np.asarray(x, np.float64) for x in osc.bounds())
        ref.twin = DR.Twin(*ref.tris, ref.mn, ref.mx)
        ref.grids = make_grids(ref.mn, ref.mx)
        ref.answers = {(gi, bi): ref.twin.answer(g, band) for gi, g in enumerate(ref.grids) for bi, band in enumerate(bands(g))}
        _REF[name] = ref
    return _REF[name]


_CONDITIONS = {}


def check_conditions(oracle):
    """what the twin's outputs together must show before anything is compared"""
    if not _CONDITIONS:
        inside = by_band = ties = 0
        crossings = set()
        every_word = False
        for name in SCENES:
            ref = reference(oracle, name)
            for (gi, bi), ans in ref.answers.items():
                by_band += int(ans.by_band.sum())
                ties += int(ans.ties.sum())
                if bi == 0:
                    inside += int(ans.inside.sum())
                    crossings |= set(int(c) for c in np.unique(ans.crossings))
                    if ref.grids[gi].dims[0] == 70:
                        every_word |= any(len(set(int(b) >> 5 for b in m)) == 3 for m in ans.m)
        _CONDITIONS.update(inside=inside, by_band=by_band, ties=ties, crossings=sorted(crossings), every_word=every_word)
    c = _CONDITIONS
    assert c["inside"] >= 50 and c["by_band"] >= 100 and c["ties"] >= 50 and c["every_word"], c
    assert 0 in c["crossings"] and 2 in c["crossings"] and max(c["crossings"]) >= 4, c
    return c


def desc_of(grid, band=np.inf, flags=1):
    return A.DistanceGridDesc((C.c_float * 3)(*[float(x) for x in grid.origin]), float(grid.spacing), (C.c_uint32 * 3)(*grid.dims), float(band), flags)


# ---- CPU tier ------------------------------------------------------------------------------------------------------------------------
def test_abi_surface(halart):
    """the header, the export list, the Python and Rust declarations and the library name the functions and the description"""
    header = open(os.path.join(ROOT, "include", "halart.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    rust = open(os.path.join(ROOT, "rust", "hala-renderer-halart", "src", "lib.rs")).read()
    lib = C.CDLL(halart.LIB_PATH)
    for fn in FUNCTIONS:
        assert re.search(rf"\bint {fn}\s*\(", code), fn
        assert fn in A.EXPORTS and fn in A.PROTOTYPES, fn
        assert f"fn {fn}(" in rust, fn
        assert hasattr(lib, fn), fn
    assert re.search(r"typedef struct hala_distance_grid_desc \{\s*float origin\[3\];\s*float spacing;\s*uint32_t dims\[3\];\s*float band;\s*uint32_t flags;\s*\} "
                     r"hala_distance_grid_desc;", code)
    assert C.sizeof(A.DistanceGridDesc) == 36
    assert [f[0] for f in A.DistanceGridDesc._fields_] == ["origin", "spacing", "dims", "band", "flags"]
    assert "pub struct hala_distance_grid_desc" in rust
    assert re.search(r"#define HALA_GRID_SIGNED 1u", code) and A.GRID_SIGNED == 1 and A.GRID_METHOD_SHIFT == 1 and A.MAX_GRID_DIM == 1024
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*typedef struct hala_distance_grid_desc", header, flags=re.S)
    assert m and "RENDER_SPEC 4.9" in m.group(1) and "Not built" in m.group(1), "cites its section of the spec and names what is not built"
    assert callable(halart.HalaRenderer.distance_grid)
    spec = open(os.path.join(ROOT, "docs", "RENDER_SPEC.md")).read()
    assert "### 4.9 Distance grids (no reference equivalent)" in spec
    assert "distance_grid.hip" in open(os.path.join(ROOT, "hala-renderer_amd", "csrc", "Makefile")).read()


def test_sign_against_the_float64_winding_number(oracle):
    """the twin's inside flag against |w| > 1/2 of the generalised winding number in float64, on the two closed blobs.  Left out: voxels
    within 1e-4 diagonals of the surface (float64) and rows within 1e-4 (barycentric) of an edge: at most 2 % of the voxels of a grid;
    at least 50 voxels inside; none disagrees"""
    inside_total = 0
    for name, dims in (("blob3", (13, 10, 7)), ("blob3", (9, 6, 5)), ("blob2", (13, 10, 7))):
        ref = reference(oracle, name)
        grid = DR.grid_over(ref.mn, ref.mx, dims)
        inside = ref.twin.rows(grid)[0]
        pts = grid.points()
        q = np.empty(len(pts), dtype=A.POINT_QUERY_DTYPE)
        q["point"] = pts; q["radius"] = np.inf
        least, _ = ref.twin.points.float64(q, np.full(len(pts), CR.MISS, np.uint32))
        diag = float(np.linalg.norm(ref.mx - ref.mn))
        nx, ny, nz = dims
        skip = (least < 1e-4 * diag).reshape(nz, ny, nx) | DR.rows_near_an_edge(*ref.tris, grid)[:, :, None]
        w = DR.winding_number(*ref.tris, pts).reshape(nz, ny, nx)
        stray = np.abs(np.abs(w) - np.round(np.abs(w)))[~skip].max()
        want = np.abs(w) > 0.5
        keep = ~skip
        print(f"{name} {dims}: {int((inside & keep).sum())} inside, {int(skip.sum())} left out, {int(((inside != want) & keep).sum())} disagree, "
              f"|w| within {stray:.1e} of an integer")
        # the records' corners v0 + e1, v0 + e2 are within an ulp32 (2^-23 relative) of the shared vertices, so the surface of records is
        # closed up to slits of that width: |w| is an integer to a few 2^-23, far below the 1/2 that decides
        assert stray < 1e-5, "a closed surface: the winding number is an integer"
        assert skip.mean() <= 0.02, (name, dims)
        assert not ((inside != want) & keep).any(), (name, dims)
        inside_total += int((inside & keep).sum())
    assert inside_total >= 50


def test_reference_shows_inside_band_crossings_words_and_ties(oracle):
    print(check_conditions(oracle))


def test_twin_bookkeeping(oracle):
    """what the twin says of special scenes: every distance of the duplicated blob is a tie and all its rows' parities are even; outside
    the band the value is the band; voxel 0 of a row is inside iff the row has an odd number of crossings"""
    dup = reference(oracle, "blob3_dup")
    for (gi, bi), ans in dup.answers.items():
        assert ans.ties[~ans.by_band].all() and not ans.inside.any() and (ans.crossings % 2 == 0).all()
    blob = reference(oracle, "blob3")
    for (gi, bi), ans in blob.answers.items():
        assert np.array_equal(ans.crossings % 2 == 1, ans.inside[:, :, 0]), "every hit lies beyond voxel 0 (t > 0 = t_0)"
        band = bands(blob.grids[gi])[bi]
        assert (ans.distance[ans.by_band] == band).all() and (ans.prim[ans.by_band] == DR.MISS).all() and (ans.distance[~ans.by_band] <= band).all()
    assert any(ans.far_rows.all() for ans in blob.answers.values()), "the far grid's rows are re-based"


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


def assert_grid(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        k, j, i = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {got.size} voxels differ; first (i, j, k) = ({i}, {j}, {k}): got {got[k, j, i]!r} want {want[k, j, i]!r}")


def assert_equals_twin(r, grid, band, ans, what):
    want_signed = DR.signed(ans.distance, ans.inside)
    for method in METHODS:
        d, p = r.distance_grid(band=band, signed=True, method=method, want_prim=True, **grid.kwargs())
        assert_grid(d, want_signed, f"{what} signed method {method}")
        assert_grid(p, ans.prim, f"{what} prim method {method}")
        d = r.distance_grid(band=band, signed=False, method=method, **grid.kwargs())
        assert_grid(d, ans.distance, f"{what} unsigned method {method}")


@gpu
@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("name", list(SCENES))
def test_grids_equal_the_twin(halart, oracle, renderers, name, builder):
    """every scene x grid x band x builder x method, signed and unsigned: distance and prim equal the twin byte for byte"""
    check_conditions(oracle)
    ref = reference(oracle, name)
    r = renderers(name, builder)
    assert_form(r, SCENES[name][1])
    for (gi, bi), ans in ref.answers.items():
        grid = ref.grids[gi]
        assert_equals_twin(r, grid, bands(grid)[bi], ans, f"{name} {builder} {grid.dims} band {bi}")


@gpu
@pytest.mark.parametrize("name", ["blob3", "sheets512"])
def test_a_grid_the_twin_cannot_afford(halart, oracle, renderers, name):
    """(48, 40, 36): the unsigned grid of each method equals hala_rt_closest_points on the same points bit for bit; the two methods' signed
    grids are the same bytes; on every row with fewer than 16 hits the sign is the parity counted from hala_rt_trace_rays_multi"""
    ref = reference(oracle, name)
    r = renderers(name)
    grid = DR.grid_over(ref.mn, ref.mx, (48, 40, 36))
    nx, ny, nz = grid.dims
    pts = grid.points()
    for band in bands(grid):
        rec = r.closest_points(pts, band)
        want = np.where(rec["prim"] != CR.MISS, rec["distance"], f32(band)).astype(f32).reshape(nz, ny, nx)
        assert (rec["prim"] == CR.MISS).any() == bool(band != np.inf), "the finite band answers some voxels, the infinite one none"
        grids = []
        for method in (1, 2):
            d, p = r.distance_grid(band=band, signed=False, method=method, want_prim=True, **grid.kwargs())
            assert_grid(d, want, f"{name} unsigned method {method}")
            assert_grid(p, rec["prim"].reshape(nz, ny, nx), f"{name} prim method {method}")
            grids.append(r.distance_grid(band=band, signed=True, method=method, **grid.kwargs()))
        assert grids[0].tobytes() == grids[1].tobytes()
        assert (np.abs(grids[0]) == want).all()
    rays = np.zeros(ny * nz, dtype=A.RAY_DTYPE)
    rays["origin"] = pts.reshape(nz, ny, nx, 3)[:, :, 0, :].reshape(-1, 3)
    rays["direction"] = (1.0, 0.0, 0.0); rays["tmin"] = 0.0; rays["tmax"] = np.inf
    hits, counts = r.trace_rays_multi_host(rays, 16)
    t_i = (np.arange(nx).astype(f32) * grid.spacing).astype(f32)
    got_inside = np.signbit(grids[0]).reshape(ny * nz, nx)
    checked = crossed = 0
    for row in np.nonzero(counts < 16)[0]:
        m = np.searchsorted(t_i, hits["t"][row, :counts[row]], side="left")
        above = np.bincount(m, minlength=nx + 1)[::-1].cumsum()[::-1]
        assert np.array_equal(got_inside[row], above[1:] % 2 == 1), (name, row)
        checked += 1; crossed += int(counts[row] > 0)
    # the blob's rows cross it 0, 2 or 4 times; a row through the pile of sheets crosses far more than 16 of them and is not checked here
    assert checked >= 0.5 * ny * nz and (crossed >= 100 if name == "blob3" else (counts == 16).any()), (checked, crossed)


@gpu
def test_refusals_and_no_ops(halart, oracle, renderers):
    """each refusal raises, names its reason and leaves a prefilled buffer as it was"""
    import torch
    from test_gpu_parity import make_renderer
    ref = reference(oracle, "cornell")
    r = renderers("cornell")
    grid = ref.grids[1]
    n = 64
    d_out = torch.full((n * 4,), 0xAB, dtype=torch.uint8, device="cuda")
    d_prim = torch.full((n * 4,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    fresh = halart.HalaRenderer("uncommitted", 16, 16, 5, 3, False, False, False, 0)
    instanced = make_renderer(halart, two_blobs(), 16, 16, build=dict(instancing=True))
    assert instanced.bvh_info().instance_ref_count > 0
    good = desc_of(grid)

    def changed(**kw):
        d = desc_of(grid)
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    cases = [(r, None, d_out.data_ptr(), "null"), (r, good, 0, "null"),
             (fresh, good, d_out.data_ptr(), "acceleration structure"), (instanced, good, d_out.data_ptr(), "two-level"),
             (r, changed(dims=(C.c_uint32 * 3)(0, 4, 4)), d_out.data_ptr(), "dims"), (r, changed(dims=(C.c_uint32 * 3)(4, 1025, 4)), d_out.data_ptr(), "dims"),
             (r, changed(spacing=0.0), d_out.data_ptr(), "spacing"), (r, changed(spacing=-1.0), d_out.data_ptr(), "spacing"),
             (r, changed(spacing=float("inf")), d_out.data_ptr(), "spacing"), (r, changed(spacing=float("nan")), d_out.data_ptr(), "spacing"),
             (r, changed(band=float("nan")), d_out.data_ptr(), "band"), (r, changed(band=-1.0), d_out.data_ptr(), "band"),
             (r, changed(flags=8), d_out.data_ptr(), "flags"), (r, changed(flags=1 | (3 << 1)), d_out.data_ptr(), "flags"),
             (r, changed(flags=0x80000001), d_out.data_ptr(), "flags")]
    for who, desc, out, match in cases:
        with pytest.raises(halart.HalaRendererError, match=match):
            who._check(who._lib.hala_rt_distance_grid(who._h, C.byref(desc) if desc is not None else None, C.c_void_p(out), C.c_void_p(d_prim.data_ptr()), None))
    with pytest.raises(halart.HalaRendererError, match="two-level"):
        instanced.distance_grid(**grid.kwargs())
    with pytest.raises(halart.HalaRendererError, match="band"):
        r.distance_grid(band=-0.5, **grid.kwargs())
    r.wait_idle(); instanced.wait_idle()
    torch.cuda.synchronize()
    assert bool((d_out == 0xAB).all()) and bool((d_prim == 0xAB).all())
    fresh.close(); instanced.close()
    # accepted: a band of 0 and of +inf, -0.0 as a band, the smallest grid
    ans = ref.answers[(2, 0)]
    assert_grid(r.distance_grid(band=np.inf, **ref.grids[2].kwargs()), DR.signed(ans.distance, ans.inside), "1 x 1 x 1")
    zero = r.distance_grid(band=0.0, signed=False, **grid.kwargs())
    assert (zero == 0.0).all()


@gpu
@pytest.mark.parametrize("name", ["cornell", "blob3"])
def test_device_form_on_two_streams(halart, oracle, renderers, name):
    """on a second stream and on the renderer's stream, with and without d_prim; the same grid twice gives the same bytes"""
    import torch
    ref = reference(oracle, name)
    r = renderers(name)
    grid, ans = ref.grids[0], ref.answers[(0, 1)]
    band = bands(grid)[1]
    n = int(np.prod(grid.dims))
    want = DR.signed(ans.distance, ans.inside)
    d_out = torch.zeros(n, dtype=torch.float32, device="cuda")
    d_prim = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for method in (1, 2):
        r.distance_grid(band=band, method=method, out=d_out, out_prim=d_prim, stream=side.cuda_stream, **grid.kwargs())
        side.synchronize()
        first = d_out.cpu().numpy().tobytes()
        assert first == want.tobytes() and d_prim.cpu().numpy().view(np.uint32).tobytes() == ans.prim.tobytes()
        d_out.zero_(); d_prim.fill_(7)
        torch.cuda.synchronize()
        r.distance_grid(band=band, method=method, out=d_out.data_ptr(), **grid.kwargs())  # raw pointer, no prim, the renderer's stream
        r.wait_idle()
        assert d_out.cpu().numpy().tobytes() == first and bool((d_prim == 7).all())


@gpu
def test_counters_and_the_automatic_method(halart, oracle, renderers):
    """hala_rt_distance_grid_counted: the same bytes, six counters that mean what the header says; an automatic grid runs the wave kernel
    (which alone fetches per wave) on a large tree with an unlimited band and fine voxels, and the lane kernel elsewhere"""
    import torch
    d_ctr = torch.zeros(6, dtype=torch.int64, device="cuda")

    def counted(name, gi, bi, method, signed=True):
        ref = reference(oracle, name)
        grid, ans = ref.grids[gi], ref.answers[(gi, bi)]
        d_out = torch.zeros(int(np.prod(grid.dims)), dtype=torch.float32, device="cuda")
        d_ctr.fill_(-1)
        torch.cuda.synchronize()
        r = renderers(name)
        r.distance_grid(band=bands(grid)[bi], signed=signed, method=method, out=d_out, d_counters=d_ctr.data_ptr(), **grid.kwargs())
        r.wait_idle()
        want = DR.signed(ans.distance, ans.inside) if signed else ans.distance
        assert d_out.cpu().numpy().tobytes() == want.tobytes()
        return [int(x) for x in d_ctr.cpu()], int(np.prod(grid.dims)), grid.dims[1] * grid.dims[2]
    c, voxels, rows = counted("blob3", 4, 0, 1)
    assert c[0] >= voxels and c[1] >= voxels and c[2] >= rows and c[3] > 0 and c[4] == 0 and c[5] == 0, c
    c, voxels, rows = counted("blob3", 4, 0, 2)
    assert c[0] >= voxels and c[1] >= voxels and c[2] >= rows and 0 < c[4] <= c[0] and 0 < c[5] <= c[1], c
    c, voxels, rows = counted("blob3", 4, 0, 2, signed=False)
    assert c[2] == 0 and c[3] == 0 and c[4] > 0, c
    assert counted("blob3", 4, 0, None)[0][4] > 0, "large tree, unlimited band, 70 voxels across the box: a brick per wave"
    assert counted("blob3", 4, 1, None)[0][4] == 0, "a band of two spacings: a voxel per lane"
    assert counted("blob3", 1, 0, None)[0][4] == 0, "4 voxels across the box: a voxel per lane"
    assert counted("cornell", 4, 0, None)[0][4] == 0, "a staged tree: a voxel per lane"


@gpu
@pytest.mark.parametrize("name", ["cornell", "blob3"])
def test_frames_around_a_grid_are_unchanged(halart, oracle, name):
    """update, grid, update: the grid shares the renderer's scratch; images 0-3 are those of a run without the grid, bit for bit"""
    from test_gpu_parity import make_renderer
    ref = reference(oracle, name)
    grid, ans = ref.grids[0], ref.answers[(0, 0)]
    images = []
    for with_grid in (False, True):
        r = make_renderer(halart, ref.scene, 32, 32)
        r.update(); r.render()
        if with_grid:
            for method in (1, 2):
                assert_grid(r.distance_grid(method=method, **grid.kwargs()), DR.signed(ans.distance, ans.inside), f"between frames, {name}")
        r.update(); r.render()
        images.append([r.read_image(which).tobytes() for which in range(4)])
        r.close()
    assert images[0] == images[1]


def assert_edited(r, what):
    """the twin on the triangles and the box the renderer holds after a refit"""
    tris = CR.bvh_triangles(r.download_bvh()[1])
    i = r.bvh_info()
    mn, mx = np.array(list(i.scene_min), np.float64), np.array(list(i.scene_max), np.float64)
    twin = DR.Twin(*tris, mn, mx)
    for grid in (DR.grid_over(mn, mx, (13, 10, 7)), DR.far_grid(mn, mx)):
        for band in bands(grid):
            ans = twin.answer(grid, band)
            if grid.dims == (13, 10, 7):
                assert ans.inside.sum() >= 20 and (~ans.by_band).sum() >= 100
            assert_equals_twin(r, grid, band, ans, f"{what} {grid.dims}")
    return tris


@gpu
def test_after_a_node_refit(halart, oracle):
    """update_node_transform + refit on the flattened two_blobs: the grid is the twin's on the edited triangles"""
    from test_gpu_parity import make_renderer
    r = make_renderer(halart, two_blobs(), 16, 16, build=dict(instancing=False))
    assert r.bvh_info().instance_ref_count == 0
    before = CR.bvh_triangles(r.download_bvh()[1])
    m = np.eye(4, dtype=f32); m[:3, :3] *= f32(0.75); m[:3, 3] = (1.5, 0.25, -0.5)  # into the other blob
    r.update_node_transform(0, m)
    r.refit()
    assert not np.array_equal(assert_edited(r, "node refit")[0], before[0])
    r.close()


@gpu
def test_after_a_deformer_refit(halart, oracle):
    """a posed morph target + refit on the blob: the grid is the twin's on the posed triangles"""
    from test_gpu_parity import make_renderer
    s = RC.blob_scene(3)
    r = make_renderer(halart, s, 16, 16)
    before = CR.bvh_triangles(r.download_bvh()[1])
    pos = np.asarray(s.meshes[0].primitives[0].vertices["position"], dtype=f32)
    delta = (pos * (0.3 * np.sin(5.0 * pos[:, 1:2]))).astype(f32)
    r.set_deformer(0, 0, targets=delta[None])
    r.update_deformer(0, 0, morph_weights=[0.7])
    r.refit()
    assert not np.array_equal(assert_edited(r, "deformer refit")[0], before[0])
    r.close()
