"""Multi-hit ray batches (docs/RENDER_SPEC.md 4.7): hala_rt_trace_rays_multi / hala_rtprog_trace_rays_multi against the numpy twin of
tests/multihit_ref.py, byte for byte.

CPU tier: the twin is tied to the oracle (k = 1 equals the oracle's brute force bit for bit on every scene and ray set used below; on
rays without a tie and without a far origin its first 8 entries equal an 8-step peel through the oracle), and the ABI surface is there.
GPU tier: the three tree forms (LDS-staged, large one-level, two-level) at the capacities of the issue's table, every builder, the
limits, the refusals, the device-pointer and program forms, the neighbours (frames before and after a batch), refit, determinism.

A comparison of empty lists proves nothing: before a GPU result is looked at, the twin's own output must show — over the cases of each
tree form together — at least 100 truncated lists, 100 partly filled ones, 50 misses, 20 rays with a tie and 10 rays whose tie straddles
position k.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hala_renderer_amd as H
import multihit_ref as MR
import ray_conditioning as RC
from hala_renderer_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = H._abi
f32 = np.float32
FUNCTIONS = ("hala_rt_trace_rays_multi", "hala_rt_trace_rays_multi_host", "hala_rtprog_trace_rays_multi")
BUILDERS = ("sah", "ploc", "lbvh")  # hala_rt_build_options::builder = 1, 2, 3


# ---- scenes and ray sets -------------------------------------------------------------------------------------------------------------
def duplicated(scene):
    """every mesh node a second time, in place (the scene is changed): every hit becomes a pair of hits at the same t under two ids"""
    s = scene
    nodes = []
    for nd in s.nodes:
        nodes.append(nd)
        if nd.mesh_index != A.INVALID_INDEX:
            nodes.append(H.HalaNode(name=nd.name + "_again", parent=nd.parent, local_transform=np.array(nd.local_transform, dtype=f32), mesh_index=nd.mesh_index))
    assert all(nd.parent is None for nd in s.nodes)
    s.nodes = nodes
    return s


def two_blobs():
    s = RC.blob_scene(3)
    m = np.eye(4, dtype=f32); m[:3, 3] = (3.0, 0.5, -1.0)
    s.nodes.insert(1, H.HalaNode(name="blob_b", mesh_index=0, local_transform=m))
    return s


SCENES = {
    "cornell": scenes.cornell_box,
    "cornell_dup": lambda: duplicated(scenes.cornell_box()),
    "sheets64": lambda: scenes.stacked_sheets(64),
    "blob": lambda: RC.blob_scene(3),
    "blob_dup": lambda: duplicated(RC.blob_scene(3)),
    "sheets512": lambda: scenes.stacked_sheets(512),
    "two_blobs": two_blobs,
    "sheets4096": lambda: scenes.stacked_sheets(4096),               # a stack deeper than the large form's LDS entries
    "sheets512_dup": lambda: duplicated(scenes.stacked_sheets(512)),  # ... and, two-level, deeper with a world-space ray parked on it
}


def probe_rays(osc, n=250):
    """24 x 17 camera rays and n rays of each probe kind of tests/ray_conditioning.py"""
    mn, mx = osc.bounds()
    return np.concatenate([osc.camera_rays(24, 17), RC.near_rays(mn, mx, n, 11), RC.far_rays(mn, mx, 0.5, n, 12), RC.lattice_rays(osc.triangles(), n, 13),
                           RC.near_axis_rays(mn, mx, n, 14)])


def far_rays(decades, n):
    def make(osc):
        mn, mx = osc.bounds()
        return np.concatenate([RC.far_rays(mn, mx, d, n, 20 + int(d)) for d in decades])
    return make


RAYS = {
    "probe": probe_rays,
    "far_2_4": far_rays((2, 4), 300),   # every ray re-based
    "probe_far_3": lambda osc: np.concatenate([probe_rays(osc, 150), far_rays((3,), 150)(osc)]),
    "probe_600": lambda osc: probe_rays(osc)[:600],
}

# (scene, instancing, ray set) -> capacities, per tree form: the table of the issue
CASES = {
    "staged": [("cornell", False, "probe", (1, 2, 3, 5, 16)), ("cornell_dup", False, "probe", (1, 2, 3, 5, 16)), ("sheets64", False, "far_2_4", (8, 16))],
    "large": [("blob", False, "probe", (1, 3, 4)), ("blob_dup", False, "probe", (1, 3, 4)), ("sheets512", False, "probe", (1, 8, 16)),
              ("sheets4096", False, "probe_600", (16,))],
    "two_level": [("two_blobs", True, "probe_far_3", (1, 2, 3, 4)), ("blob_dup", True, "probe_far_3", (1, 2, 3, 4)),
                  ("sheets512_dup", True, "probe_600", (16,))],
}
BUILDER_K = {"blob": 3, "blob_dup": 3, "sheets512": 8, "two_blobs": 2, "sheets4096": 16, "sheets512_dup": 16}  # the one capacity each large / two-level case runs at with every builder

_REF = {}


def reference(oracle, scene, instancing, rays_key):
    """(scene, oracle scene, rays, the twin's sorted lists): computed once, shared by every test and left unchanged"""
    key = (scene, instancing, rays_key)
    if key not in _REF:
        s = SCENES[scene]()
        oracle.set_instancing(instancing)
        try:
            osc = oracle.OracleScene(s)
        finally:
            oracle.set_instancing(False)
        rays = RAYS[rays_key](osc)
        _REF[key] = (s, osc, rays, MR.Twin(s, osc, instancing).lists(rays))
    return _REF[key]


_CONDITIONS = {}


def check_conditions(oracle, form):
    """what the twin's output must show over the cases of one tree form before a GPU result counts"""
    if form not in _CONDITIONS:
        truncated = partial = misses = ties = straddle = 0
        for scene, instancing, rays_key, ks in CASES[form]:
            full = reference(oracle, scene, instancing, rays_key)[3]
            misses += int((full.total == 0).sum())
            ties += int(full.tie.sum())
            for k in ks:
                truncated += int((full.total > k).sum())
                partial += int(((full.total > 0) & (full.total < k)).sum())
                straddle += int(MR.straddles(full, k).sum())
        _CONDITIONS[form] = dict(truncated=truncated, partial=partial, misses=misses, ties=ties, straddle=straddle)
    c = _CONDITIONS[form]
    assert c["truncated"] >= 100 and c["partial"] >= 100 and c["misses"] >= 50 and c["ties"] >= 20 and c["straddle"] >= 10, (form, c)
    return c


# ---- CPU tier ------------------------------------------------------------------------------------------------------------------------
def test_abi_surface(halart):
    """the header, the export list, the Rust declarations and the library name the three functions and the constant"""
    header = open(os.path.join(ROOT, "include", "halart.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    rust = open(os.path.join(ROOT, "rust", "hala-renderer-halart", "src", "lib.rs")).read()
    lib = C.CDLL(halart.LIB_PATH)
    for fn in FUNCTIONS:
        assert re.search(rf"\bint {fn}\s*\(", code), fn
        assert fn in A.EXPORTS and fn in A.PROTOTYPES, fn
        assert f"fn {fn}(" in rust, fn
        assert hasattr(lib, fn), fn
    assert re.search(r"#define HALA_MAX_MULTI_HITS 16\b", code) and A.MAX_MULTI_HITS == 16
    assert re.search(r"pub const HALA_MAX_MULTI_HITS: u32 = 16;", rust)
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*#define HALA_MAX_MULTI_HITS", header, flags=re.S)
    assert m and "RENDER_SPEC 4.7" in m.group(1), "cites its section of the spec"
    assert callable(halart.HalaRenderer.trace_rays_multi) and callable(halart.HalaRenderer.trace_rays_multi_host)
    assert callable(halart.HalaRayTracingProgram.trace_rays_multi)
    assert "### 4.7 Multi-hit rays" in open(os.path.join(ROOT, "docs", "RENDER_SPEC.md")).read()


ALL_REFERENCES = sorted({(scene, instancing, rays_key) for cases in CASES.values() for scene, instancing, rays_key, _ in cases})


@pytest.mark.parametrize("scene,instancing,rays_key", ALL_REFERENCES, ids=lambda v: str(v))
def test_twin_equals_the_oracle(oracle, scene, instancing, rays_key):
    """k = 1 is the oracle's brute force, bit for bit (far sets included, instancing as the case has it); without ties and far origins
    the first 8 entries are what 8 closest-hit batches through the oracle peel off"""
    s, osc, rays, full = reference(oracle, scene, instancing, rays_key)
    rec, counts = MR.cut(full, 1)
    want = osc.trace(rays, 0, brute=True)
    assert rec[:, 0].tobytes() == want.tobytes()
    assert np.array_equal(counts, (want["prim"] != MR.MISS).astype(np.uint32))
    plain = ~full.tie & ~full.far
    if rays_key == "far_2_4":  # every ray of this set is re-based: nothing to peel
        assert full.far.all()
        return
    assert plain.sum() >= 100
    rec8, counts8 = MR.cut(full, 8)
    peel = rays[plain].copy()
    alive = np.ones(len(peel), bool)
    for j in range(8):
        hit = osc.trace(peel, 0, brute=True)
        hit[~alive] = (-1.0, 0.0, 0.0, MR.MISS)
        assert hit.tobytes() == rec8[plain][:, j].tobytes(), j
        alive &= hit["prim"] != MR.MISS
        peel["tmin"] = np.where(alive, hit["t"], peel["tmin"])
    assert np.array_equal(counts8[plain], np.minimum(full.total[plain], 8))


@pytest.mark.parametrize("form", list(CASES))
def test_reference_shows_truncation_padding_misses_and_ties(oracle, form):
    print(form, check_conditions(oracle, form))


def test_twin_flags_and_padding(oracle):
    """the twin's own bookkeeping on the duplicated Cornell box: pairs of equal t, a pair across position k at odd k, miss records behind the count"""
    full = reference(oracle, "cornell_dup", False, "probe")[3]
    assert (full.total % 2 == 0).all() and np.array_equal(full.tie, full.total > 0)
    assert np.array_equal(MR.straddles(full, 3), full.total > 3)
    two = MR.straddles(full, 2)  # at even k only the ties the box had before (shared edges) straddle: four entries at one t
    assert (full.t[two, 0] == full.t[two, 3]).all() and two.sum() < (full.total > 3).sum()
    rec, counts = MR.cut(full, 5)
    pad = np.arange(5)[None, :] >= counts[:, None]
    assert (rec["prim"][pad] == MR.MISS).all() and (rec["t"][pad] == -1.0).all() and (rec["u"][pad] == 0.0).all() and (rec["v"][pad] == 0.0).all()
    assert (rec["prim"][~pad] != MR.MISS).all()
    hit = ~pad
    assert (np.diff(rec["t"], axis=1)[hit[:, 1:]] >= 0.0).all()
    same_t = (rec["t"][:, 1:] == rec["t"][:, :-1]) & hit[:, 1:]
    assert (rec["prim"][:, 1:][same_t] > rec["prim"][:, :-1][same_t]).all(), "equal t: ascending triangle id"


# ---- GPU tier ------------------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def renderers(halart, oracle):
    """one committed renderer per (scene, instancing, builder), closed when the module is done"""
    from test_gpu_parity import make_renderer
    made = {}

    def get(scene, instancing, builder=None):
        key = (scene, instancing, builder)
        if key not in made:
            s = reference(oracle, scene, instancing, CASE_RAYS[(scene, instancing)])[0]
            made[key] = make_renderer(halart, s, 16, 16, build=dict(builder=builder, instancing=instancing))
        return made[key]
    yield get
    for r in made.values():
        r.close()


CASE_RAYS = {(scene, instancing): rays_key for cases in CASES.values() for scene, instancing, rays_key, _ in cases}


def assert_form(r, form):
    i = r.bvh_info()
    if form == "staged":
        assert i.lds_node_count > 0
    elif form == "large":
        assert i.lds_node_count == 0 and i.instance_ref_count == 0
    else:
        assert i.instance_ref_count > 0
    return i


def assert_spills(r, form, scene):
    """the deep-stack cases: up to three entries a level (and, two-level, the four of a parked world-space ray) outgrow the form's LDS
    entries — the proxy of test_gpu_parity.test_deep_stack_spills_to_global_scratch"""
    if scene in ("sheets4096", "sheets512_dup"):
        i = assert_form(r, form)
        macro = "RT_STACK_LDS_INST" if form == "two_level" else "RT_STACK_LDS"  # the form's LDS entries per lane, as the library is built by default
        levels = int(re.search(rf"#define {macro} (\d+)", open(os.path.join(ROOT, "hala-renderer_amd", "csrc", "traverse.h")).read()).group(1))
        assert 3 * i.max_depth + (4 if form == "two_level" else 0) > levels, (scene, i.max_depth, levels)


def assert_equals_twin(r, rays, full, k, what):
    want, want_counts = MR.cut(full, k)
    got, counts = r.trace_rays_multi_host(rays, k)
    if got.tobytes() != want.tobytes():
        bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).reshape(len(rays), -1).any(axis=1))[0]
        raise AssertionError(f"{what}: {len(bad)} of {len(rays)} lists differ; first ray {bad[0]}: got {got[bad[0]]} want {want[bad[0]]}")
    assert counts.tobytes() == want_counts.tobytes(), what


GPU_CASES = [(form, scene, instancing, rays_key, k) for form, cases in CASES.items() for scene, instancing, rays_key, ks in cases for k in ks]


@gpu
@pytest.mark.parametrize("form,scene,instancing,rays_key,k", GPU_CASES, ids=lambda v: str(v))
def test_lists_equal_the_twin(halart, oracle, renderers, form, scene, instancing, rays_key, k):
    check_conditions(oracle, form)
    _, _, rays, full = reference(oracle, scene, instancing, rays_key)
    r = renderers(scene, instancing)
    assert_form(r, form)
    assert_spills(r, form, scene)
    assert_equals_twin(r, rays, full, k, f"{form} {scene} k={k}")


BUILDER_CASES = [(form, scene, instancing, rays_key, b) for form in ("large", "two_level") for scene, instancing, rays_key, _ in CASES[form] for b in BUILDERS]


@gpu
@pytest.mark.parametrize("form,scene,instancing,rays_key,builder", BUILDER_CASES, ids=lambda v: str(v))
def test_every_builder_gives_the_same_bytes(halart, oracle, renderers, form, scene, instancing, rays_key, builder):
    check_conditions(oracle, form)
    _, _, rays, full = reference(oracle, scene, instancing, rays_key)
    r = renderers(scene, instancing, builder)
    assert_form(r, form)
    assert_equals_twin(r, rays, full, BUILDER_K[scene], f"{form} {scene} {builder}")


FORM_SCENES = [("staged", "cornell", False), ("large", "blob", False), ("two_level", "two_blobs", True)]


@gpu
@pytest.mark.parametrize("form,scene,instancing", FORM_SCENES, ids=lambda v: str(v))
def test_capacity_one_is_the_closest_hit_batch(halart, oracle, renderers, form, scene, instancing):
    _, _, rays, _ = reference(oracle, scene, instancing, CASE_RAYS[(scene, instancing)])
    r = renderers(scene, instancing)
    assert_form(r, form)
    got, counts = r.trace_rays_multi_host(rays, 1)
    closest = r.trace_rays_host(rays, 0)
    assert got[:, 0].tobytes() == closest.tobytes()
    assert np.array_equal(counts, (closest["prim"] != MR.MISS).astype(np.uint32))
    first, second = r.trace_rays_multi_host(rays, 4), r.trace_rays_multi_host(rays, 4)  # two identical calls: identical bytes
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()


def limit_reference(oracle, scene, instancing):
    """rays with tmax inside the scene, tmin > 0, negative tmin, tmax <= tmin and NaN tmax (300 of each, made from the case's camera and
    near rays and their own first hits), and the twin's lists for them; the twin's output must show that the limits bite"""
    if ("limits", scene, instancing) in _REF:
        return _REF[("limits", scene, instancing)]
    s, osc, rays, ref_full = reference(oracle, scene, instancing, CASE_RAYS[(scene, instancing)])
    mn, mx = osc.bounds()
    diag = float(np.linalg.norm(mx.astype(np.float64) - mn))
    sel = slice(0, 600, 2)  # camera rays and near rays: none of them far
    base, n = rays[sel], 300
    assert not ref_full.far[sel].any()
    rng = np.random.RandomState(5)
    first = np.where(ref_full.total[sel] > 0, ref_full.t[sel, 0], f32(0.5 * diag)).astype(np.float64)  # the first hit, or somewhere inside
    sets = []
    for kind in range(5):
        q = base.copy()
        if kind == 0:
            q["tmax"] = (first * rng.uniform(0.5, 2.0, n)).astype(f32)
        elif kind == 1:
            q["tmin"] = (first * rng.uniform(0.5, 2.0, n)).astype(f32)
        elif kind == 2:
            q["tmin"] = (-rng.rand(n) * diag).astype(f32)
        elif kind == 3:
            q["tmin"] = (first * rng.uniform(0.5, 2.0, n)).astype(f32); q["tmax"] = q["tmin"] * rng.choice([f32(1.0), f32(0.5)], n)
        else:
            q["tmax"] = np.nan
        sets.append(q)
    q = np.concatenate(sets)
    full = MR.Twin(s, osc, instancing).lists(q)
    whole = ref_full.total[sel]
    for kind in (0, 1):  # some lists survive, some are cut short
        got = full.total[kind * n:(kind + 1) * n]
        assert (got > 0).sum() >= 20 and (got < whole).sum() >= 20, (scene, kind)
    assert np.array_equal(full.total[2 * n:3 * n], whole), "a negative tmin is tmin = 0"
    assert (full.total[3 * n:] == 0).all(), "an empty or NaN range admits nothing"
    _REF[("limits", scene, instancing)] = (q, full)
    return q, full


@pytest.mark.parametrize("form,scene,instancing", FORM_SCENES, ids=lambda v: str(v))
def test_limit_rays_bite(oracle, form, scene, instancing):
    limit_reference(oracle, scene, instancing)


@gpu
@pytest.mark.parametrize("form,scene,instancing", FORM_SCENES, ids=lambda v: str(v))
def test_limits(halart, oracle, renderers, form, scene, instancing):
    """tmax inside the scene, tmin > 0, negative tmin, tmax <= tmin, NaN tmax: the twin's answer"""
    q, full = limit_reference(oracle, scene, instancing)
    assert_equals_twin(renderers(scene, instancing), q, full, 4, f"limits {form}")


@gpu
def test_null_counts_and_refusals(halart, oracle, renderers):
    """counts = NULL works; k = 0, k = 17, a null batch and an uncommitted renderer raise and leave a prefilled hit buffer as it was"""
    import torch
    _, _, rays, full = reference(oracle, "cornell", False, "probe")
    r = renderers("cornell", False)
    got, counts = r.trace_rays_multi_host(rays, 3, want_counts=False)
    assert counts is None and got.tobytes() == MR.cut(full, 3)[0].tobytes()
    n = 64
    d_rays = torch.from_numpy(rays[:n].view(np.uint8).copy()).cuda()
    d_hits = torch.full((n * 17 * 16,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    fresh = halart.HalaRenderer("uncommitted", 16, 16, 5, 3, False, False, False, 0)
    for who, args, match in ((r, (d_rays.data_ptr(), d_hits.data_ptr(), n, 0), "capacity"), (r, (d_rays.data_ptr(), d_hits.data_ptr(), n, 17), "capacity"),
                             (r, (0, d_hits.data_ptr(), n, 4), "null"), (r, (d_rays.data_ptr(), 0, n, 4), "null"),
                             (r, (d_rays.data_ptr(), d_hits.data_ptr(), 1 << 31, 4), "too large"),  # 2^33 records
                             (fresh, (d_rays.data_ptr(), d_hits.data_ptr(), n, 4), "acceleration structure")):
        with pytest.raises(halart.HalaRendererError, match=match):
            who.trace_rays_multi(*args)
    with pytest.raises(halart.HalaRendererError, match="capacity"):
        r.trace_rays_multi_host(rays[:n], 17)
    with pytest.raises(halart.HalaRendererError, match="capacity"):
        r.trace_rays_multi_host(rays[:n], 0)
    r.wait_idle()
    torch.cuda.synchronize()
    assert bool((d_hits == 0xAB).all())
    r.trace_rays_multi(d_rays.data_ptr(), d_hits.data_ptr(), 0, 4)  # count == 0: a no-op
    r.wait_idle()
    assert bool((d_hits == 0xAB).all())
    fresh.close()


@gpu
def test_device_pointer_form_on_a_second_stream_and_the_program_form(halart, oracle, renderers):
    import torch
    _, osc, _, _ = reference(oracle, "cornell", False, "probe")
    r = renderers("cornell", False)
    w, h, k = 24, 17, 5
    rays = osc.camera_rays(w, h)
    want, want_counts = r.trace_rays_multi_host(rays, k)
    assert (want_counts > 0).sum() > 100
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    d_hits = torch.zeros(len(rays) * k * 16, dtype=torch.uint8, device="cuda")
    d_counts = torch.zeros(len(rays), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    r.trace_rays_multi(d_rays.data_ptr(), d_hits.data_ptr(), len(rays), k, d_counts.data_ptr(), side.cuda_stream)
    side.synchronize()
    assert d_hits.cpu().numpy().tobytes() == want.tobytes()
    assert d_counts.cpu().numpy().astype(np.uint32).tobytes() == want_counts.tobytes()
    d_hits.zero_(); d_counts.zero_()
    torch.cuda.synchronize()
    desc = halart.HalaRayTracingProgramDesc(raygen_shader_file_paths=["builtin"], hit_shader_file_paths=[halart.HalaRayTracingHitShaderDesc("builtin")], push_constant_size=4)
    prog = halart.HalaRayTracingProgram(r, desc, "multi")
    with pytest.raises(halart.HalaRendererError, match="not bound"):
        prog.trace_rays_multi(w, h, 1, k)
    prog.bind(d_rays.data_ptr(), d_hits.data_ptr())
    prog.push_constants(0, (1).to_bytes(4, "little"))  # word 0 selects the behaviour of trace_rays only
    prog.trace_rays_multi(w, h, 1, k, d_counts.data_ptr())
    r.wait_idle()
    assert d_hits.cpu().numpy().tobytes() == want.tobytes()
    assert d_counts.cpu().numpy().astype(np.uint32).tobytes() == want_counts.tobytes()
    with pytest.raises(halart.HalaRendererError, match="capacity"):
        prog.trace_rays_multi(w, h, 1, 17)
    prog.close()


@gpu
@pytest.mark.parametrize("scene", ["cornell", "blob"])
def test_frames_around_a_batch_are_the_oracles(halart, oracle, scene):
    """update, multi-hit batch, update: the batch shares the renderer's scratch and leaves the frames alone"""
    from test_gpu_parity import assert_images_equal, make_renderer
    s, osc, rays, full = reference(oracle, scene, False, "probe")
    r = make_renderer(halart, s, 32, 32)
    r.update(); r.render()
    assert_equals_twin(r, rays, full, 4, f"between frames, {scene}")
    r.update(); r.render()
    imgs, _ = osc.render(32, 32, frames=2)
    assert_images_equal(r, imgs)
    r.close()


@gpu
@pytest.mark.parametrize("two_level", [False, True], ids=["flattened", "two_level"])
def test_after_a_refit(halart, oracle, two_level):
    """update_node_transform + refit on two_blobs: the lists are the twin's on the edited scene"""
    from test_gpu_parity import make_renderer
    s = two_blobs()
    r = make_renderer(halart, s, 16, 16, build=dict(instancing=two_level))
    assert (r.bvh_info().instance_ref_count > 0) == two_level
    m = np.eye(4, dtype=f32); m[:3, :3] *= f32(0.75); m[:3, 3] = (1.5, 0.25, -0.5)  # into the other blob
    r.update_node_transform(0, m)
    r.refit()
    s.nodes[0].local_transform = m
    oracle.set_instancing(two_level)
    try:
        osc = oracle.OracleScene(s)
    finally:
        oracle.set_instancing(False)
    rays = np.concatenate([probe_rays(osc, 100), RC.instance_aimed_rays(s, 400, 61)])  # the blobs overlap now: lists of 3 and 4 among them
    full = MR.Twin(s, osc, two_level).lists(rays)
    assert (full.total > 2).sum() >= 50
    assert_equals_twin(r, rays, full, 4, f"refit, two_level={two_level}")
    r.close()
