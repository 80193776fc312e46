"""The exact-math helpers of csrc/rt_math.h (rcp_rn, sqrt_rn): a short sequence on the hardware's approximate reciprocal and reciprocal
square root that must give the bits of 1.0f / x and sqrtf(x) for EVERY input.

- the exhaustive sweep: all 2^32 bit patterns through hala_rt_selftest_math, helper against the plain expression, 0 mismatches;
- the plain expression the sweep compares with is IEEE: its values on 2^20 seeded patterns and an edge list equal numpy's float32 1 / x and
  sqrt bit for bit (a compiler flag that made `/` approximate would make both sides of the sweep agree on a wrong value);
- the call sites: rays with extreme and unnormalised directions, and rays through shared edges and vertices and along triangle planes
  (tiny determinants), through hala_rt_trace_rays on an LDS-staged tree (tri_test2) and on a large one (the cooperative leaf pass),
  against the oracle's walk over the same tree, bit for bit;
- CPU tier: the header, the export list, the Python binding and the library carry the entry point."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hala_renderer_amd as H
import ray_conditioning as RC
from hala_renderer_amd import scenes

gpu = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHICH = {"rcp": H.SELFTEST_RCP, "sqrt": H.SELFTEST_SQRT}
SWEEP_LAUNCHES = 16  # 2^28 patterns each
N_RANDOM = 1 << 20
N_RAYS = 4096


# ---- CPU tier ---------------------------------------------------------------------------------------------------------------------------
def test_header_exports_and_library_carry_the_entry_point(halart):
    header = open(os.path.join(ROOT, "include", "halart.h")).read()
    lib = C.CDLL(halart.LIB_PATH)
    for name in ("hala_rt_selftest_math", "hala_rt_selftest_math_values"):
        assert re.search(rf"\bint {name}\(", header), name
        assert name in H._abi.EXPORTS and name in H._abi.PROTOTYPES, name
        assert hasattr(lib, name), name
    assert callable(halart.selftest_math) and callable(halart.selftest_math_values)


def test_arguments_are_checked_before_any_device_work(halart):
    """an empty range is answered on the host; a bad selector and a range past 2^32 are errors"""
    assert halart.selftest_math(H.SELFTEST_RCP, 0, 0) == (0, None)
    with pytest.raises(halart.HalaRendererError, match="which"):
        halart.selftest_math(2, 0, 0)
    with pytest.raises(halart.HalaRendererError, match="2\\^32"):
        halart.selftest_math(H.SELFTEST_SQRT, 0xFFFFFFFF, 2)


# ---- the sweep --------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("which", sorted(WHICH))
def test_exhaustive_sweep(halart, which):
    """every one of the 2^32 bit patterns, in SWEEP_LAUNCHES launches"""
    per = (1 << 32) // SWEEP_LAUNCHES
    total = 0
    for k in range(SWEEP_LAUNCHES):
        bad, first_bad = halart.selftest_math(WHICH[which], k * per, per)
        print(f"{which} [{k * per:#010x}, {k * per + per - 1:#010x}]: {bad} mismatches" + (f", lowest {first_bad:#010x}" if bad else ""))
        assert (bad, first_bad) == (0, None), f"{which}: {bad} patterns of launch {k} differ from the IEEE expression, the lowest is {first_bad:#010x}"
        total += per
    assert total == 1 << 32


def edge_patterns():
    e = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF,  # +-0, smallest and largest denormal
         0x00800000, 0x80800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001,  # FLT_MIN, FLT_MAX, inf, NaNs
         0x3F800001, 0x3F7FFFFF, 0xBF800001, 0xBF7FFFFF]  # 1 +- 1 ulp
    for k in range(-126, 127):  # 2^k, and 2^k with an all-ones mantissa, both signs
        b = (k + 127) << 23
        e += [b, b | 0x007FFFFF, b | 0x80000000, b | 0x807FFFFF]
    return np.array(e, dtype=np.uint32)


def same_bits_or_both_nan(a_bits, b_bits):
    a, b = a_bits.view(f32), b_bits.view(f32)
    return (a_bits == b_bits) | (np.isnan(a) & np.isnan(b))


@gpu
@pytest.mark.parametrize("which", sorted(WHICH))
def test_the_reference_expression_is_ieee(halart, which):
    patterns = np.concatenate([np.random.RandomState(20260 + WHICH[which]).randint(0, 1 << 32, N_RANDOM, dtype=np.uint64).astype(np.uint32), edge_patterns()])
    helper, ref, bad = halart.selftest_math_values(WHICH[which], patterns)
    x = patterns.view(f32)
    with np.errstate(all="ignore"):
        want = (f32(1.0) / x if which == "rcp" else np.sqrt(x)).astype(f32)
    assert want.dtype == f32
    # numpy must not be flushing denormals, or it is no reference: the smallest denormal, 2^-149, has the root 2^-74.5; 2^-127 the reciprocal 2^127
    probe = np.array([0x00000001, 0x00400000], dtype=np.uint32).view(f32)
    with np.errstate(all="ignore"):
        assert np.sqrt(probe).view(np.uint32)[0] == 0x1A3504F3 and (f32(1.0) / probe).view(np.uint32)[1] == 0x7F000000
    ok = same_bits_or_both_nan(ref, want.view(np.uint32))
    k = np.nonzero(~ok)[0]
    assert ok.all(), f"{which}: the kernel's plain expression differs from numpy on {len(k)} patterns, first {patterns[k[:4]]} -> {ref[k[:4]]} want {want.view(np.uint32)[k[:4]]}"
    ok = same_bits_or_both_nan(helper, ref)
    assert ok.all() and bad == 0, f"{which}: the helper differs from the plain expression on {int((~ok).sum())} patterns ({bad} counted)"
    # the edge list reaches both paths of the helper
    assert np.isnan(want).any() and np.isinf(want).any() and (want == 0).any() and np.isfinite(want).sum() > N_RANDOM // 4


# ---- the call sites -----------------------------------------------------------------------------------------------------------------------
def _rays(o, d, tmax):
    rays = np.zeros(len(o), dtype=H._abi.RAY_DTYPE)
    rays["origin"] = np.asarray(o, dtype=f32)
    rays["direction"] = np.asarray(d, dtype=f32)  # as given: not normalised
    rays["tmin"] = 0.0
    rays["tmax"] = np.asarray(tmax, dtype=f32)
    return rays


def call_site_rays(osc, seed):
    """N_RAYS rays in four families of N_RAYS / 4: random directions of any length; direction components from the list of extremes; rays
    aimed (in float32) at vertices and at points of edges; rays that start in a triangle's plane and run inside it"""
    rng = np.random.RandomState(seed)
    n = N_RAYS // 4
    mn, mx = [v.astype(np.float64) for v in osc.bounds()]
    size = mx - mn
    tri = osc.triangles().astype(np.float64).reshape(-1, 3, 3)

    def origins(k):
        return ((mn - 0.25 * size) + rng.rand(k, 3) * 1.5 * size).astype(f32)

    fams = []
    d = rng.randn(n, 3) * 10.0 ** rng.uniform(-3, 3, (n, 1))
    fams.append((origins(n), d))
    extremes = np.array([0.0, 1e-21, -1e-21, 1e-19, -1e-19, 1e30, -1e30, 1.0, -1.0], dtype=np.float64)
    d = np.where(rng.rand(n, 3) < 0.6, extremes[rng.randint(0, len(extremes), (n, 3))], rng.randn(n, 3))
    fams.append((origins(n), d))
    t = tri[rng.randint(0, len(tri), n)]
    a = rng.randint(0, 3, n)
    va, vb = t[np.arange(n), a], t[np.arange(n), (a + 1) % 3]
    s = np.where(rng.rand(n) < 0.4, 0.0, rng.rand(n))[:, None]  # s = 0: the vertex itself
    target = (va + s * (vb - va)).astype(f32)
    o = origins(n)
    fams.append((o, (target - o) * f32(10.0) ** rng.randint(-2, 3, (n, 1)).astype(f32)))  # float32 differences, scaled by exact or near-exact factors
    t = tri[rng.randint(0, len(tri), n)]
    e1, e2 = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    w = rng.uniform(-1.0, 2.0, (n, 2))
    o = (t[:, 0] + w[:, :1] * e1 + w[:, 1:] * e2).astype(f32)
    c = rng.uniform(-1.0, 1.0, (n, 2))
    fams.append((o, (c[:, :1] * e1 + c[:, 1:] * e2).astype(f32)))
    o = np.concatenate([f[0] for f in fams]); d = np.concatenate([f[1] for f in fams])
    tmax = np.where(rng.rand(N_RAYS) < 0.3, rng.rand(N_RAYS) * 2.0 * np.linalg.norm(size), 3.0e38)
    rays = _rays(o, d, tmax)
    comp = rays["direction"].ravel()
    for v in (0.0, 1e-21, -1e-19, 1e30, -1e30):
        assert (comp == f32(v)).any()
    norms = np.linalg.norm(rays["direction"].astype(np.float64), axis=1)
    assert (norms < 0.5).any() and (norms > 2.0).any()
    return rays


_SCENES = {"cornell": scenes.cornell_box, "blob": lambda: RC.blob_scene(3)}
_REF = {}


def reference(oracle, name):
    if name not in _REF:
        s = _SCENES[name]()
        osc = oracle.OracleScene(s)
        _REF[name] = (s, osc, call_site_rays(osc, 7 + len(name)))
    return _REF[name]


@gpu
@pytest.mark.parametrize("name", sorted(_SCENES))
def test_call_sites_match_the_oracle(halart, oracle, name):
    """cornell: the LDS-staged kernels and tri_test2; blob_scene(3), 1280 triangles: the large-tree kernels and the cooperative leaf pass.
    Closest hits equal the oracle's walk over the renderer's tree in every bit of (t, u, v, prim), any hits in t."""
    import torch
    from test_gpu_parity import make_renderer
    s, osc, rays = reference(oracle, name)
    r = make_renderer(halart, s, 16, 16)
    info = r.bvh_info()
    assert (info.lds_node_count > 0) == (name == "cornell") and (name == "cornell" or info.triangle_count == 1280)
    nodes, tris = r.download_bvh()
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    d_hits = torch.zeros(len(rays) * 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    staged = int(name == "cornell")
    for mode in (0, 1):
        d_hits.zero_()
        torch.cuda.synchronize()
        r.trace_rays(d_rays.data_ptr(), d_hits.data_ptr(), len(rays), mode)
        r.wait_idle()
        got = np.frombuffer(d_hits.cpu().numpy().tobytes(), dtype=H._abi.HIT_DTYPE)
        want, _ = oracle.trace_on_bvh(nodes, tris, rays, mode, None, bounds=osc.bounds())
        launched = halart.variant_ledger(1)[0]
        assert launched >> (mode + 8 * staged) & 1, f"k_trace_batch<ANY={mode}, STAGED={staged}> was not launched"
        fields = ("t", "u", "v", "prim") if mode == 0 else ("t",)
        for f in fields:
            g, w = got[f].view(np.uint32), want[f].view(np.uint32)
            k = np.nonzero(g != w)[0]
            assert len(k) == 0, f"{name}, mode {mode}: {len(k)} rays differ in {f}, first ray {rays[k[:1]]} got {got[k[:1]]} want {want[k[:1]]}"
        if mode == 0:
            hit = got["prim"] != RC.MISS
            per = N_RAYS // 4
            print(f"{name}: hits per family {[int(hit[i * per:(i + 1) * per].sum()) for i in range(4)]}")
            assert hit[:per].mean() > 0.2 and hit[2 * per:3 * per].any() and not hit[2 * per:3 * per].all()
    r.close()
