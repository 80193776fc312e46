"""The float32 numpy twin of occlusion batches (docs/RENDER_SPEC.md 4.10), operation for operation.

    rays, valid = expand(samples, N, seed)              # the count * N rays of the batch as A.RAY_DTYPE, entry i * N + j = ray j of sample i
    rec, masks = reduce(samples, N, seed, occluded)     # the 16-B records and the mask words from the rays' occlusion bits [count, N]
    o, d, valid = expand64(samples, N, seed)            # the same rays in float64 with libm sin / cos

The occlusion bits are not made here: they are what a mode-1 (any-hit) trace answers for the expanded batch — the oracle's brute force
(OracleScene.trace(rays, mode=1, brute=True)) on the CPU tier, the renderer's own hala_rt_trace_rays on the GPU tier.  pcg is
first_hit_ref's, fma and dot are aov_ref's (RENDER_SPEC 2.1), sincos_2pi is the oracle's (RENDER_SPEC 2.2); the basis and to_world of
RENDER_SPEC 2.4 are written here in the operation order of csrc/rt_math.h.  An invalid sample's rays are (0, 0, (0, 0, 1), -1): a limit
that admits nothing, so the expanded batch can be traced as it is."""
import numpy as np

import oracle_lib as O
from aov_ref import dot, fma
from first_hit_ref import pcg
from hala_renderer_amd import _abi as A

f32, f64 = np.float32, np.float64
M32 = np.uint64(0xFFFFFFFF)
INVALID = (-1.0, (0.0, 0.0, 0.0))
GOLDEN, SEED_ADD = 0x9E3779B9, 0x85EBCA6B


def words(n_rays):
    return (n_rays + 31) // 32


def valid_flags(samples):
    """(valid, nn): nn = dot(normal, normal); valid iff nn > 0, nn < +inf, point and bias finite"""
    nrm = samples["normal"].astype(f32)
    finite = np.isfinite(nrm).all(axis=1)
    with np.errstate(all="ignore"):
        nn = dot(np.where(finite[:, None], nrm, f32(0.0)), np.where(finite[:, None], nrm, f32(0.0))).astype(f32)
    nn = np.where(finite, nn, f32(np.nan)).astype(f32)  # an infinite component squares to +inf, a NaN stays one: both fail
    with np.errstate(invalid="ignore"):
        ok = (nn > 0) & (nn < np.inf) & np.isfinite(samples["point"]).all(axis=1) & np.isfinite(samples["bias"])
    return ok, nn


def seed_key(seed):
    return pcg((np.uint64(seed & 0xFFFFFFFF) * np.uint64(GOLDEN) + np.uint64(SEED_ADD)) & M32)


def streams(first, count, seed):
    """RENDER_SPEC 2.3 with pixel_id = the global sample index and frame_index = seed"""
    i = np.arange(first, first + count, dtype=np.uint64)
    return pcg((i + seed_key(seed)) & M32)


def uniforms(s, n_rays):
    """(u1, u2) [count, N]: draws 2j and 2j + 1 of each stream by random access (uint32 arithmetic, wrapping); exact in float32"""
    j = np.arange(n_rays, dtype=np.uint64)[None, :]
    x1 = pcg((s[:, None] + np.uint64(2) * j) & M32)
    x2 = pcg((s[:, None] + np.uint64(2) * j + np.uint64(1)) & M32)
    to_unit = lambda x: ((x >> np.uint64(8)).astype(f64) * 2.0 ** -24).astype(f32)  # noqa: E731
    return to_unit(x1), to_unit(x2)


def basis(n):
    """RENDER_SPEC 2.4 (Duff et al.), in the operation order of rt_math.h's onb: no fma"""
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    sign = np.copysign(f32(1.0), nz).astype(f32)
    a = (f32(-1.0) / (sign + nz)).astype(f32)
    bb = ((nx * ny) * a).astype(f32)
    t = np.stack([f32(1.0) + ((sign * nx) * nx) * a, sign * bb, (-sign) * nx], axis=1).astype(f32)
    b = np.stack([bb, sign + (ny * ny) * a, -ny], axis=1).astype(f32)
    return t, b


def frames(samples, nn):
    """(n, t, b, o) of the samples (rows of invalid samples hold anything)"""
    with np.errstate(all="ignore"):
        inv = (f32(1.0) / np.sqrt(nn.astype(f32))).astype(f32)
        n = (samples["normal"].astype(f32) * inv[:, None]).astype(f32)
        t, b = basis(n)
        o = fma(n, samples["bias"].astype(f32)[:, None], samples["point"].astype(f32))
    return n, t, b, o


def directions(n, t, b, u1, u2):
    """to_world(cosine_hemisphere(u1, u2), t, b, n) [count, N, 3], not normalised again"""
    count, n_rays = u1.shape
    r = np.sqrt(u1).astype(f32)
    sn, cs = O.probe_sincos_2pi(np.ascontiguousarray(u2).reshape(-1))
    lx, ly = (r * cs.reshape(u1.shape)).astype(f32), (r * sn.reshape(u1.shape)).astype(f32)
    lz = np.sqrt(np.maximum(f32(0.0), f32(1.0) - u1)).astype(f32)
    with np.errstate(all="ignore"):
        d = [fma(n[:, None, c], lz, fma(b[:, None, c], ly, t[:, None, c] * lx)) for c in range(3)]
    return np.stack(d, axis=2).astype(f32)


def expand(samples, n_rays, seed, first=0):
    """the batch's rays and the samples' valid flags; `first`: the global index of samples[0] (a batch starts at 0)"""
    samples = np.ascontiguousarray(samples, dtype=A.OCCLUSION_SAMPLE_DTYPE)
    count = len(samples)
    ok, nn = valid_flags(samples)
    n, t, b, o = frames(samples, nn)
    u1, u2 = uniforms(streams(first, count, seed), n_rays)
    d = directions(n, t, b, u1, u2)
    rays = np.zeros((count, n_rays), dtype=A.RAY_DTYPE)
    rays["origin"] = np.where(ok[:, None, None], o[:, None, :], f32(0.0))
    rays["direction"] = np.where(ok[:, None, None], d, np.array([0.0, 0.0, 1.0], f32))
    rays["tmax"] = np.where(ok, samples["reach"], f32(-1.0))[:, None]
    return rays.reshape(-1), ok


def reduce(samples, n_rays, seed, occluded, first=0):
    """records (A.OCCLUSION_DTYPE) and masks [count, W] from the occlusion bits [count, N] of the expanded batch"""
    samples = np.ascontiguousarray(samples, dtype=A.OCCLUSION_SAMPLE_DTYPE)
    count = len(samples)
    rays, ok = expand(samples, n_rays, seed, first)
    d = rays["direction"].reshape(count, n_rays, 3)
    occ = np.asarray(occluded, dtype=bool).reshape(count, n_rays) & ok[:, None]
    masks = np.zeros((count, words(n_rays)), dtype=np.uint32)
    for j in range(n_rays):
        masks[:, j >> 5] |= occ[:, j].astype(np.uint32) << np.uint32(j & 31)
    clear = ~occ
    total = np.zeros((count, 3), f32)
    for j in range(n_rays):  # S = S + d_j for the unoccluded j in ascending order
        total = np.where(clear[:, j, None], (total + d[:, j]).astype(f32), total)
    ss = dot(total, total).astype(f32)
    with np.errstate(all="ignore"):
        bent = np.where((ss > 0)[:, None], total * (f32(1.0) / np.sqrt(ss))[:, None], f32(0.0)).astype(f32)
    rec = np.zeros(count, dtype=A.OCCLUSION_DTYPE)
    rec["visibility"] = np.where(ok, clear.sum(axis=1).astype(f32) / f32(n_rays), f32(-1.0))
    rec["bent"] = np.where(ok[:, None], bent, f32(0.0))
    return rec, masks


def bits_of(masks, n_rays):
    """[count, N] bool from mask words"""
    j = np.arange(n_rays)
    return ((np.asarray(masks, dtype=np.uint32)[:, j >> 5] >> (j & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)


def expand64(samples, n_rays, seed, first=0):
    """(o [count, 3], d [count, N, 3], valid) in float64 from the float32 samples: the same uniforms (they are exact), libm sin / cos"""
    samples = np.ascontiguousarray(samples, dtype=A.OCCLUSION_SAMPLE_DTYPE)
    ok, _ = valid_flags(samples)
    with np.errstate(all="ignore"):
        nrm = samples["normal"].astype(f64)
        n = nrm / np.sqrt((nrm * nrm).sum(axis=1))[:, None]
        sign = np.copysign(1.0, n[:, 2])
        a = -1.0 / (sign + n[:, 2])
        bb = n[:, 0] * n[:, 1] * a
        t = np.stack([1.0 + sign * n[:, 0] * n[:, 0] * a, sign * bb, -sign * n[:, 0]], axis=1)
        b = np.stack([bb, sign + n[:, 1] * n[:, 1] * a, -n[:, 1]], axis=1)
        o = samples["point"].astype(f64) + n * samples["bias"].astype(f64)[:, None]
    u1, u2 = (u.astype(f64) for u in uniforms(streams(first, len(samples), seed), n_rays))
    r, phi = np.sqrt(u1), 2.0 * np.pi * u2
    lx, ly, lz = r * np.cos(phi), r * np.sin(phi), np.sqrt(np.maximum(0.0, 1.0 - u1))
    with np.errstate(all="ignore"):
        d = t[:, None, :] * lx[..., None] + b[:, None, :] * ly[..., None] + n[:, None, :] * lz[..., None]
    return o, d, ok


def pcg_inverse(x):
    """v with pcg(v) == x (pcg is a bijection of uint32): python ints"""
    x = int(x) & 0xFFFFFFFF
    w = x ^ (x >> 22)
    w = (w * pow(277803737, -1, 1 << 32)) & 0xFFFFFFFF
    shift = (w >> 28) + 4  # the top four bits pass through the xorshift
    s = w
    for _ in range(8):
        s = w ^ (s >> shift)
    return ((s - 2891336453) * pow(747796405, -1, 1 << 32)) & 0xFFFFFFFF


def equivalent_seed(seed, offset):
    """RENDER_SPEC 2.3: the seed under which sample i draws what sample i + offset draws under `seed`"""
    key = (int(seed_key(seed)) + offset) & 0xFFFFFFFF
    return ((pcg_inverse(key) - SEED_ADD) * pow(GOLDEN, -1, 1 << 32)) & 0xFFFFFFFF
