"""numpy float32 twin of docs/RENDER_SPEC.md 11 (adaptive sampling; hala-renderer_amd/csrc/adaptive.hip).

Given the running means a renderer without adaptive sampling would hold after every frame, it replays the schedule (snapshot, checks)
and predicts which 8 x 8 block stops when.  Every constant is np.float32 and every operation is one IEEE binary32 operation in the
order the spec writes it, so the GPU's decisions are reproduced exactly.
"""
import numpy as np

f32 = np.float32
BLOCK = 8
EPS = f32(1e-4)


def is_check(n, min_samples, interval):
    return n >= min_samples and (n - min_samples) % interval == 0


def check_k(s, n):
    """k = sqrtf((float)s / (float)(n - s)), computed once per check on the host"""
    return f32(np.sqrt(f32(s) / f32(n - s)))


def pixel_errors(accum, snap, k, exposure=1.0):
    """e per pixel: [H, W] float32 (NaN where the image is not finite)"""
    E = f32(exposure)
    a = np.asarray(accum, f32)
    p = np.asarray(snap, f32)
    with np.errstate(all="ignore"):
        ix, iy, iz = a[..., 0] * E, a[..., 1] * E, a[..., 2] * E
        px, py, pz = p[..., 0] * E, p[..., 1] * E, p[..., 2] * E
        d = (np.abs(ix - px) + np.abs(iy - py)) + np.abs(iz - pz)
        l = (ix + iy) + iz
        return ((d * f32(k)) / (EPS + np.sqrt(np.where(l > 0, l, f32(0)).astype(f32)))).astype(f32)


def _blocks(x, fill):
    """[H, W] -> [BH, BW, 64]: the pixels of each block, the out-of-frame ones of border blocks set to `fill`"""
    h, w = x.shape
    bh, bw = -(-h // BLOCK), -(-w // BLOCK)
    pad = np.full((bh * BLOCK, bw * BLOCK), fill, dtype=x.dtype)
    pad[:h, :w] = x
    return pad.reshape(bh, BLOCK, bw, BLOCK).transpose(0, 2, 1, 3).reshape(bh, bw, BLOCK * BLOCK)


def block_passes(e, threshold):
    """[BH, BW] bool: every in-frame pixel has e < threshold (NaN fails; out-of-frame pixels do not vote)"""
    with np.errstate(invalid="ignore"):
        ok = e < f32(threshold)
    return _blocks(ok, True).all(axis=-1)


def block_max_errors(e):
    """[BH, BW]: the largest in-frame error of each block (NaN counts as +inf): the block passes iff this is < threshold"""
    e = np.where(np.isnan(e), f32(np.inf), e).astype(f32)
    return _blocks(e, f32(-np.inf)).max(axis=-1)


def expand(blocks, h, w):
    return np.repeat(np.repeat(blocks, BLOCK, axis=0), BLOCK, axis=1)[:h, :w]


def simulate(accums, threshold, min_samples, interval, exposure=1.0):
    """accums[n - 1]: the running mean (RGBA32F [H, W, 4]) after n frames, n = 1 ... N.  Returns (counts [H, W] uint32: the samples folded
    into each pixel after N frames, block_counts [BH, BW]: c_b, 0 for blocks still active, s: the last snapshot)."""
    h, w = accums[0].shape[:2]
    bh, bw = -(-h // BLOCK), -(-w // BLOCK)
    cb = np.zeros((bh, bw), np.uint32)
    snap, s = None, 0
    for n in range(1, len(accums) + 1):
        a = np.asarray(accums[n - 1], f32)
        if not (cb == 0).any():
            break
        if n == min_samples // 2:
            snap, s = a.copy(), n
        if is_check(n, min_samples, interval):
            e = pixel_errors(a, snap, check_k(s, n), exposure)
            cb[block_passes(e, threshold) & (cb == 0)] = n
            still = expand(cb == 0, h, w)
            snap[still] = a[still]
            s = n
    counts = expand(cb, h, w).astype(np.uint32)
    counts[counts == 0] = len(accums)
    return counts, cb, s


def pick_threshold(accums, min_samples, interval, exposure=1.0):
    """a threshold under which some blocks converge at the first check, some at a later one and some never (asserted)"""
    n0, s0 = min_samples, min_samples // 2
    bm = block_max_errors(pixel_errors(accums[n0 - 1], accums[s0 - 1], check_k(s0, n0), exposure))
    finite = np.sort(bm[np.isfinite(bm) & (bm > 0)])
    assert finite.size >= 3, "too few blocks with a finite error to split"
    for q in (0.3, 0.2, 0.4, 0.15, 0.5, 0.1, 0.6, 0.05, 0.7):
        thr = f32(finite[int(q * (finite.size - 1))])
        counts, cb, _ = simulate(accums, thr, min_samples, interval, exposure)
        first, later, never = (cb == n0).sum(), ((cb > n0)).sum(), (cb == 0).sum()
        if first and later and never:
            return thr
    raise AssertionError("no threshold gives blocks that converge at the first check, at a later one and never")
