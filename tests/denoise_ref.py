"""numpy float32 twin of docs/RENDER_SPEC.md 10 (the a-trous denoiser of hala-renderer_amd/csrc/denoise.hip).

Vectorised over pixels, the 25 taps in spec order (dy outer, dx inner).  Every constant is np.float32 and every operation is one
IEEE binary32 operation in the order the spec writes it, so that the GPU result is reproduced bit for bit.
"""
import numpy as np

f32 = np.float32
H = [f32(1 / 16), f32(1 / 4), f32(3 / 8), f32(1 / 4), f32(1 / 16)]
MIN_ALBEDO = f32(1 / 256)
ONE, ZERO = f32(1), f32(0)


def _max(a, b):
    """`a > b ? a : b` (NaN -> b), as the kernel writes it"""
    return np.where(a > b, a, b).astype(f32)


def _lum(x, y, z):
    return (f32(0.212671) * x + f32(0.715160) * y) + f32(0.072169) * z


def _g(e):
    t = ONE / (ONE + _lum(e[..., 0], e[..., 1], e[..., 2]))
    return e * t[..., None]


def denoise(color, albedo, normal, iterations=5, sigma_color=0.5, sigma_albedo=0.1, normal_power=32, demodulate=True):
    """color / albedo / normal: [H, W, >=3] (only rgb is read).  Returns RGBA32F [H, W, 4] with alpha 1."""
    c = np.asarray(color, f32)[..., :3]
    a = np.ascontiguousarray(np.asarray(albedo, f32)[..., :3])
    n = np.asarray(normal, f32)[..., :3]
    h, w = c.shape[:2]
    with np.errstate(all="ignore"):
        l2 = (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]
        pos = l2 > ZERO
        inv = np.where(pos, ONE / np.sqrt(np.where(pos, l2, ONE)), ZERO).astype(f32)
        nh = np.where(pos[..., None], n * inv[..., None], ZERO).astype(f32)
        zero_n = (nh[..., 0] == 0) & (nh[..., 1] == 0) & (nh[..., 2] == 0)
        ad = _max(a, MIN_ALBEDO) if demodulate else None
        e = (c / ad).astype(f32) if demodulate else c.copy()
        g = _g(e)
        sa = f32(sigma_albedo)
        ia = ONE / (sa * sa)
        sc = f32(sigma_color)
        inv_c = ONE / (sc * sc)
        log2p = int(normal_power).bit_length() - 1
        ys, xs = np.mgrid[0:h, 0:w]
        for i in range(iterations):
            s = 1 << i
            ic = f32(4 ** i) * inv_c
            sum_e = np.zeros_like(e)
            sum_w = np.zeros((h, w), f32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qy, qx = ys + s * dy, xs + s * dx
                    valid = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                    qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                    hh = H[dx + 2] * H[dy + 2]
                    eq = e[qy, qx]
                    if dx == 0 and dy == 0:
                        wt = np.full((h, w), hh, f32)
                    else:
                        nq = nh[qy, qx]
                        d = (nh[..., 0] * nq[..., 0] + nh[..., 1] * nq[..., 1]) + nh[..., 2] * nq[..., 2]
                        d = _max(d, ZERO)
                        d = np.where(zero_n & zero_n[qy, qx], ONE, d).astype(f32)
                        for _ in range(log2p):
                            d = d * d
                        da = a - a[qy, qx]
                        wa = ONE / (ONE + ((da[..., 0] * da[..., 0] + da[..., 1] * da[..., 1]) + da[..., 2] * da[..., 2]) * ia)
                        dc = g - g[qy, qx]
                        wc = ONE / (ONE + ((dc[..., 0] * dc[..., 0] + dc[..., 1] * dc[..., 1]) + dc[..., 2] * dc[..., 2]) * ic)
                        wt = hh * ((d * wa) * wc)
                    sum_e = np.where(valid[..., None], sum_e + eq * wt[..., None], sum_e).astype(f32)
                    sum_w = np.where(valid, sum_w + wt, sum_w).astype(f32)
            e = (sum_e / sum_w[..., None]).astype(f32)
            g = _g(e)
        out = e * ad if demodulate else e
    return np.concatenate([out.astype(f32), np.ones((h, w, 1), f32)], axis=2)


def b3_blur(x):
    """the plain B3-spline blur at step 1 with out-of-frame taps dropped (the weights of the remaining taps renormalised)"""
    x = np.asarray(x, np.float64)
    h, w = x.shape[:2]
    hk = [1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16]
    s = np.zeros_like(x)
    sw = np.zeros((h, w))
    ys, xs = np.mgrid[0:h, 0:w]
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            qy, qx = ys + dy, xs + dx
            valid = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
            wt = hk[dx + 2] * hk[dy + 2] * valid
            s += x[np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)] * wt[..., None]
            sw += wt
    return s / sw[..., None]
