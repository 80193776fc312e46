"""numpy twin of docs/RENDER_SPEC.md 16 "History clamp": the resolve of temporal reprojection, rigid and vertex motion alike, with the
reprojected history colour clamped to the neighbourhood statistics of the current accumulation before the blend.  resolve() and capture()
take what tests/temporal_vertex_ref.py's take plus `clamp`: None (off) or (radius, gamma).  The projection, the motion of an instance, the
triangle tables and the float32 building blocks are temporal_ref's and temporal_vertex_ref's own; the steps of the resolve are written out
once more here, from the spec text, because the clamp sits between two of them.  With clamp=None the result equals the two existing twins
bit for bit (tests/test_temporal_clamp.py); csrc/temporal.hip is held to this file byte for byte."""
import numpy as np

import temporal_ref as T
import temporal_vertex_ref as V
from aov_ref import dot, fma

f32 = np.float32
ABSENT = T.ABSENT
DEFAULT_CLAMP = (1, 2.0)


def check_params(radius, gamma, reserved=(0, 0)):
    """"" or the reason RENDER_SPEC 16 "History clamp" refuses the parameters (the wording of hala_rt_set_temporal_clamp)"""
    g = f32(gamma)
    if not (1 <= int(radius) <= 3):
        return "Invalid temporal clamp radius: expected 1, 2 or 3."
    if not (g > f32(0.0) and g <= f32(1000.0)):
        return "Invalid temporal clamp gamma: expected a finite value in (0, 1000]."
    if any(reserved):
        return "The reserved words of the temporal clamp parameters must be zero."
    return ""


def clamp_bounds(C, radius, gamma):
    """steps 1-3 of the rule for every pixel of C [H, W, >= 3] float32 -> lo, hi [H, W, 3] float32 and the tap count k [H, W] float32"""
    Hh, W = C.shape[:2]
    r = int(radius)
    rgb = np.ascontiguousarray(C[..., :3], dtype=f32)
    pad = np.zeros((Hh + 2 * r, W + 2 * r, 3), f32)
    pad[r:r + Hh, r:r + W] = rgb
    inside = np.zeros((Hh + 2 * r, W + 2 * r), bool)
    inside[r:r + Hh, r:r + W] = True
    taps = [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1)]  # dy outside, dx inside

    def tap(dy, dx):
        return pad[r + dy:r + dy + Hh, r + dx:r + dx + W], inside[r + dy:r + dy + Hh, r + dx:r + dx + W]

    with np.errstate(all="ignore"):
        k = np.zeros((Hh, W), f32)
        s1 = np.zeros((Hh, W, 3), f32)
        for dy, dx in taps:
            q, ok = tap(dy, dx)
            k = np.where(ok, (k + f32(1.0)).astype(f32), k)
            s1 = np.where(ok[..., None], (s1 + q).astype(f32), s1)
        mu = (s1 / k[..., None]).astype(f32)
        s2 = np.zeros((Hh, W, 3), f32)
        for dy, dx in taps:
            q, ok = tap(dy, dx)
            d = (q - mu).astype(f32)
            s2 = np.where(ok[..., None], (s2 + (d * d).astype(f32)).astype(f32), s2)
        v = (s2 / k[..., None]).astype(f32)
        half = (f32(gamma) * np.sqrt((v / k[..., None]).astype(f32)).astype(f32)).astype(f32)
        lo, hi = (mu - half).astype(f32), (mu + half).astype(f32)
    return lo, hi, k


def clamp_history(hrgb, lo, hi):
    """step 4: a NaN history stays NaN, NaN bounds leave the history as it is"""
    with np.errstate(invalid="ignore"):
        return np.where(hrgb < lo, lo, np.where(hrgb > hi, hi, hrgb)).astype(f32)


def resolve(C, Pm, I, n, hist, cam_cur, world_cur, inst_marked=None, mat_marked=None, material_count=None, params=T.Params(), tris_cur=None,
            vertex_marked=None, clamp=None):
    """-> (temporal, motion) [H, W, 4] float32: temporal_vertex_ref.resolve with the history clamp.  clamp: None or (radius, gamma)"""
    H, W = C.shape[:2]
    N = H * W
    Cf = np.ascontiguousarray(C, dtype=f32).reshape(N, 4)
    Pf = np.ascontiguousarray(Pm, dtype=f32).reshape(N, 4)
    If = np.ascontiguousarray(I).view(np.uint32).reshape(N, 4)
    nf = f32(n)
    Tm = np.concatenate([Cf[:, :3], np.full((N, 1), nf, f32)], axis=1)
    M = np.zeros((N, 4), f32)
    done = lambda: (Tm.reshape(H, W, 4), M.reshape(H, W, 4))  # noqa: E731
    world_cur = np.asarray(world_cur, dtype=f32).reshape(-1, 16)
    if hist is None or hist.world.shape != world_cur.shape:
        return done()
    ni = world_cur.shape[0]
    nm = int(material_count) if material_count is not None else (len(mat_marked) if mat_marked is not None else int(1 << 31))
    # the mark of every instance: 0 rigid motion by D, 1 no history, 2 vertex motion
    im = np.zeros(ni, bool) if inst_marked is None else np.asarray(inst_marked, bool)
    vm = np.zeros(ni, bool) if vertex_marked is None else np.asarray(vertex_marked, bool)
    follow = V.follows(hist, tris_cur, vm)
    D = np.empty((ni, 3, 4), f32)
    mark = np.zeros(ni, np.int64)
    for i in range(ni):
        D[i], ok = T.motion_matrix(hist.world[i], world_cur[i])
        mark[i] = 1 if (not ok or im[i] or (vm[i] and not follow)) else (2 if vm[i] else 0)
    mmark = np.zeros(0, bool) if mat_marked is None else np.asarray(mat_marked, bool)
    inst, mat, gid = If[:, 1], If[:, 2], If[:, 3]
    one = f32(1.0)
    with np.errstate(all="ignore"):
        live = (inst != ABSENT) & (Pf[:, 3] > f32(0.0)) & (inst < ni) & (mat < nm)
        if mmark.size:  # a material mark wins over vertex motion
            k = live & (mat < mmark.size)
            live[k] &= ~mmark[mat[k]]
        imark = np.full(N, 1, np.int64)
        imark[live] = mark[inst[live]]
        # rigid motion: Pprev = D . Pw, and cam_cur projects Pw
        idx = np.nonzero(live & (imark == 0))[0]
        Pw = (Pf[idx, :3] / Pf[idx, 3:4]).astype(f32)
        Di = D[inst[idx]]
        Pprev = np.stack([fma(Di[:, r, 2], Pw[:, 2], fma(Di[:, r, 1], Pw[:, 1], fma(Di[:, r, 0], Pw[:, 0], Di[:, r, 3]))) for r in range(3)],
                         axis=-1).reshape(-1, 3)
        au, av, az, aok = T.project(hist.cam, Pprev, W, H)
        bu, bv, _, bok = T.project(cam_cur, Pw, W, H)
        ok = aok & bok
        parts = [(idx[ok], Pprev[ok], au[ok], av[ok], az[ok], bu[ok], bv[ok])]
        # vertex motion: the barycentrics of the foot of Pw on its triangle now, placed on the triangle now (R) and as captured (Pprev)
        idx = np.nonzero(live & (imark == 2))[0]
        if idx.size:
            v0c, e1c, e2c = V._parts(tris_cur)
            v0p, e1p, e2p = V._parts(hist.tris)
            idx = idx[gid[idx] < v0c.shape[0]]
            g = gid[idx].astype(np.int64)
            Pw = (Pf[idx, :3] / Pf[idx, 3:4]).astype(f32)
            v0, e1, e2 = v0c[g], e1c[g], e2c[g]
            q = (Pw - v0).astype(f32)
            d11, d12, d22 = dot(e1, e1), dot(e1, e2), dot(e2, e2)
            q1, q2 = dot(q, e1), dot(q, e2)
            det = ((d11 * d22).astype(f32) - (d12 * d12).astype(f32)).astype(f32)
            u = (((d22 * q1).astype(f32) - (d12 * q2).astype(f32)).astype(f32) / det).astype(f32)
            v = (((d11 * q2).astype(f32) - (d12 * q1).astype(f32)).astype(f32) / det).astype(f32)
            w0 = ((one - u).astype(f32) - v).astype(f32)
            ok = (det > f32(0.0)) & (u >= V.BARY_MIN) & (v >= V.BARY_MIN) & (w0 >= V.BARY_MIN)
            idx, g, Pw, u, v, v0, e1, e2 = idx[ok], g[ok], Pw[ok], u[ok], v[ok], v0[ok], e1[ok], e2[ok]
            R = np.stack([fma(v, e2[:, c], fma(u, e1[:, c], v0[:, c])) for c in range(3)], axis=-1).reshape(-1, 3)
            Pprev = np.stack([fma(v, e2p[g][:, c], fma(u, e1p[g][:, c], v0p[g][:, c])) for c in range(3)], axis=-1).reshape(-1, 3)
            ok = np.isfinite(Pprev).all(axis=-1)
            idx, Pw, R, Pprev = idx[ok], Pw[ok], R[ok], Pprev[ok]
            au, av, az, aok = T.project(hist.cam, Pprev, W, H)
            bu, bv, bz, bok = T.project(cam_cur, R, W, H)
            rr = (Pw - R).astype(f32)
            zc = bz if cam_cur.type == 0 else np.full(idx.shape, f32(f32(2.0) * cam_cur.ymag) * np.sqrt(dot(cam_cur.up, cam_cur.up)), f32)
            rl = (f32(params.tol) * zc).astype(f32)
            r2 = ((rr[:, 0] * rr[:, 0] + rr[:, 1] * rr[:, 1]).astype(f32) + rr[:, 2] * rr[:, 2]).astype(f32)
            ok = aok & bok & (r2 <= (rl * rl).astype(f32))
            parts.append((idx[ok], Pprev[ok], au[ok], av[ok], az[ok], bu[ok], bv[ok]))
        idx, Pprev, au, av, az, bu, bv = (np.concatenate([p[j] for p in parts]) for j in range(7))
        if idx.size == 0:
            return done()
        # steps 2-5: the motion, the four taps, the blend
        mx, my = (au - bu).astype(f32), (av - bv).astype(f32)
        M[idx] = np.stack([mx, my, az, np.ones_like(mx)], axis=-1)
        px, py = (idx % W).astype(f32), (idx // W).astype(f32)
        fx, fy = (px + mx).astype(f32), (py + my).astype(f32)
        inside = (fx > f32(-1.0)) & (fx < f32(W)) & (fy > f32(-1.0)) & (fy < f32(H))
        idx, Pprev, az, fx, fy = idx[inside], Pprev[inside], az[inside], fx[inside], fy[inside]
        x0f, y0f = np.floor(fx), np.floor(fy)
        tx, ty = (fx - x0f).astype(f32), (fy - y0f).astype(f32)
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        zt = az if hist.cam.type == 0 else np.full(idx.shape, f32(f32(2.0) * hist.cam.ymag) * np.sqrt(dot(hist.cam.up, hist.cam.up)), f32)
        lim = (f32(params.tol) * zt).astype(f32)
        lim2 = (lim * lim).astype(f32)
        Hc = np.ascontiguousarray(hist.Hc, dtype=f32).reshape(N, 4)
        Hp = np.ascontiguousarray(hist.Hp, dtype=f32).reshape(N, 4)
        Hi = np.ascontiguousarray(hist.Hi).view(np.uint32).reshape(N, 4)
        s = np.zeros((idx.size, 4), f32)
        sw = np.zeros(idx.size, f32)
        for k in range(4):
            qx, qy = x0 + (k & 1), y0 + (k >> 1)
            wx = tx if (k & 1) else (one - tx).astype(f32)
            wy = ty if (k >> 1) else (one - ty).astype(f32)
            w = (wx * wy).astype(f32)
            valid = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H) & (w > f32(0.0))
            qq = np.where(valid, qy * W + qx, 0)
            qc, qp, qi = Hc[qq], Hp[qq], Hi[qq]
            valid &= (qc[:, 3] > f32(0.0)) & (qp[:, 3] > f32(0.0)) & (qi[:, 1] == If[idx, 1]) & (qi[:, 2] == If[idx, 2])
            e = ((qp[:, :3] / qp[:, 3:4]).astype(f32) - Pprev).astype(f32)
            d2 = ((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]).astype(f32) + e[:, 2] * e[:, 2]).astype(f32)
            valid &= d2 <= lim2
            s = np.where(valid[:, None], (s + (qc * w[:, None]).astype(f32)).astype(f32), s)
            sw = np.where(valid, (sw + w).astype(f32), sw)
        good = sw >= f32(params.min_weight)
        idx, s, sw = idx[good], s[good], sw[good]
        hrgb = (s[:, :3] / sw[:, None]).astype(f32)
        hl = (s[:, 3] / sw).astype(f32)
        if clamp is not None:  # "History clamp": between Hrgb and the blend
            lo, hi, _ = clamp_bounds(np.asarray(C, dtype=f32), clamp[0], clamp[1])
            hrgb = clamp_history(hrgb, lo.reshape(N, 3)[idx], hi.reshape(N, 3)[idx])
        mh = f32(params.max_history)
        h = np.where(hl > mh, mh, hl).astype(f32)
        tw = (h + nf).astype(f32)
        rgb = (((hrgb * h[:, None]).astype(f32) + (Cf[idx, :3] * nf).astype(f32)).astype(f32) / tw[:, None]).astype(f32)
        Tm[idx] = np.concatenate([rgb, tw[:, None]], axis=1)
    return done()


def capture(C, Pm, I, n, hist, cam_cur, world_cur, inst_marked=None, mat_marked=None, material_count=None, params=T.Params(), tris_cur=None,
            vertex_marked=None, snapshot=False, clamp=None):
    """RENDER_SPEC 16 "Capture": the history is the resolved image, so with the clamp on it is the clamped one.  n = 0: the old history"""
    if n == 0:
        return hist
    Tm, _ = resolve(C, Pm, I, n, hist, cam_cur, world_cur, inst_marked, mat_marked, material_count, params, tris_cur, vertex_marked, clamp)
    return V.History(Tm, np.array(Pm, dtype=f32), np.ascontiguousarray(I).view(np.uint32).copy(), cam_cur,
                     np.asarray(world_cur, dtype=f32).reshape(-1, 16).copy(),
                     np.array(tris_cur, dtype=np.uint32).reshape(-1, 12).copy() if snapshot and tris_cur is not None else None)
