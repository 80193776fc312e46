"""numpy twin of docs/RENDER_SPEC.md 16 "Vertex motion": temporal reprojection that follows vertex edits on a one-level tree.  resolve()
and capture() extend tests/temporal_ref.py by the current triangle table, the history's snapshot of it and the vertex marks; the
projection, the motion of an instance and the float32 building blocks are temporal_ref's own.  tris_of() restates RENDER_SPEC 3 (what
k_flatten writes into tris_by_id) in float32.  csrc/temporal.hip is held to this file byte for byte (tests/test_temporal_vertex.py).

A triangle table is [triangles, 12] uint32 in id order: (v0.xyz, id), (e1.xyz, 0), (e2.xyz, 0), the floats by their bits."""
import dataclasses

import numpy as np

import temporal_ref as T
from aov_ref import dot, fma

f32 = np.float32
ABSENT = T.ABSENT
BARY_MIN = f32(-1.0)  # step 3 of the rule: the triangle plus its mirror images across its three edges (a definition, not a tuning result)


@dataclasses.dataclass
class History(T.History):
    tris: object = None  # the snapshot: the triangle table at capture, or None (captured with the feature off, or on a two-level tree)


def tris_of(scene, world):
    """the triangle table of `scene` flattened to world space: per instance (aov_ref.instance_table order) and triangle
    v[c] = fma(m8, z, fma(m4, y, m0 * x)) + m12 (and rows 1, 2 alike) of the instance's column-major transform world[i], then e1 = v1 - v0,
    e2 = v2 - v0.  world: [instances, 16] float32"""
    world = np.asarray(world, dtype=f32).reshape(-1, 16)
    prims = [p for nd in scene.nodes if nd.mesh_index != 0xFFFFFFFF for p in scene.meshes[nd.mesh_index].primitives]
    out, first = [], 0
    for m, p in zip(world, prims):
        idx = np.asarray(p.indices, dtype=np.int64).reshape(-1, 3)
        pos = np.asarray(p.vertices["position"], dtype=f32)
        x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
        wp = np.stack([(fma(m[8 + r], z, fma(m[4 + r], y, (m[r] * x).astype(f32))) + m[12 + r]).astype(f32) for r in range(3)], axis=-1)
        v0, v1, v2 = wp[idx[:, 0]], wp[idx[:, 1]], wp[idx[:, 2]]
        rec = np.zeros((len(idx), 12), np.uint32)
        rec[:, 0:3] = v0.view(np.uint32)
        rec[:, 3] = first + np.arange(len(idx), dtype=np.uint32)
        rec[:, 4:7] = (v1 - v0).astype(f32).view(np.uint32)
        rec[:, 8:11] = (v2 - v0).astype(f32).view(np.uint32)
        out.append(rec)
        first += len(idx)
    return np.concatenate(out) if out else np.zeros((0, 12), np.uint32)


def by_id(tris_u32):
    """a downloaded triangle array (hala_rt_download_bvh: tree order) -> the table in id order"""
    t = np.asarray(tris_u32, dtype=np.uint32).reshape(-1, 12)
    out = np.empty_like(t)
    out[t[:, 3]] = t
    return out


def _parts(tris):
    t = np.ascontiguousarray(tris, dtype=np.uint32).reshape(-1, 12).view(f32)
    return t[:, 0:3], t[:, 4:7], t[:, 8:11]


def follows(hist, tris_cur, vertex_marked):
    """whether the instances of vertex_marked can carry mark 2: a snapshot of the current triangle count"""
    return (vertex_marked is not None and np.any(vertex_marked) and hist is not None and getattr(hist, "tris", None) is not None
            and tris_cur is not None and np.shape(hist.tris) == np.shape(tris_cur))


def resolve(C, Pm, I, n, hist, cam_cur, world_cur, inst_marked=None, mat_marked=None, material_count=None, params=T.Params(), tris_cur=None,
            vertex_marked=None):
    """temporal_ref.resolve plus RENDER_SPEC 16 "Vertex motion".  vertex_marked: bool per instance, the vertex marks while the feature is on
    and the tree is one-level (else None); inst_marked: every other instance mark.  An instance of vertex_marked carries mark 2 when
    hist.tris is a snapshot of tris_cur's size and W_cur is invertible, else mark 1.  With no mark 2 this is temporal_ref.resolve."""
    world_cur = np.asarray(world_cur, dtype=f32).reshape(-1, 16)
    ni = world_cur.shape[0]
    vm = np.zeros(ni, bool) if vertex_marked is None else np.asarray(vertex_marked, bool)
    im = np.zeros(ni, bool) if inst_marked is None else np.asarray(inst_marked, bool)
    # every vertex mark as "no history": the pixels of mark 2 are overwritten below
    Tm, M = T.resolve(C, Pm, I, n, hist, cam_cur, world_cur, im | vm, mat_marked, material_count, params)
    if hist is None or hist.world.shape != world_cur.shape or not follows(hist, tris_cur, vm):
        return Tm, M
    two = vm & ~im
    for i in np.nonzero(two)[0]:
        two[i] = T.motion_matrix(hist.world[i], world_cur[i])[1]
    if not two.any():
        return Tm, M
    H, W = C.shape[:2]
    N = H * W
    Cf = np.ascontiguousarray(C, dtype=f32).reshape(N, 4)
    Pf = np.ascontiguousarray(Pm, dtype=f32).reshape(N, 4)
    If = np.ascontiguousarray(I).view(np.uint32).reshape(N, 4)
    nf = f32(n)
    Tm, M = Tm.reshape(N, 4).copy(), M.reshape(N, 4).copy()
    nm = int(material_count) if material_count is not None else (len(mat_marked) if mat_marked is not None else int(1 << 31))
    mmark = np.zeros(0, bool) if mat_marked is None else np.asarray(mat_marked, bool)
    inst, mat, gid = If[:, 1], If[:, 2], If[:, 3]
    v0c, e1c, e2c = _parts(tris_cur)
    v0p, e1p, e2p = _parts(hist.tris)
    nt = v0c.shape[0]
    one = f32(1.0)
    with np.errstate(all="ignore"):
        live = (inst != ABSENT) & (Pf[:, 3] > f32(0.0)) & (inst < ni) & (mat < nm)
        live[live] &= two[inst[live]]
        if mmark.size:  # a material mark wins
            k = live & (mat < mmark.size)
            live[k] &= ~mmark[mat[k]]
        live &= gid < nt
        idx = np.nonzero(live)[0]
        if idx.size == 0:
            return Tm.reshape(H, W, 4), M.reshape(H, W, 4)
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
        ok = (det > f32(0.0)) & (u >= BARY_MIN) & (v >= BARY_MIN) & (w0 >= BARY_MIN)
        idx, g, Pw, u, v, v0, e1, e2 = idx[ok], g[ok], Pw[ok], u[ok], v[ok], v0[ok], e1[ok], e2[ok]
        R = np.stack([fma(v, e2[:, c], fma(u, e1[:, c], v0[:, c])) for c in range(3)], axis=-1)
        Pprev = np.stack([fma(v, e2p[g][:, c], fma(u, e1p[g][:, c], v0p[g][:, c])) for c in range(3)], axis=-1)
        ok = np.isfinite(Pprev).all(axis=-1)
        idx, Pw, R, Pprev = idx[ok], Pw[ok], R[ok], Pprev[ok]
        if idx.size == 0:
            return Tm.reshape(H, W, 4), M.reshape(H, W, 4)
        au, av, az, aok = T.project(hist.cam, Pprev, W, H)
        bu, bv, bz, bok = T.project(cam_cur, R, W, H)
        r = (Pw - R).astype(f32)
        if cam_cur.type == 0:
            zc = bz
        else:
            zc = np.full(idx.shape, f32(f32(2.0) * cam_cur.ymag) * np.sqrt(dot(cam_cur.up, cam_cur.up)), f32)
        rl = (f32(params.tol) * zc).astype(f32)
        r2 = ((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]).astype(f32) + r[:, 2] * r[:, 2]).astype(f32)
        ok = aok & bok & (r2 <= (rl * rl).astype(f32))
        idx, Pprev, au, av, az, bu, bv = idx[ok], Pprev[ok], au[ok], av[ok], az[ok], bu[ok], bv[ok]
        # from here on: steps 2-5 of the existing rule, as temporal_ref.resolve writes them
        mx, my = (au - bu).astype(f32), (av - bv).astype(f32)
        M[idx] = np.stack([mx, my, az, np.ones_like(mx)], axis=-1)
        px, py = (idx % W).astype(f32), (idx // W).astype(f32)
        fx, fy = (px + mx).astype(f32), (py + my).astype(f32)
        inside = (fx > f32(-1.0)) & (fx < f32(W)) & (fy > f32(-1.0)) & (fy < f32(H))
        idx, Pprev, az, fx, fy = idx[inside], Pprev[inside], az[inside], fx[inside], fy[inside]
        x0f, y0f = np.floor(fx), np.floor(fy)
        tx, ty = (fx - x0f).astype(f32), (fy - y0f).astype(f32)
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        if hist.cam.type == 0:
            zt = az
        else:
            zt = np.full(idx.shape, f32(f32(2.0) * hist.cam.ymag) * np.sqrt(dot(hist.cam.up, hist.cam.up)), f32)
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
        mh = f32(params.max_history)
        h = np.where(hl > mh, mh, hl).astype(f32)
        tw = (h + nf).astype(f32)
        rgb = (((hrgb * h[:, None]).astype(f32) + (Cf[idx, :3] * nf).astype(f32)).astype(f32) / tw[:, None]).astype(f32)
        Tm[idx] = np.concatenate([rgb, tw[:, None]], axis=1)
    return Tm.reshape(H, W, 4), M.reshape(H, W, 4)


def capture(C, Pm, I, n, hist, cam_cur, world_cur, inst_marked=None, mat_marked=None, material_count=None, params=T.Params(), tris_cur=None,
            vertex_marked=None, snapshot=False):
    """RENDER_SPEC 16 "Capture" with the snapshot: the new history keeps tris_cur when `snapshot` (the feature is on and the tree is
    one-level), else none.  n = 0: the old history, untouched"""
    if n == 0:
        return hist
    Tm, _ = resolve(C, Pm, I, n, hist, cam_cur, world_cur, inst_marked, mat_marked, material_count, params, tris_cur, vertex_marked)
    return History(Tm, np.array(Pm, dtype=f32), np.ascontiguousarray(I).view(np.uint32).copy(), cam_cur,
                   np.asarray(world_cur, dtype=f32).reshape(-1, 16).copy(),
                   np.array(tris_cur, dtype=np.uint32).reshape(-1, 12).copy() if snapshot and tris_cur is not None else None)
