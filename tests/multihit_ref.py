"""numpy twin of multi-hit ray batches (docs/RENDER_SPEC.md 4.7): brute force over all triangles of the scene in float32, with the fma,
dot and cross of aov_ref (RENDER_SPEC 2.1).  Nothing of the oracle's ray casting is used: the triangles come from the scene description,
flattened by the arithmetic of RENDER_SPEC 3 (the oracle only supplies the node world matrices and the scene bounds, as it does for
aov_ref); instanced primitives stay in object space and the ray is moved to them (4.5); the far-origin rule of 4.2 is restated here.

    twin = Twin(scene, oracle_scene, instancing=False)
    full = twin.lists(rays)          # every ray's whole hit list, sorted by (t', id): the expensive part, shared by all k
    rec, counts = cut(full, k)       # [n, k] hit records padded with miss records, [n] counts
    full.tie, straddles(full, k)     # per ray: its list holds two equal t'; a pair of equal t' sits at positions k - 1, k
"""
import numpy as np

import hala_renderer_amd as H
from aov_ref import cross, dot, fma

f32 = np.float32
A = H._abi
MISS = 0xFFFFFFFF
REBASE_K = f32(16.0)  # RENDER_SPEC 4.2
KEEP = A.MAX_MULTI_HITS + 1  # columns kept of a sorted list: the largest k and the entry behind it


def _transform_point(m, p):
    """RENDER_SPEC 3: p' = fma(m8, z, fma(m4, y, m0 * x)) + m12 (rows 1, 2 alike); m = 16 floats, column-major"""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([fma(m[8 + r], z, fma(m[4 + r], y, m[r] * x)) + m[12 + r] for r in range(3)], axis=1).astype(f32)


def _world_to_object(m):
    """RENDER_SPEC 4.5: rows r_i = k_i * (1 / det) of the inverse of the upper 3x3 and the translation, or None"""
    c0, c1, c2 = m[0:3], m[4:7], m[8:11]
    k0, k1, k2 = cross(c1, c2), cross(c2, c0), cross(c0, c1)
    det = f32(dot(c0, k0))
    if not (det != 0.0) or not np.isfinite(det):
        return None
    with np.errstate(all="ignore"):
        inv = f32(1.0) / det
        rows = np.stack([k0 * inv, k1 * inv, k2 * inv]).astype(f32)
    tr = m[12:15].astype(f32)
    return (rows, tr) if np.isfinite(rows).all() and np.isfinite(tr).all() else None


def _safe_inv(d):
    """RENDER_SPEC 4.3"""
    dd = np.where(np.abs(d) < f32(1e-20), np.copysign(f32(1e-20), d), d).astype(f32)
    return (f32(1.0) / dd).astype(f32)


class Lists:
    """the sorted hit lists of a ray set: t (re-based ray), u, v, prim as [n, KEEP] (columns beyond a ray's hits: +inf, 0, 0, MISS), total
    = hits per ray (all of them), ts = the distance a far origin was moved (0 elsewhere), tie = the whole list holds two equal t"""
    def __init__(self, t, u, v, prim, total, ts, tie, far):
        self.t, self.u, self.v, self.prim, self.total, self.ts, self.tie, self.far = t, u, v, prim, total, ts, tie, far


class Twin:
    def __init__(self, scene, osc, instancing=False):
        import oracle_lib as O
        world = O.world_transforms(scene)
        refs = {}
        for nd in scene.nodes:
            if nd.mesh_index != H.scene.INVALID:
                for p in range(len(scene.meshes[nd.mesh_index].primitives)):
                    refs[(nd.mesh_index, p)] = refs.get((nd.mesh_index, p), 0) + 1
        v0, e1, e2, inst_of = [], [], [], []
        self.inst = []  # per instance: None (flattened) or (rows, tr)
        for k, nd in enumerate(scene.nodes):
            if nd.mesh_index == H.scene.INVALID:
                continue
            m = world[k].astype(f32)
            for p, pr in enumerate(scene.meshes[nd.mesh_index].primitives):
                idx = np.asarray(pr.indices, dtype=np.int64)[: (len(pr.indices) // 3) * 3].reshape(-1, 3)
                pos = np.ascontiguousarray(pr.vertices["position"], dtype=f32)
                w2o = _world_to_object(m) if instancing and refs[(nd.mesh_index, p)] >= 2 and len(idx) >= 1 else None
                pts = pos if w2o is not None else _transform_point(m, pos)
                a, b, c = pts[idx[:, 0]], pts[idx[:, 1]], pts[idx[:, 2]]
                v0.append(a); e1.append(b - a); e2.append(c - a)
                inst_of.append(np.full(len(idx), len(self.inst), dtype=np.int64))
                self.inst.append(w2o)
        self.v0, self.e1, self.e2 = (np.concatenate(x).astype(f32) if x else np.zeros((0, 3), f32) for x in (v0, e1, e2))
        self.inst_of = np.concatenate(inst_of) if inst_of else np.zeros(0, np.int64)
        mn, mx = osc.bounds()
        self.box_min, self.box_max = mn.astype(f32), mx.astype(f32)
        self.far_limit = REBASE_K * f32(max(np.abs(mn).max(), np.abs(mx).max()))
        ext = (mx - mn).astype(f32)
        self.diag = f32(np.sqrt(dot(ext, ext)))

    def rebase(self, rays):
        """RENDER_SPEC 4.2, far origins: (o', tmin', tmax', ts, far)"""
        o = rays["origin"].astype(f32).copy(); d = rays["direction"].astype(f32)
        tmin = rays["tmin"].astype(f32).copy(); tmax = rays["tmax"].astype(f32).copy()
        far = np.abs(o).max(axis=1) > self.far_limit
        ts = np.zeros(len(rays), f32)
        if far.any():
            with np.errstate(all="ignore"):
                of, df = o[far], d[far]
                idir = _safe_inv(df)
                ood = of * idir
                t0 = fma(np.broadcast_to(self.box_min, of.shape), idir, -ood)
                t1 = fma(np.broadcast_to(self.box_max, of.shape), idir, -ood)
                lo = np.fmin(t0, t1)
                tn = np.fmax(np.fmax(lo[:, 0], lo[:, 1]), np.fmax(lo[:, 2], f32(0.0)))
                s = np.fmax(tn - self.diag, f32(0.0)).astype(f32)
                o[far] = fma(df, s[:, None], of)
                tmin[far] = np.fmax(tmin[far] - s, f32(0.0))
                tmax[far] = tmax[far] - s
                ts[far] = s
        return o, tmin, tmax, ts, far

    def lists(self, rays, chunk=128):
        rays = np.ascontiguousarray(rays, dtype=A.RAY_DTYPE)
        n, T = len(rays), len(self.v0)
        o_all, tmin_all, tmax_all, ts, far = self.rebase(rays)
        tmin_all = np.where(tmin_all > 0.0, tmin_all, f32(0.0)).astype(f32)  # rays start at or after their origin (a NaN tmin too)
        d_all = rays["direction"].astype(f32)
        out_t = np.full((n, KEEP), np.inf, f32); out_u = np.zeros((n, KEEP), f32); out_v = np.zeros((n, KEEP), f32)
        out_p = np.full((n, KEEP), MISS, np.uint32)
        total = np.zeros(n, np.int64); tie = np.zeros(n, bool)
        any_inst = any(w is not None for w in self.inst)
        E1, E2, V0 = self.e1[None], self.e2[None], self.v0[None]
        with np.errstate(all="ignore"):
            for a in range(0, n, chunk):
                o, d = o_all[a:a + chunk], d_all[a:a + chunk]
                m = len(o)
                if any_inst:  # the ray each triangle is tested with: the world-space ray, or the one moved into its instance's object space
                    oi = np.repeat(o[:, None, :], len(self.inst), axis=1); di = np.repeat(d[:, None, :], len(self.inst), axis=1)
                    for i, w in enumerate(self.inst):
                        if w is None:
                            continue
                        rows, tr = w
                        tv = (o - tr).astype(f32)
                        oi[:, i] = np.stack([dot(np.broadcast_to(rows[r], tv.shape), tv) for r in range(3)], axis=1)
                        di[:, i] = np.stack([dot(np.broadcast_to(rows[r], d.shape), d) for r in range(3)], axis=1)
                    O3, D3 = oi[:, self.inst_of], di[:, self.inst_of]
                else:
                    O3, D3 = np.broadcast_to(o[:, None, :], (m, T, 3)), np.broadcast_to(d[:, None, :], (m, T, 3))
                e1, e2 = np.broadcast_to(E1, (m, T, 3)), np.broadcast_to(E2, (m, T, 3))
                p = cross(D3, e2)
                det = dot(e1, p)
                inv = (f32(1.0) / det).astype(f32)
                tv = (O3 - V0).astype(f32)
                u = (dot(tv, p) * inv).astype(f32)
                q = cross(tv, e1)
                v = (dot(D3, q) * inv).astype(f32)
                t = (dot(e2, q) * inv).astype(f32)
                ok = (det != 0.0) & (u >= 0.0) & (u <= 1.0) & (v >= 0.0) & ((u + v).astype(f32) <= 1.0)
                ok &= (t > tmin_all[a:a + chunk, None]) & (t < tmax_all[a:a + chunk, None])
                ts_sort = np.where(ok, t, f32(np.inf))
                order = np.argsort(ts_sort, axis=1, kind="stable")  # stable: equal t keeps ascending triangle id
                cnt = ok.sum(axis=1)
                total[a:a + chunk] = cnt
                srt = np.take_along_axis(ts_sort, order, axis=1)
                if T > 1:
                    tie[a:a + chunk] = ((srt[:, 1:] == srt[:, :-1]) & (np.arange(1, T)[None, :] < cnt[:, None])).any(axis=1)
                keep = min(KEEP, T)
                head = order[:, :keep]
                valid = np.arange(keep)[None, :] < cnt[:, None]
                out_t[a:a + m, :keep] = np.where(valid, np.take_along_axis(t, head, axis=1), f32(np.inf))
                out_u[a:a + m, :keep] = np.where(valid, np.take_along_axis(u, head, axis=1), f32(0.0))
                out_v[a:a + m, :keep] = np.where(valid, np.take_along_axis(v, head, axis=1), f32(0.0))
                out_p[a:a + m, :keep] = np.where(valid, head.astype(np.uint32), np.uint32(MISS))
        return Lists(out_t, out_u, out_v, out_p, total, ts, tie, far)


def cut(full, k):
    """the answer of RENDER_SPEC 4.7 for capacity k: (records [n, k], counts [n])"""
    assert 1 <= k <= A.MAX_MULTI_HITS
    n = len(full.total)
    counts = np.minimum(full.total, k).astype(np.uint32)
    valid = np.arange(k)[None, :] < counts[:, None]
    rec = np.zeros((n, k), dtype=A.HIT_DTYPE)
    with np.errstate(all="ignore"):
        rec["t"] = np.where(valid, (full.t[:, :k] + full.ts[:, None]).astype(f32), f32(-1.0))  # reported: t' + ts, one float add
    rec["u"] = np.where(valid, full.u[:, :k], f32(0.0))
    rec["v"] = np.where(valid, full.v[:, :k], f32(0.0))
    rec["prim"] = np.where(valid, full.prim[:, :k], np.uint32(MISS))
    return rec, counts


def straddles(full, k):
    """per ray: entries k - 1 and k of its list (the last one kept and the first one cut) have the same t"""
    return (full.total > k) & (full.t[:, k - 1] == full.t[:, k])
