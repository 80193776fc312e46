"""The float32 numpy twin of transfer bakes (docs/RENDER_SPEC.md 4.13), operation for operation, by brute force: the receiver's samples
and texel records are bake_ref's (4.11), every owned texel's ray is tested against every triangle of the scene in the arithmetic of
multihit_ref.Twin.lists (the cross / dot / fma of RENDER_SPEC 2.1, the acceptance of 4.2, the far-origin rule restated), the triangles
of instances that are no targets are struck out ahead of the minimum by (t', id), the hit's normal is bake_ref's shading normal of the
HIT triangle, and the dilation is bake_ref's, which copies rows of any record dtype.  Nothing of the oracle's ray casting is used.

    twin = Twin(bake_ref.Twin(scene, osc), osc)
    samples, texels = twin.base.samples(instance, W, H, flags=flags)          # RENDER_SPEC 4.11
    rays, valid = twin.rays(samples, front, back)                              # A.RAY_DTYPE, [W * H]; valid: the texel has a ray
    hits = twin.first(rays, valid, twin.target_mask(instance, targets))        # Hits: t' (re-based), u, v, prim, ts
    rec = twin.records(hits, front)                                            # A.BAKE_TRANSFER_HIT_DTYPE, undilated
    rec, texels = twin.transfer(instance, W, H, flags, front, back, targets, margin)   # all of it, then bake_ref.dilate
    first64(twin, rays, valid, mask)                                           # the same rays and filtered minimum in float64
"""
import numpy as np

import bake_ref as BR
import hala_renderer_amd as H
import multihit_ref as MR
import occlusion_ref as OR
from aov_ref import cross, dot, fma

f32, f64 = np.float32, np.float64
A = H._abi
MISS = 0xFFFFFFFF


class Hits:
    """per ray: t (of the re-based ray; +inf: none), u, v, prim (MISS: none), ts (the distance a far origin was moved, 0 elsewhere)"""
    def __init__(self, t, u, v, prim, ts, far):
        self.t, self.u, self.v, self.prim, self.ts, self.far = t, u, v, prim, ts, far

    @property
    def found(self):
        return self.prim != MISS


class Twin:
    def __init__(self, base, osc):
        self.base = base  # bake_ref.Twin: v0, e1, e2, inst, first, shading_normal, samples
        mn, mx = osc.bounds()
        self.box_min, self.box_max = mn.astype(f32), mx.astype(f32)
        self.far_limit = MR.REBASE_K * f32(max(np.abs(mn).max(), np.abs(mx).max()))
        ext = (mx - mn).astype(f32)
        self.diag = f32(np.sqrt(dot(ext, ext)))

    @property
    def instances(self):
        return len(self.base.first) - 1

    def target_mask(self, receiver, targets=None):
        """[instances] bool: the target set; None or empty: every instance but the receiver.  A set: the order of `targets` is lost here"""
        mask = np.zeros(self.instances, bool)
        if targets is None or len(targets) == 0:
            mask[:] = True
            mask[receiver] = False
        else:
            mask[np.asarray(targets, dtype=np.int64)] = True
            assert not mask[receiver] and mask.sum() == len(targets)
        return mask

    @staticmethod
    def rays(samples, front, back):
        """RENDER_SPEC 4.13: validity is 4.10's rule on (point, 0, normal); n = normal * (1 / sqrt(nn)), o = fma(n, front, point), d = -n,
        tmin = 0, tmax = front + back (one float add).  Rows of texels without a ray are zero."""
        s0 = samples.copy()
        s0["bias"] = 0.0
        valid, nn = OR.valid_flags(s0)
        rays = np.zeros(len(samples), dtype=A.RAY_DTYPE)
        with np.errstate(all="ignore"):
            inv = (f32(1.0) / np.sqrt(nn.astype(f32))).astype(f32)
            n = (samples["normal"].astype(f32) * inv[:, None]).astype(f32)
            o = fma(n, np.broadcast_to(f32(front), n.shape), samples["point"].astype(f32))
            tmax = f32(f32(front) + f32(back))
        rays["origin"][valid], rays["direction"][valid] = o[valid], -n[valid]
        rays["tmax"][valid] = tmax
        return rays, valid

    def rebase(self, rays):
        """RENDER_SPEC 4.2, far origins, as multihit_ref.Twin.rebase states it: (o', tmin', tmax', ts, far)"""
        o = rays["origin"].astype(f32).copy(); d = rays["direction"].astype(f32)
        tmin = rays["tmin"].astype(f32).copy(); tmax = rays["tmax"].astype(f32).copy()
        far = np.abs(o).max(axis=1) > self.far_limit
        ts = np.zeros(len(rays), f32)
        if far.any():
            with np.errstate(all="ignore"):
                of, df = o[far], d[far]
                idir = MR._safe_inv(df)
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

    def first(self, rays, valid, mask):
        """the least (t', id) over the triangles of the instances `mask` marks, of every valid ray: the arithmetic of multihit_ref.Twin.lists"""
        b = self.base
        n, T = len(rays), len(b.v0)
        o_all, tmin_all, tmax_all, ts, far = self.rebase(rays)
        tmin_all = np.where(tmin_all > 0.0, tmin_all, f32(0.0)).astype(f32)
        d_all = rays["direction"].astype(f32)
        out_t = np.full(n, np.inf, f32); out_u = np.zeros(n, f32); out_v = np.zeros(n, f32); out_p = np.full(n, MISS, np.uint32)
        admitted = mask[b.inst] if T else np.zeros(0, bool)
        which = np.nonzero(valid)[0]
        chunk = max(8, min(512, 1_500_000 // max(T, 1)))
        E1, E2, V0 = b.e1[None], b.e2[None], b.v0[None]
        with np.errstate(all="ignore"):
            for a in range(0, len(which) if T else 0, chunk):
                sel = which[a:a + chunk]
                m = len(sel)
                O3, D3 = np.broadcast_to(o_all[sel][:, None, :], (m, T, 3)), np.broadcast_to(d_all[sel][:, None, :], (m, T, 3))
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
                ok &= (t > tmin_all[sel, None]) & (t < tmax_all[sel, None])
                ok &= admitted[None, :]
                best = np.argmin(np.where(ok, t, f32(np.inf)), axis=1)  # the first least: equal t goes to the lower id
                got = ok[np.arange(m), best]
                rows = np.arange(m)[got]
                out_t[sel[got]] = t[rows, best[got]]; out_u[sel[got]] = u[rows, best[got]]; out_v[sel[got]] = v[rows, best[got]]
                out_p[sel[got]] = best[got].astype(np.uint32)
        return Hits(out_t, out_u, out_v, out_p, ts, far)

    def records(self, hits, front):
        """RENDER_SPEC 4.13's record of every ray: t = t' + ts, the hit triangle's shading normal at (u, v), height = front - t"""
        rec = np.zeros(len(hits.t), dtype=A.BAKE_TRANSFER_HIT_DTYPE)
        rec["t"], rec["prim"] = f32(-1.0), MISS
        m = hits.found
        if m.any():
            ids = hits.prim[m].astype(np.int64)
            with np.errstate(all="ignore"):
                t = (hits.t[m] + hits.ts[m]).astype(f32)
                rec["normal"][m] = self.base.shading_normal(ids, hits.u[m], hits.v[m])
                rec["height"][m] = (f32(front) - t).astype(f32)
            rec["t"][m], rec["u"][m], rec["v"][m], rec["prim"][m] = t, hits.u[m], hits.v[m], hits.prim[m]
        return rec

    def transfer(self, receiver, W, H, flags, front, back, targets=None, margin=0, owner=None):
        """(records, texels) [H * W] of one call, dilated"""
        samples, texels = self.base.samples(receiver, W, H, flags=flags, owner=owner)
        rays, valid = self.rays(samples, front, back)
        rec = self.records(self.first(rays, valid, self.target_mask(receiver, targets)), front)
        return BR.dilate(rec, texels, W, H, margin) if margin else (rec, texels)


def first64(twin, rays, valid, mask):
    """The reference of the float64 comparison: the same float32 rays (re-based as the twin re-bases them) against the float32 triangle
    records, every operation of the test and the filtered minimum in float64.  -> (t' [n] float64, +inf: none; prim [n])"""
    b = twin.base
    n, T = len(rays), len(b.v0)
    o_all, tmin_all, tmax_all, _, _ = twin.rebase(rays)
    d_all = rays["direction"].astype(f64)
    o_all, tmin_all, tmax_all = o_all.astype(f64), np.maximum(tmin_all.astype(f64), 0.0), tmax_all.astype(f64)
    out_t = np.full(n, np.inf, f64); out_p = np.full(n, MISS, np.uint32)
    admitted = mask[b.inst] if T else np.zeros(0, bool)
    which = np.nonzero(valid)[0]
    chunk = max(8, min(512, 1_000_000 // max(T, 1)))
    e1, e2, v0 = b.e1.astype(f64)[None], b.e2.astype(f64)[None], b.v0.astype(f64)[None]
    with np.errstate(all="ignore"):
        for a in range(0, len(which) if T else 0, chunk):
            sel = which[a:a + chunk]
            m = len(sel)
            o, d = o_all[sel][:, None, :], d_all[sel][:, None, :]
            p = np.cross(d, e2)
            det = (e1 * p).sum(-1)
            tv = o - v0
            u = (tv * p).sum(-1) / det
            q = np.cross(tv, e1)
            v = (d * q).sum(-1) / det
            t = (e2 * q).sum(-1) / det
            ok = (det != 0.0) & (u >= 0.0) & (u <= 1.0) & (v >= 0.0) & (u + v <= 1.0) & (t > tmin_all[sel, None]) & (t < tmax_all[sel, None])
            ok &= admitted[None, :]
            best = np.argmin(np.where(ok, t, np.inf), axis=1)
            got = ok[np.arange(m), best]
            out_t[sel[got]] = t[np.arange(m)[got], best[got]]
            out_p[sel[got]] = best[got].astype(np.uint32)
    return out_t, out_p
