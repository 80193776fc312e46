"""numpy twin of signed distance grids (docs/RENDER_SPEC.md 4.9) and an independent float64 reference of the sign.

    grid = Grid(origin, spacing, dims)                    # float32 origin and spacing, dims = (nx, ny, nz)
    twin = Twin(v0, e1, e2, box_min, box_max)             # the 48-B triangle records in global-id order, the unpadded scene box
    ans = twin.answer(grid, band)                         # distance / prim [nz, ny, nx] (unsigned), inside [nz, ny, nx], crossings [nz, ny]
    signed(ans.distance, ans.inside)                      # the signed grid: inside flips the sign bit

Distances come through closest_point_ref.Twin on the grid's points (4.8 with radius = band).  The rows restate the Moeller-Trumbore test
of 4.2 and the far-origin rule (multihit_ref.Twin.rebase) on the rays o = p(0, j, k), d = (1, 0, 0), tmin = 0, tmax = +inf and keep EVERY
hit (multihit_ref.Lists keeps 17 columns).  The triangles come from the scene description (closest_point_ref.scene_triangles) or from
hala_rt_download_bvh after an edit (closest_point_ref.bvh_triangles).  winding_inside is the float64 generalised winding number."""
import numpy as np

import closest_point_ref as CR
import hala_renderer_amd as H
from aov_ref import cross, dot, fma

f32, f64 = np.float32, np.float64
A = H._abi
MISS = 0xFFFFFFFF
REBASE_K = f32(16.0)  # RENDER_SPEC 4.2
JITTER = (0.0137, 0.0071, -0.0093)  # of a spacing: no row runs through a vertex


class Grid:
    def __init__(self, origin, spacing, dims):
        self.origin = np.asarray(origin, dtype=f32)
        self.spacing = f32(spacing)
        self.dims = tuple(int(d) for d in dims)

    def axis(self, a):
        """p.a = fma((float)i, spacing, origin.a)"""
        return fma(np.arange(self.dims[a]).astype(f32), self.spacing, self.origin[a]).astype(f32)

    def points(self):
        """[nz * ny * nx, 3], x fastest"""
        x, y, z = self.axis(0), self.axis(1), self.axis(2)
        zz, yy, xx = np.meshgrid(z, y, x, indexing="ij")
        return np.stack([xx.ravel(), yy.ravel(), zz.ravel()], axis=1).astype(f32)

    def kwargs(self):
        return dict(origin=self.origin, spacing=self.spacing, dims=self.dims)


def grid_over(mn, mx, dims, width=1.3, lead=None):
    """a grid of `dims` voxels centred on the box [mn, mx] and `width` boxes wide along its longest axis (the first of them), its origin
    jittered; lead: voxel 0 stands that many boxes before the box along x instead"""
    mn, mx = np.asarray(mn, f64), np.asarray(mx, f64)
    ext, c = mx - mn, 0.5 * (mn + mx)
    a = int(np.argmax(dims))
    spacing = f32(width * ext[a] / (dims[a] - 1) if dims[a] > 1 else width * ext.max())
    origin = c - 0.5 * (np.asarray(dims, f64) - 1.0) * f64(spacing)
    if lead is not None:
        origin[0] = mn[0] - lead * ext[0]
    return Grid((origin + np.asarray(JITTER) * f64(spacing)).astype(f32), spacing, dims)


def far_grid(mn, mx, dims=(8, 2, 2)):
    """origin.x at 40 amax on the -x side and a spacing that takes the rows through the scene; row (0, 0) runs through the box, the others
    pass it at one (huge) spacing: the far-origin rule on every row, and points far from every triangle"""
    mn, mx = np.asarray(mn, f64), np.asarray(mx, f64)
    amax = max(np.abs(mn).max(), np.abs(mx).max())
    ext, c = mx - mn, 0.5 * (mn + mx)
    x0 = -40.0 * amax
    spacing = f32((mx[0] + 0.15 * ext[0] - x0) / (dims[0] - 1.5))
    origin = np.array([x0, c[1] - 0.2 * ext[1], c[2] + 0.1 * ext[2]]) + np.asarray(JITTER) * f64(spacing)
    return Grid(origin.astype(f32), spacing, dims)


def signed(distance, inside):
    d = np.ascontiguousarray(distance, dtype=f32).view(np.uint32) ^ (inside.astype(np.uint32) << np.uint32(31))
    return d.view(f32)


def _safe_inv(d):
    dd = np.where(np.abs(d) < f32(1e-20), np.copysign(f32(1e-20), d), d).astype(f32)
    return (f32(1.0) / dd).astype(f32)


class Answer:
    """distance, prim: the unsigned grid [nz, ny, nx]; inside: bool [nz, ny, nx]; crossings: hits per row [nz, ny]; by_band: voxels the band
    answered; ties: voxels whose least dd two or more triangles share; m: per row the sorted bit indices of its hits (a list of arrays)"""
    def __init__(self, **kw):
        self.__dict__.update(kw)


class Twin:
    def __init__(self, v0, e1, e2, box_min, box_max):
        self.v0, self.e1, self.e2 = (np.ascontiguousarray(x, dtype=f32) for x in (v0, e1, e2))
        self.points = CR.Twin(self.v0, self.e1, self.e2)
        self.box_min, self.box_max = np.asarray(box_min, f32), np.asarray(box_max, f32)
        self.far_limit = REBASE_K * f32(max(np.abs(self.box_min).max(), np.abs(self.box_max).max()))
        ext = (self.box_max - self.box_min).astype(f32)
        self.diag = f32(np.sqrt(dot(ext, ext)))

    def rebase(self, o, d):
        """RENDER_SPEC 4.2, far origins, for rays with tmin = 0, tmax = +inf: (o', ts)"""
        o = o.copy()
        far = np.abs(o).max(axis=1) > self.far_limit
        ts = np.zeros(len(o), f32)
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
                ts[far] = s
        return o, ts, far

    def rows(self, grid, chunk=64):
        """inside [nz, ny, nx], crossings [nz, ny], the bit indices of every row, which rows were far"""
        nx, ny, nz = grid.dims
        y, z = grid.axis(1), grid.axis(2)
        x0 = fma(f32(0.0), grid.spacing, grid.origin[0])
        o_all = np.stack([np.full(ny * nz, x0, f32), np.tile(y, nz), np.repeat(z, ny)], axis=1).astype(f32)  # row = k * ny + j
        d_all = np.broadcast_to(np.array([1.0, 0.0, 0.0], f32), o_all.shape).copy()
        o_all, ts, far = self.rebase(o_all, d_all)
        t_i = (np.arange(nx).astype(f32) * grid.spacing).astype(f32)  # one product
        T = len(self.v0)
        inside = np.zeros((ny * nz, nx), bool)
        crossings = np.zeros(ny * nz, np.int64)
        ms = []
        E1, E2, V0 = self.e1[None], self.e2[None], self.v0[None]
        with np.errstate(all="ignore"):
            for a in range(0, ny * nz, chunk):
                o, d = o_all[a:a + chunk], d_all[a:a + chunk]
                m = len(o)
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
                ok &= (t > f32(0.0)) & (t < f32(np.inf))  # tmin' = 0, tmax' = +inf - ts
                rep = (t + ts[a:a + m, None]).astype(f32)  # reported: t' + ts
                for i in range(m):
                    bit = np.sort(np.searchsorted(t_i, rep[i][ok[i]], side="left"))  # #{i < nx : t_i < t}
                    ms.append(bit)
                    crossings[a + i] = len(bit)
                    hist = np.bincount(bit, minlength=nx + 1)
                    above = hist[::-1].cumsum()[::-1]  # hits with m >= b
                    inside[a + i] = (above[1:] % 2) == 1  # voxel i: hits with m > i
        return inside.reshape(nz, ny, nx), crossings.reshape(nz, ny), ms, far

    def answer(self, grid, band):
        nx, ny, nz = grid.dims
        q = np.empty(nx * ny * nz, dtype=A.POINT_QUERY_DTYPE)
        q["point"] = grid.points(); q["radius"] = f32(band)
        ans = self.points.answer(q)
        hit = ans.rec["prim"] != MISS
        distance = np.where(hit, ans.rec["distance"], f32(band)).astype(f32).reshape(nz, ny, nx)
        prim = ans.rec["prim"].reshape(nz, ny, nx).copy()
        inside, crossings, ms, far = self.rows(grid)
        return Answer(distance=distance, prim=prim, inside=inside, crossings=crossings, m=ms, far_rows=far, by_band=(~hit).reshape(nz, ny, nx),
                      ties=(ans.ties & hit).reshape(nz, ny, nx))


# ---- float64: the generalised winding number (Van Oosterom-Strackee solid angles) -----------------------------------------------------
def winding_number(v0, e1, e2, points, chunk=256):
    """w(p) = sum over triangles of the signed solid angle / 4 pi, float64 on the float32 records"""
    a0, b0, c0 = v0.astype(f64), (v0.astype(f64) + e1.astype(f64)), (v0.astype(f64) + e2.astype(f64))
    out = np.empty(len(points), f64)
    for s in range(0, len(points), chunk):
        p = points[s:s + chunk].astype(f64)[:, None, :]
        a, b, c = a0[None] - p, b0[None] - p, c0[None] - p
        la, lb, lc = (np.linalg.norm(x, axis=-1) for x in (a, b, c))
        num = (a * np.cross(b, c)).sum(axis=-1)
        den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
        out[s:s + chunk] = (2.0 * np.arctan2(num, den)).sum(axis=1) / (4.0 * np.pi)
    return out


def rows_near_an_edge(v0, e1, e2, grid, margin=1e-4):
    """[nz, ny]: the row's line y = p.y, z = p.z passes within `margin` (barycentric) of an edge of some triangle, in float64"""
    nx, ny, nz = grid.dims
    y, z = grid.axis(1).astype(f64), grid.axis(2).astype(f64)
    V0, E1, E2 = v0.astype(f64), e1.astype(f64), e2.astype(f64)
    # d = (1, 0, 0): p = cross(d, e2) = (0, -e2.z, e2.y); the barycentrics do not depend on o.x
    det = -E1[:, 1] * E2[:, 2] + E1[:, 2] * E2[:, 1]
    near = np.zeros((nz, ny), bool)
    with np.errstate(all="ignore"):
        for k in range(nz):
            for j in range(ny):
                ty, tz = y[j] - V0[:, 1], z[k] - V0[:, 2]
                u = (-ty * E2[:, 2] + tz * E2[:, 1]) / det
                v = (ty * E1[:, 2] - tz * E1[:, 1]) / det
                w = 1.0 - u - v
                lo = np.minimum(np.minimum(u, v), w)
                near[k, j] = bool(((lo > -margin) & (lo < margin) & (det != 0.0)).any())
    return near
