"""Brute-force references of closest-point queries (docs/RENDER_SPEC.md 4.8) over all triangles of a scene.

    twin = Twin(v0, e1, e2)            # the 48-B triangle records (RENDER_SPEC 3) in global-id order, float32 [T, 3] each
    ans = twin.answer(queries)         # the float32 twin of 4.8, operation for operation: records of A.CLOSEST_POINT_DTYPE and flags
    ref = twin.float64(queries, prim)  # the same regions in float64: the least distance over all triangles, and the distance to `prim`

The float32 twin uses the fma and dot of aov_ref (RENDER_SPEC 2.1); nothing else is fused.  The triangles come from the scene
description through multihit_ref.Twin (the flattening arithmetic of RENDER_SPEC 3), or from a downloaded tree (bvh_triangles)."""
import numpy as np

import hala_renderer_amd as H
from aov_ref import dot, fma

f32, f64 = np.float32, np.float64
A = H._abi
MISS = 0xFFFFFFFF
REGION_NAMES = ("face", "AB", "AC", "BC", "A", "B", "C")


def scene_triangles(scene, osc):
    """(v0, e1, e2) of the flattened scene, global-id order"""
    import multihit_ref as MR
    t = MR.Twin(scene, osc, False)
    return t.v0, t.e1, t.e2


def bvh_triangles(tris_words):
    """(v0, e1, e2) from the triangle words of hala_rt_download_bvh (12 words each, BVH order, word 3 = global id), global-id order"""
    w = np.asarray(tris_words, dtype=np.uint32).reshape(-1, 12)
    order = np.argsort(w[:, 3], kind="stable")
    assert np.array_equal(w[order, 3], np.arange(len(w), dtype=np.uint32)), "a one-level tree stores every triangle once"
    f = w[order].view(f32)
    return f[:, 0:3].copy(), f[:, 4:7].copy(), f[:, 8:11].copy()


def _regions(d1, d2, d3, d4, d5, d6, one, zero):
    """the region tests of 4.8 in the spec's order, in the dtype of the inputs: (u, v, region)"""
    with np.errstate(all="ignore"):
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        bc0, bc1 = d4 - d3, d5 - d6
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (d6 >= 0) & (d5 <= d6),
                 (vc <= 0) & (d1 >= 0) & (d3 <= 0), (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (bc0 >= 0) & (bc1 >= 0)]
        v_bc = bc0 / (bc0 + bc1)
        den = one / ((va + vb) + vc)
        us = [zero, one, zero, d1 / (d1 - d3), zero, one - v_bc]
        vs = [zero, zero, one, zero, d2 / (d2 - d6), v_bc]
        u = np.select(conds, us, vb * den)
        v = np.select(conds, vs, vc * den)
        region = np.select(conds, [4, 5, 6, 1, 2, 3], 0).astype(np.uint32)
    return u, v, region


class Answer:
    """rec: the records; ties: the least dd is shared by two or more admitted triangles; by_radius: a miss that radius = +inf answers;
    free_distance, free_prim: the answer of the same point without a limit (what the float64 comparison looks at: no query is left out)"""
    def __init__(self, rec, ties, by_radius, free_distance, free_prim):
        self.rec, self.ties, self.by_radius, self.free_distance, self.free_prim = rec, ties, by_radius, free_distance, free_prim


class Twin:
    def __init__(self, v0, e1, e2):
        self.v0, self.e1, self.e2 = (np.ascontiguousarray(x, dtype=f32) for x in (v0, e1, e2))

    def answer(self, queries, chunk=192):
        q = np.ascontiguousarray(queries, dtype=A.POINT_QUERY_DTYPE)
        n, T = len(q), len(self.v0)
        rec = np.zeros(n, dtype=A.CLOSEST_POINT_DTYPE)
        rec["distance"] = -1.0; rec["prim"] = MISS
        ties = np.zeros(n, bool); by_radius = np.zeros(n, bool)
        free_distance = np.full(n, -1.0, f32); free_prim = np.full(n, MISS, np.uint32)
        V0, E1, E2 = self.v0[None], self.e1[None], self.e2[None]
        one, zero = f32(1.0), f32(0.0)
        with np.errstate(all="ignore"):
            for a in range(0, n, chunk):
                p = q["point"][a:a + chunk].astype(f32)
                rad = q["radius"][a:a + chunk].astype(f32)
                m = len(p)
                e1, e2 = np.broadcast_to(E1, (m, T, 3)), np.broadcast_to(E2, (m, T, 3))
                ap = (p[:, None, :] - V0).astype(f32)
                bp = (ap - E1).astype(f32)
                cp = (ap - E2).astype(f32)
                d1, d2, d3, d4, d5, d6 = dot(e1, ap), dot(e2, ap), dot(e1, bp), dot(e2, bp), dot(e1, cp), dot(e2, cp)
                u, v, region = _regions(d1, d2, d3, d4, d5, d6, one, zero)
                u = u.astype(f32); v = v.astype(f32)
                qp = fma(v[..., None], e2, fma(u[..., None], e1, np.broadcast_to(V0, (m, T, 3))))
                r = (p[:, None, :] - qp).astype(f32)
                dd = dot(r, r)
                r2 = np.where(rad >= 0, (rad * rad).astype(f32), f32(-1.0))  # a NaN or negative radius admits nothing
                ok = dd <= r2[:, None]  # a NaN dd fails
                key = np.where(ok, dd, f32(np.inf))
                best = np.argmin(key, axis=1)  # the first least one: ties go to the lower id
                first_ok = np.argmax(ok, axis=1)
                rows = np.arange(m)
                best = np.where(ok[rows, best], best, first_ok)  # (only dd = +inf under an unlimited radius gets here)
                found = ok.any(axis=1)
                bdd = dd[rows, best]
                ties[a:a + m] = found & ((ok & (dd == bdd[:, None])).sum(axis=1) >= 2)
                by_radius[a:a + m] = ~found & (dd == dd).any(axis=1) & (rad >= 0)
                fkey = np.where(dd == dd, dd, f32(np.inf))
                fbest = np.argmin(fkey, axis=1)
                fok = (dd == dd)[rows, fbest]
                free_distance[a:a + m] = np.where(fok, np.sqrt(dd[rows, fbest]).astype(f32), f32(-1.0))
                free_prim[a:a + m] = np.where(fok, fbest.astype(np.uint32), np.uint32(MISS))
                out = rec[a:a + m]
                out["distance"] = np.where(found, np.sqrt(bdd).astype(f32), f32(-1.0))
                out["u"] = np.where(found, u[rows, best], zero)
                out["v"] = np.where(found, v[rows, best], zero)
                out["prim"] = np.where(found, best.astype(np.uint32), np.uint32(MISS))
                out["point"] = np.where(found[:, None], qp[rows, best], zero)
                out["region"] = np.where(found, region[rows, best], np.uint32(0))
                rec[a:a + m] = out
        return Answer(rec, ties, by_radius, free_distance, free_prim)

    def float64(self, queries, prim, chunk=512):
        """(the least float64 distance over all triangles, the float64 distance to triangle prim[i]; NaN where prim is a miss): the regions
        of 4.8 on the float32 records, every operation in float64; the radius plays no part"""
        q = np.ascontiguousarray(queries, dtype=A.POINT_QUERY_DTYPE)
        n = len(q)
        V0, E1, E2 = (x[None].astype(f64) for x in (self.v0, self.e1, self.e2))
        least = np.empty(n, f64); to_prim = np.full(n, np.nan, f64)
        prim = np.asarray(prim)
        with np.errstate(all="ignore"):
            for a in range(0, n, chunk):
                p = q["point"][a:a + chunk].astype(f64)[:, None, :]
                ap = p - V0; bp = ap - E1; cp = ap - E2
                s = lambda x, y: (x * y).sum(axis=-1)  # noqa: E731
                u, v, _ = _regions(s(E1, ap), s(E2, ap), s(E1, bp), s(E2, bp), s(E1, cp), s(E2, cp), 1.0, 0.0)
                r = p - (V0 + u[..., None] * E1 + v[..., None] * E2)
                d = np.sqrt(s(r, r))
                d = np.where(d == d, d, np.inf)  # degenerate triangles
                least[a:a + chunk] = d.min(axis=1)
                pr = prim[a:a + chunk]
                hit = pr != MISS
                rows = np.nonzero(hit)[0]
                to_prim[a + rows] = d[rows, pr[hit].astype(np.int64)]
        return least, to_prim


# ---- query sets (RENDER_SPEC 4.8; tests/test_closest_points.py, scripts/closest_point_timing.py) ---------------------------------------
def bounds_of(v0, e1, e2):
    pts = np.concatenate([v0, (v0 + e1).astype(f32), (v0 + e2).astype(f32)]).astype(f64)
    return pts.min(axis=0), pts.max(axis=0)


def surface_points(v0, e1, e2, n, rng):
    t = rng.randint(0, len(v0), n)
    a, b = rng.rand(n), rng.rand(n)
    flip = a + b > 1.0
    a, b = np.where(flip, 1.0 - a, a), np.where(flip, 1.0 - b, b)
    return (v0[t].astype(f64) + a[:, None] * e1[t] + b[:, None] * e2[t]).astype(f32), t


def point_sets(v0, e1, e2, seed, sizes=(700, 600, 900, 1200, 300, 300)):
    """the point sets of the issue, in order: on the surface; exact vertices and edge midpoints; offset along face normals by 1e-4 ... 1
    diagonal on both sides; uniform in twice the box; at 10^2 and at 10^4 diagonals.  Returns (points float32 [n, 3], the index ranges)"""
    rng = np.random.RandomState(seed)
    mn, mx = bounds_of(v0, e1, e2)
    c, ext = 0.5 * (mn + mx), mx - mn
    diag = float(np.linalg.norm(ext))
    sets = []
    sets.append(surface_points(v0, e1, e2, sizes[0], rng)[0])
    t = rng.randint(0, len(v0), sizes[1])
    half = (v0[t] + f32(0.5) * e1[t]).astype(f32)
    sets.append(np.where((np.arange(sizes[1]) % 2 == 0)[:, None], v0[t], half).astype(f32))
    base, t = surface_points(v0, e1, e2, sizes[2], rng)
    nrm = np.cross(e1[t].astype(f64), e2[t].astype(f64))
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
    off = diag * 10.0 ** rng.uniform(-4.0, 0.0, sizes[2]) * rng.choice([-1.0, 1.0], sizes[2])
    sets.append((base.astype(f64) + nrm * off[:, None]).astype(f32))
    sets.append((c + (rng.rand(sizes[3], 3) - 0.5) * 2.0 * ext).astype(f32))
    for k, decade in ((4, 2.0), (5, 4.0)):
        d = rng.randn(sizes[k], 3); d /= np.linalg.norm(d, axis=1, keepdims=True)
        sets.append((c + d * diag * 10.0 ** decade).astype(f32))
    ends = np.cumsum([len(s) for s in sets])
    return np.concatenate(sets), [slice(int(e - len(s)), int(e)) for s, e in zip(sets, ends)], diag


def with_radii(points, diag, seed):
    """queries over `points`: half of them unlimited (+inf, FLT_MAX), the others with radii of 10 %, 1 % of the diagonal, 0, NaN and -1,
    dealt out at random"""
    rng = np.random.RandomState(seed)
    choices = np.array([np.inf, np.inf, np.inf, np.inf, 3.402823466e38, 0.1 * diag, 0.1 * diag, 0.01 * diag, 0.0, np.nan, -1.0, 0.01 * diag])
    q = np.empty(len(points), dtype=A.POINT_QUERY_DTYPE)
    q["point"] = points
    with np.errstate(all="ignore"):
        q["radius"] = choices[rng.randint(0, len(choices), len(points))].astype(f32)
    return q
