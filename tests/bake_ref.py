"""The float32 numpy twin of bake maps (docs/RENDER_SPEC.md 4.11), operation for operation, by brute force: every triangle of the instance
against every texel of the map.

    twin = Twin(scene, osc)                                   # the triangle and shading records of the flattened scene
    owner = twin.owners(instance, W, H)                       # [H * W] uint32: the lowest covering global id, MISS: none
    samples, texels = twin.samples(instance, W, H, ...)       # A.OCCLUSION_SAMPLE_DTYPE and A.BAKE_TEXEL_DTYPE, [H * W] each
    rec, texels = dilate(rec, texels, W, H, margin)           # the dilation of the occlusion records of those samples
    owner64 = twin.owners64(instance, W, H)                   # the same rule with float64 edge values on the float32 UVs

The triangle records (v0, e1, e2) are closest_point_ref's (the flattening arithmetic of RENDER_SPEC 3), the world transforms the oracle's
(`oracle_lib.world_transforms`, as occlusion_ref takes its sincos from it); fma, dot and cross are aov_ref's (RENDER_SPEC 2.1).  Nothing
else is fused: numpy rounds every float32 operation on its own.  The occlusion records are not made here: they are occlusion_ref's
reduction of an any-hit trace of the twin's samples, as tests/test_occlusion.py gets them."""
import numpy as np

import closest_point_ref as CR
import hala_renderer_amd as H
import oracle_lib as O
from aov_ref import cross, dot, fma

f32, f64 = np.float32, np.float64
A = H._abi
MISS = 0xFFFFFFFF
SHADING_NORMAL, FLIP_NORMAL = 1, 2


def edge_raw(ax, ay, bx, by, px, py):
    """E(a, b, p): every difference and product rounded, one subtraction, no fma (the operands' dtype decides the precision)"""
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def edge(ax, ay, bx, by, px, py):
    """E with the endpoints in canonical order: -E(b, a, p) where (a.x, a.y) > (b.x, b.y), comparing x, then y"""
    with np.errstate(all="ignore"):
        swap = (ax > bx) | ((ax == bx) & (ay > by))
        return np.where(swap, -edge_raw(bx, by, ax, ay, px, py), edge_raw(ax, ay, bx, by, px, py))


def covers(area, w0, w1, w2):
    with np.errstate(invalid="ignore"):
        return ((area > 0) & (w0 >= 0) & (w1 >= 0) & (w2 >= 0)) | ((area < 0) & (w0 <= 0) & (w1 <= 0) & (w2 <= 0))


def centres(W, H, dt=f32):
    """texel centres in texel units, index y * W + x"""
    y, x = np.divmod(np.arange(W * H), W)
    return (x.astype(dt) + dt(0.5)), (y.astype(dt) + dt(0.5))


class Twin:
    def __init__(self, scene, osc):
        self.v0, self.e1, self.e2 = CR.scene_triangles(scene, osc)
        world = O.world_transforms(scene)
        uv, nrm, inst, first, xf = [], [], [], [0], []
        for k, nd in enumerate(scene.nodes):
            if nd.mesh_index == H.scene.INVALID:
                continue
            for pr in scene.meshes[nd.mesh_index].primitives:
                idx = np.asarray(pr.indices, dtype=np.int64)[: (len(pr.indices) // 3) * 3].reshape(-1, 3)
                uv.append(np.ascontiguousarray(pr.vertices["tex_coord"], dtype=f32)[idx])
                nrm.append(np.ascontiguousarray(pr.vertices["normal"], dtype=f32)[idx])
                inst.append(np.full(len(idx), len(xf), dtype=np.int64))
                xf.append(world[k].astype(f32))
                first.append(first[-1] + len(idx))
        self.uv = np.concatenate(uv) if uv else np.zeros((0, 3, 2), f32)      # [T, 3, 2]
        self.normals = np.concatenate(nrm) if nrm else np.zeros((0, 3, 3), f32)  # [T, 3, 3]
        self.inst = np.concatenate(inst) if inst else np.zeros(0, np.int64)
        self.first = np.array(first, dtype=np.int64)  # [instances + 1]
        self.transform = np.stack(xf) if xf else np.zeros((0, 16), f32)
        assert len(self.uv) == len(self.v0)

    def corners(self, ids, W, H, dt=f32):
        """the UV corners of triangles `ids` in texel units, one float32 product each (then widened to dt): ((ax, ay), (bx, by), (cx, cy))"""
        with np.errstate(all="ignore"):
            t = (self.uv[ids] * np.array([W, H], f32)).astype(f32).astype(dt)
        return [(t[:, c, 0], t[:, c, 1]) for c in range(3)]

    def edge_values(self, ids, W, H, px, py, dt=f32, pairwise=False):
        """(area, w0, w1, w2) of triangles `ids`: every triangle at every point (w [n, P]) or, pairwise, triangle k at point k (w [n])"""
        (ax, ay), (bx, by), (cx, cy) = self.corners(ids, W, H, dt)
        with np.errstate(all="ignore"):
            area = edge(ax, ay, bx, by, cx, cy)
            if not pairwise:
                ax, ay, bx, by, cx, cy = (z[:, None] for z in (ax, ay, bx, by, cx, cy))
                px, py = px[None, :], py[None, :]
            w0 = edge(bx, by, cx, cy, px, py)
            w1 = edge(cx, cy, ax, ay, px, py)
            w2 = edge(ax, ay, bx, by, px, py)
        return area, w0, w1, w2

    def _owners(self, instance, W, H, dt, chunk=512):
        lo, hi = int(self.first[instance]), int(self.first[instance + 1])
        px, py = centres(W, H, dt)
        owner = np.full(W * H, MISS, dtype=np.uint32)
        for a in range(lo, hi, chunk):
            ids = np.arange(a, min(a + chunk, hi))
            area, w0, w1, w2 = self.edge_values(ids, W, H, px, py, dt)
            cov = covers(area[:, None], w0, w1, w2)
            cand = np.where(cov, ids[:, None].astype(np.uint32), np.uint32(MISS)).min(axis=0)
            owner = np.minimum(owner, cand)
        return owner

    def owners(self, instance, W, H):
        """[H * W] uint32: the lowest global id among the instance's triangles that cover the texel's centre, MISS: none"""
        return self._owners(instance, W, H, f32)

    def owners64(self, instance, W, H):
        """the same rule with float64 edge values on the float32 corners (the corner products stay float32: they are the inputs)"""
        return self._owners(instance, W, H, f64)

    def at_owner(self, owner, W, H, dt=f32):
        """(area, w0, w1, w2) [P] of each texel's owner at the texel's centre (rows of ownerless texels hold triangle 0's or zeros)"""
        px, py = centres(W, H, dt)
        ids = np.where(owner == MISS, 0, owner).astype(np.int64)
        if len(self.uv) == 0:
            z = np.zeros(W * H, dt)
            return z, z, z, z
        return self.edge_values(ids, W, H, px, py, dt, pairwise=True)

    def samples(self, instance, W, H, flags=0, bias=0.0, reach=np.inf, owner=None):
        """(samples, texels) [H * W]: RENDER_SPEC 4.11's sample and texel record of every texel"""
        owner = self.owners(instance, W, H) if owner is None else owner
        owned = owner != MISS
        ids = np.where(owned, owner, 0).astype(np.int64)
        samples = np.zeros(W * H, dtype=A.OCCLUSION_SAMPLE_DTYPE)
        texels = np.zeros(W * H, dtype=A.BAKE_TEXEL_DTYPE)
        texels["prim"], texels["source"] = MISS, MISS
        if not owned.any():
            return samples, texels
        area, _, w1, w2 = self.at_owner(owner, W, H)
        with np.errstate(all="ignore"):
            inv = (f32(1.0) / area).astype(f32)
            u, v = (w1 * inv).astype(f32), (w2 * inv).astype(f32)
            v0, e1, e2 = self.v0[ids], self.e1[ids], self.e2[ids]
            point = fma(e2, v[:, None], fma(e1, u[:, None], v0))
            if flags & SHADING_NORMAL:
                n = self.shading_normal(ids, u, v)
            else:
                n = cross(e1, e2).astype(f32)
            if flags & FLIP_NORMAL:
                n = -n
        m = owned
        samples["point"][m], samples["normal"][m] = point[m], n[m]
        samples["bias"][m], samples["reach"][m] = f32(bias), f32(reach)
        texels["u"][m], texels["v"][m], texels["prim"][m] = u[m], v[m], owner[m]
        texels["source"][m] = np.nonzero(m)[0].astype(np.uint32)
        return samples, texels

    def shading_normal(self, ids, u, v):
        """RENDER_SPEC 6 step 4 ahead of the normal map and of any flip: normalize(transform_normal(M, n0 * w0 + n1 * u + n2 * v)) in the
        operation order of shading.h (make_surface, transform_normal)"""
        n0, n1, n2 = self.normals[ids, 0], self.normals[ids, 1], self.normals[ids, 2]
        w0 = ((f32(1.0) - u).astype(f32) - v).astype(f32)
        nl = fma(n2, v[:, None], fma(n1, u[:, None], (n0 * w0[:, None]).astype(f32)))
        m = self.transform[self.inst[ids]]
        c0, c1, c2 = m[:, 0:3], m[:, 4:7], m[:, 8:11]
        k0, k1, k2 = cross(c1, c2), cross(c2, c0), cross(c0, c1)
        det = dot(c0, k0)
        r = fma(k2, nl[:, 2:3], fma(k1, nl[:, 1:2], (k0 * nl[:, 0:1]).astype(f32)))
        r = np.where((det < 0)[:, None], -r, r).astype(f32)
        return (r * (f32(1.0) / np.sqrt(dot(r, r).astype(f32)))[:, None]).astype(f32)


def dilate(rec, texels, W, H, margin):
    """RENDER_SPEC 4.11, dilation: every ownerless texel takes the record of the owned texel with the least (dx^2 + dy^2, index) among those
    with |dx|, |dy| <= margin, and names it in `source`; integers throughout.  Returns copies."""
    rec, texels = rec.copy(), texels.copy()
    owned = (texels["prim"] != MISS).reshape(H, W)
    best = np.full((H, W), np.iinfo(np.int64).max, dtype=np.int64)
    ys, xs = np.mgrid[0:H, 0:W]
    for dy in range(-margin, margin + 1):
        for dx in range(-margin, margin + 1):
            sy, sx = ys + dy, xs + dx
            inside = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
            ok = inside & owned[np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)]
            key = np.int64(dx * dx + dy * dy) * np.int64(1 << 32) + (sy * W + sx)
            best = np.where(ok & (key < best), key, best)
    fill = (~owned & (best != np.iinfo(np.int64).max)).reshape(-1)
    src = (best.reshape(-1) & np.int64(0xFFFFFFFF)).astype(np.int64)
    rec[fill] = rec[src[fill]]
    texels["source"][fill] = src[fill].astype(np.uint32)
    return rec, texels
