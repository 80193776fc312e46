"""Rays and scenes outside the comfortable regime (docs/RENDER_SPEC.md 4.1, 4.1b, 4.2 "far origins"), shared by the CPU tier
(tests/test_ray_conditioning.py: the oracle against ground truth) and the GPU tier (tests/test_gpu_ray_conditioning.py: the kernels against the
oracle).  Everything is seeded; nothing here traces a ray but float64_truth, the plain numpy reference.
"""
import copy
import math

import numpy as np

import hala_renderer_amd as H
from hala_renderer_amd import scenes

f32 = np.float32
MISS = 0xFFFFFFFF
N_RAYS = 20000  # per family, CPU tier
K = 16.0  # RENDER_SPEC 4.2: origins beyond K x the scene's largest absolute coordinate are re-based

# (scale, offset) of the scene's geometry: the regimes in which the oracle's trees and brute force were found to agree
TRANSFORMS = [(1e-4, (0.0, 0.0, 0.0)), (1e5, (0.0, 0.0, 0.0)), (1.0, (1e4, 1e4, 1e4)), (1.0, (1e5, -1e5, 1e5)), (1.0, (1e6, 1e6, 1e6)),
              (1e-3, (100.0, 100.0, 100.0)), (1.0, (0.0, 0.0, 0.0))]
FAR_DECADES = (1, 2, 3, 4, 5, 6)  # origins at 10^k scene diagonals


def transform_id(t):
    return f"s{t[0]:g}_o{t[1][0]:g}_{t[1][1]:g}_{t[1][2]:g}"


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def blob_scene(subdivisions=3):
    """the displaced icosphere alone: 20 * 4^s triangles (s = 3: 1280, a tree above the 40-KB threshold of RENDER_SPEC 4.4b)"""
    s = H.HalaScene()
    s.materials = [H.HalaMaterial(type=0, base_color=(0.8, 0.6, 0.4))]
    blob = scenes.blob_mesh(subdivisions); blob.material_index = 0
    s.meshes = [H.HalaMesh([blob])]
    s.nodes = [H.HalaNode(name="blob", mesh_index=0),
               H.HalaNode(name="camera", camera_index=0, local_transform=scenes.look_at_node_transform((0.0, 0.6, 4.2), (0.0, 0.0, 0.0)))]
    s.cameras = [H.HalaPerspectiveCamera(aspect=1.0, yfov=math.radians(40.0), znear=0.1)]
    return s


def placed(scene, scale, offset):
    """a copy of `scene` with every mesh node (all of them roots) scaled and moved; the camera node moves with them and keeps its axes"""
    s = copy.copy(scene)
    s.nodes = []
    t = np.eye(4, dtype=np.float64)
    t[:3, :3] *= scale
    t[:3, 3] = offset
    for nd in scene.nodes:
        assert nd.parent is None
        m = np.asarray(nd.local_transform, dtype=np.float64)
        if nd.mesh_index != H._abi.INVALID_INDEX:
            m = t @ m
        elif nd.camera_index != H._abi.INVALID_INDEX:
            m = m.copy(); m[:3, 3] = scale * m[:3, 3] + np.asarray(offset)
        s.nodes.append(H.HalaNode(name=nd.name, local_transform=m.astype(f32), mesh_index=nd.mesh_index, camera_index=nd.camera_index,
                                  light_index=nd.light_index))
    return s


def tiny_on_huge():
    """a 1e-3-sized blob standing on a 2000-unit ground quad: the pad and the node quanta follow the ground, the hits are on the blob"""
    s = blob_scene(3)
    ground = scenes._merge_quads([((-1000, 0, 1000), (1000, 0, 1000), (1000, 0, -1000), (-1000, 0, -1000))]); ground.material_index = 0
    s.meshes.append(H.HalaMesh([ground]))
    m = np.eye(4, dtype=f32); m[:3, :3] *= 0.5e-3; m[:3, 3] = (0.3, 0.7e-3, -0.2)
    s.nodes[0] = H.HalaNode(name="blob", mesh_index=0, local_transform=m)
    s.nodes.append(H.HalaNode(name="ground", mesh_index=1))
    return s


def tiny_on_huge_rays(n, seed):
    """half of the rays start within a few blob sizes of the blob, half anywhere over the ground; all aim at the blob's box"""
    rng = np.random.RandomState(seed)
    c = np.array([0.3, 0.7e-3, -0.2]); r = 0.7e-3
    near = c + rng.uniform(-4, 4, (n // 2, 3)) * r
    wide = np.stack([rng.uniform(-1000, 1000, n - n // 2), rng.uniform(0.0, 500.0, n - n // 2), rng.uniform(-1000, 1000, n - n // 2)], 1)
    o = np.concatenate([near, wide]).astype(f32)
    target = c + rng.uniform(-1, 1, (n, 3)) * r
    return _rays(o, target - o.astype(np.float64))


# one shared primitive (the blob, radius about 1.3), instanced: as it is, tiny, huge, mirrored, and far from the origin
INSTANCES = [((1.0, 1.0, 1.0), (0.0, 0.0, 0.0)), ((1e-3, 1e-3, 1e-3), (2.5, 0.5, 0.0)), ((1e3, 1e3, 1e3), (0.0, 0.0, -4000.0)),
             ((-1.0, 1.0, 1.0), (4.0, 0.0, 1.0)), ((1.0, 1.0, 1.0), (1e4, 0.0, 0.0))]


def instanced_extremes():
    s = blob_scene(3)
    cam = s.nodes[1]
    s.nodes = []
    for k, (sc, off) in enumerate(INSTANCES):
        m = np.eye(4, dtype=f32)
        m[0, 0], m[1, 1], m[2, 2] = sc
        m[:3, 3] = off
        s.nodes.append(H.HalaNode(name=f"blob_{k}", mesh_index=0, local_transform=m))
    s.nodes.append(cam)
    return s


def instance_aimed_rays(scene, n, seed):
    """rays aimed at the instances of instanced_extremes (or of an edited copy: the nodes' transforms are read), each from a few instance sizes away"""
    rng = np.random.RandomState(seed)
    mesh_nodes = [nd for nd in scene.nodes if nd.mesh_index != H._abi.INVALID_INDEX]
    which = rng.randint(0, len(mesh_nodes), n)
    size = np.array([abs(float(np.asarray(nd.local_transform)[0, 0])) for nd in mesh_nodes])[which, None]
    centre = np.array([np.asarray(nd.local_transform, dtype=np.float64)[:3, 3] for nd in mesh_nodes])[which]
    u = rng.randn(n, 3); u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = (centre + u * size * rng.uniform(2.0, 6.0, (n, 1))).astype(f32)
    target = centre + rng.uniform(-1.0, 1.0, (n, 3)) * size
    return _rays(o, target - o.astype(np.float64))


# ---- ray families ---------------------------------------------------------------------------------------------------------------
def _rays(o, d, tmax=None):
    rays = np.zeros(len(o), dtype=H._abi.RAY_DTYPE)
    rays["origin"] = np.asarray(o, dtype=f32)
    d = np.asarray(d, dtype=np.float64)
    rays["direction"] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    rays["tmin"] = 0.0
    rays["tmax"] = 3.0e38 if tmax is None else np.asarray(tmax, dtype=f32)
    return rays


def near_rays(mn, mx, n, seed):
    """origins inside the scene box padded by a quarter, any direction; three in ten with a limit inside the scene"""
    rng = np.random.RandomState(seed)
    mn = mn.astype(np.float64); mx = mx.astype(np.float64)
    pad = (mx - mn) * 0.25
    o = (mn - pad) + rng.rand(n, 3) * (mx - mn + 2 * pad)
    tmax = np.where(rng.rand(n) < 0.3, rng.rand(n) * np.linalg.norm(mx - mn), 3.0e38)
    return _rays(o, rng.randn(n, 3), tmax)


def far_rays(mn, mx, decade, n, seed, inner=1.0):
    """origins on the sphere of radius 10^decade scene diagonals around the box centre, aimed at random points of the box (of its
    central part, `inner` < 1); three in ten with a limit within a diagonal of the target"""
    rng = np.random.RandomState(seed)
    mn = mn.astype(np.float64); mx = mx.astype(np.float64)
    c = 0.5 * (mn + mx); diag = np.linalg.norm(mx - mn)
    u = rng.randn(n, 3); u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = (c + u * diag * 10.0 ** decade).astype(f32)
    target = c + (rng.rand(n, 3) - 0.5) * (mx - mn) * inner
    d = target - o.astype(np.float64)
    dist = np.linalg.norm(d, axis=1)
    tmax = np.where(rng.rand(n) < 0.3, dist + rng.uniform(-1, 1, n) * diag, 3.0e38)
    return _rays(o, d, tmax)


def near_axis_rays(mn, mx, n, seed):
    """near rays with one direction component scaled by 1e-7 ... 1e-2 (then normalised): slab distances of 1e2 ... 1e7 box sizes"""
    rng = np.random.RandomState(seed)
    rays = near_rays(mn, mx, n, seed + 1)
    d = rays["direction"].astype(np.float64)
    d[np.arange(n), rng.randint(0, 3, n)] *= 10.0 ** rng.uniform(-7, -2, n)
    rays["direction"] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    return rays


def lattice_rays(tris9, n, seed):
    """exactly axis-aligned rays whose origin components are vertex coordinates of the scene: they start on vertices and edges and run
    inside the planes of axis-aligned faces"""
    rng = np.random.RandomState(seed)
    v = tris9.reshape(-1, 3)
    o = np.stack([v[rng.randint(0, len(v), n), k] for k in range(3)], 1)
    d = np.zeros((n, 3))
    d[np.arange(n), rng.randint(0, 3, n)] = rng.choice([-1.0, 1.0], n)
    return _rays(o, d)


def max_origin_ratio(rays, mn, mx):
    """max |o_a| over the scene's largest absolute coordinate: the quantity the far-origin rule of RENDER_SPEC 4.2 compares with K"""
    return float(np.abs(rays["origin"]).max() / max(np.abs(mn).max(), np.abs(mx).max()))


# ---- float64 ground truth -------------------------------------------------------------------------------------------------------
def float64_truth(tris9, rays, margin=1e-4, chunk=2048):
    """Möller–Trumbore in float64 over all triangles, on the float32 rays as given, no tree: (prim [n], ambiguous [n]).  prim = the
    triangle of the closest hit inside (tmin, tmax), MISS if none.  ambiguous, either of:
    - some triangle whose plane the ray reaches has its smallest barycentric margin |min(u, v, 1 - u - v)| below `margin`: the ray passes
      within that of an edge, where a float32 test may legitimately decide either way;
    - the two nearest hits lie within 2^-20 scene diagonals of each other in t (the ray passes through the line in which two surfaces
      cross, as the sheets of stacked_sheets do): a float32 t computed from coordinates of the size of the scene carries a few ulp of
      that size, 2^-20 diagonals are 4 ulp of a number between one and two diagonals — which of the two is nearer is below the format"""
    t9 = tris9.astype(np.float64)
    v0, e1, e2 = t9[:, 0:3], t9[:, 3:6] - t9[:, 0:3], t9[:, 6:9] - t9[:, 0:3]
    allv = t9.reshape(-1, 3)
    tie = float(np.linalg.norm(allv.max(0) - allv.min(0))) * 2.0 ** -20
    n = len(rays)
    prim = np.full(n, MISS, dtype=np.uint32)
    amb = np.zeros(n, dtype=bool)
    for a in range(0, n, chunk):
        r = rays[a:a + chunk]
        o = r["origin"].astype(np.float64)[:, None, :]; d = r["direction"].astype(np.float64)[:, None, :]
        p = np.cross(d, e2[None])
        det = (e1[None] * p).sum(-1)
        ok = det != 0.0
        inv = 1.0 / np.where(ok, det, 1.0)
        tv = o - v0[None]
        u = (tv * p).sum(-1) * inv
        q = np.cross(tv, e1[None])
        v = (d * q).sum(-1) * inv
        t = (e2[None] * q).sum(-1) * inv
        w = 1.0 - u - v
        lo = np.minimum(np.minimum(u, v), w)
        reach = ok & (t > r["tmin"].astype(np.float64)[:, None]) & (t < r["tmax"].astype(np.float64)[:, None])
        amb[a:a + chunk] = (reach & (np.abs(lo) < margin)).any(1)
        hit = reach & (lo >= 0.0)
        tt = np.where(hit, t, np.inf)
        k = tt.argmin(1)
        first = tt[np.arange(len(r)), k]
        prim[a:a + chunk] = np.where(np.isfinite(first), k, MISS).astype(np.uint32)
        if tt.shape[1] > 1:
            second = np.partition(tt, 1, axis=1)[:, 1]
            amb[a:a + chunk] |= np.isfinite(second) & (np.where(np.isfinite(second), second, 0.0) - np.where(np.isfinite(first), first, 0.0) < tie)
    return prim, amb
