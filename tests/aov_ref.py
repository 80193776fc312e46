"""numpy reference of the first-hit AOVs (docs/RENDER_SPEC.md 13): position (running mean of (P, hit)) and ids (node, instance,
material, triangle id of frame 0's first hit).  The camera rays and the nearest triangle hit come from the oracle (camera_rays, trace);
what is added here is the hittable-light test of the depth-0 shade (shading.h intersect_light), the fma of RENDER_SPEC 2.1 and the
instance / node / material tables derived from the scene description.

numpy has no fma.  fma(a, b, c) of float32 operands is emulated exactly: the product is exact in float64 (24 + 24 bits), the sum is
rounded to odd in float64 (TwoSum gives the error term), and the final rounding to float32 is then correct because 53 >= 24 + 2."""
import numpy as np

import hala_renderer_amd as H

f32, f64 = np.float32, np.float64
ABSENT = np.uint32(0xFFFFFFFF)
T_MAX = f32(3.402823466e38)
MAX_LIGHTS = 32  # HALA_MAX_LIGHT_COUNT


def fma(a, b, c):
    """float32 fma(a, b, c) with a single rounding (finite, non-overflowing operands)"""
    a, b, c = (np.asarray(x, dtype=f32) for x in (a, b, c))
    p = a.astype(f64) * b.astype(f64)  # exact
    cc = c.astype(f64)
    s = p + cc
    bp = s - cc
    e = (p - bp) + (cc - (s - bp))  # s + e == p + c exactly
    bits = np.atleast_1d(s).view(np.int64).copy()
    inexact = np.atleast_1d(e != 0.0) & ((bits & 1) == 0)
    # round to odd: an inexact even result moves one ulp towards the exact value
    toward = np.where(np.atleast_1d(e) > 0.0, np.inf, -np.inf)
    s_odd = np.where(inexact, np.nextafter(np.atleast_1d(s), toward), np.atleast_1d(s))
    return s_odd.astype(f32).reshape(np.shape(s))


def madd(d, t, o):
    return fma(d, t[..., None] if np.ndim(t) == np.ndim(d) - 1 else t, o)


def dot(a, b):
    return fma(a[..., 2], b[..., 2], fma(a[..., 1], b[..., 1], a[..., 0] * b[..., 0]))


def cross(a, b):
    def c(i, j):
        return fma(a[..., i], b[..., j], -(a[..., j] * b[..., i]))
    return np.stack([c(1, 2), c(2, 0), c(0, 1)], axis=-1)


def normalize(v):
    return v * (f32(1.0) / np.sqrt(dot(v, v)))[..., None]


def fold_mean(mean_old, x, frame_index):
    """RENDER_SPEC 8 (no fma)"""
    if frame_index == 0:
        return np.asarray(x, dtype=f32).copy()
    return ((mean_old * f32(frame_index) + x) / f32(frame_index + 1)).astype(f32)


def intersect_light(light, o, d):
    """shading.h intersect_light for rays o, d [N, 3] float32: t [N] (-1: no hit).  QUAD (type 3) and SPHERE (type 4) only."""
    pos = np.array(light.position[:3], dtype=f32)
    n_rays = o.shape[0]
    miss = np.full(n_rays, f32(-1.0), dtype=f32)
    with np.errstate(all="ignore"):
        if light.type == 3:
            u, v = np.array(light.u[:3], dtype=f32), np.array(light.v[:3], dtype=f32)
            n = normalize(cross(u, v))
            dn = dot(d, np.broadcast_to(n, d.shape))
            t = (dot(pos - o, np.broadcast_to(n, o.shape)) / dn).astype(f32)
            hp = madd(d, t, o) - pos
            a = dot(hp, np.broadcast_to(u, hp.shape)) / dot(u, u)
            b = dot(hp, np.broadcast_to(v, hp.shape)) / dot(v, v)
            ok = (dn < 0.0) & (t > 0.0) & (a >= 0.0) & (a <= 1.0) & (b >= 0.0) & (b <= 1.0)
            return np.where(ok, t, miss)
        if light.type == 4:
            r = f32(light.radius)
            oc = o - pos
            b = dot(oc, d)
            c = dot(oc, oc) - r * r
            disc = b * b - c
            t = (-b - np.sqrt(disc)).astype(f32)
            nl = (madd(d, t, o) - pos) * (f32(1.0) / r)
            cosl = -dot(d, nl)
            ok = (disc > 0.0) & (t > 0.0) & (cosl > 0.0)
            return np.where(ok, t, miss)
    return miss


def instance_table(scene):
    """per packed instance (node order, then primitive order: gpu_uploader.rs / hala_rt_get_packed_primitives): node index, material
    index, first global triangle id; plus the total triangle count"""
    node, material, first = [], [], []
    total = 0
    for k, nd in enumerate(scene.nodes):
        if nd.mesh_index == H.scene.INVALID:
            continue
        for p in scene.meshes[nd.mesh_index].primitives:
            node.append(k); material.append(p.material_index); first.append(total)
            total += len(p.indices) // 3
    return np.array(node, np.uint32), np.array(material, np.uint32), np.array(first + [total], np.uint64)


def light_nodes(scene):
    """per packed light (node order, at most 32): the node it came from"""
    return np.array([k for k, nd in enumerate(scene.nodes) if nd.light_index != H.scene.INVALID][:MAX_LIGHTS], np.uint32)


def first_hits(osc, scene, lights, w, h, frame):
    """(P.xyz, hit) float32 [H, W, 4] and ids uint32 [H, W, 4] of the first hit of frame `frame`'s camera ray (camera 0 of `osc`).
    lights: the packed lights (oracle_lib.pack_lights(scene)[0])."""
    rays = osc.camera_rays(w, h, frame)
    hits = osc.trace(rays, 0)
    o = np.ascontiguousarray(rays["origin"], dtype=f32)
    d = np.ascontiguousarray(rays["direction"], dtype=f32)
    prim = hits["prim"].astype(np.uint32)
    surf = prim != ABSENT
    t_light = np.where(surf, hits["t"].astype(f32), T_MAX)
    hit_light = np.full(prim.shape, -1, np.int64)
    for k, L in enumerate(lights):
        tl = intersect_light(L, o, d)
        closer = (tl > 0.0) & (tl < t_light)
        t_light = np.where(closer, tl, t_light)
        hit_light = np.where(closer, k, hit_light)
    is_light = hit_light >= 0
    is_tri = surf & ~is_light
    pos = np.zeros((prim.size, 4), f32)
    P = madd(d, t_light, o)
    pos[is_light | is_tri, :3] = P[is_light | is_tri]
    pos[is_light | is_tri, 3] = 1.0
    ids = np.full((prim.size, 4), ABSENT, np.uint32)
    inst_node, inst_mat, first = instance_table(scene)
    lnode = light_nodes(scene)
    inst = np.searchsorted(first[:-1], prim[is_tri].astype(np.uint64), side="right") - 1
    ids[is_tri] = np.stack([inst_node[inst], inst.astype(np.uint32), inst_mat[inst], prim[is_tri]], axis=-1)
    kl = hit_light[is_light]
    if kl.size:
        ids[is_light, 0] = lnode[kl]
        ids[is_light, 3] = np.uint32(0x80000000) | kl.astype(np.uint32)
    return pos.reshape(h, w, 4), ids.reshape(h, w, 4)


def reference(osc, scene, lights, w, h, frames, first_frame=0, pos=None, ids=None):
    """position / ids after folding frames first_frame .. first_frame + frames - 1 onto (pos, ids) (None: a fresh accumulation)"""
    for f in range(first_frame, first_frame + frames):
        p, i = first_hits(osc, scene, lights, w, h, f)
        pos = fold_mean(pos, p, f)
        if f == 0:
            ids = i
    return pos, ids
