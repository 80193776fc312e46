"""numpy twin of temporal reprojection (docs/RENDER_SPEC.md 16), written from the spec text: the motion of an instance in float64, the
projection, the resolve (reprojection, tap validation, blend) and the capture, every float32 operation in the order the spec writes it
(the fma of `dot` / `madd` is emulated exactly by aov_ref.fma).  csrc/temporal.hip is held to it byte for byte (tests/test_temporal.py).

It also holds a float64 geometric model that shares nothing with the twin but the scene: model_motion() takes the triangle and the
barycentrics of each sample's first hit, places the same surface point under the pre-edit transforms and projects it through the pre-edit
camera with numpy's own float64 arithmetic."""
import dataclasses
import math

import numpy as np

import aov_ref
from aov_ref import dot, fma

f32, f64 = np.float32, np.float64
ABSENT = np.uint32(0xFFFFFFFF)


@dataclasses.dataclass
class Params:
    max_history: float = 32.0
    tol: float = 0.05
    min_weight: float = 0.25


def check_params(max_history, tol, min_weight, reserved=(0, 0, 0, 0, 0)):
    """"" or the reason RENDER_SPEC 16 refuses the parameters (the wording of hala_rt_set_temporal)"""
    mh, tl, mw = f32(max_history), f32(tol), f32(min_weight)
    if not (mh >= f32(1.0) and mh <= f32(1048576.0)):
        return "Invalid temporal max_history: expected a finite value in [1, 2^20]."
    if not (tl >= f32(1e-6) and tl <= f32(1.0)):
        return "Invalid temporal tol: expected a finite value in [1e-6, 1]."
    if not (mw > f32(0.0) and mw <= f32(1.0)):
        return "Invalid temporal min_weight: expected a finite value in (0, 1]."
    if any(reserved):
        return "The reserved words of the temporal parameters must be zero."
    return ""


# ---- RENDER_SPEC 2.2 on the host: tan(yfov / 2) as the renderer computes it ----------------------------------------------------------------
def _poly(a2, coeffs):
    p = f32(coeffs[0])
    for c in coeffs[1:]:
        p = fma(p, a2, f32(c))[()]
    return p


def tan_half(yfov):
    """sin / cos of sincos_rad(yfov / 2): Taylor polynomials on [0, pi/2] by Horner with fma, quadrant table"""
    a = f32(0.5) * f32(yfov)
    t = f32(a * f32(0.15915494309189533577))
    t = f32(t - np.floor(t))
    if t >= f32(1.0):
        t = f32(0.0)
    x = f32(t * f32(4.0))
    q = int(x)
    ang = f32(f32(x - f32(q)) * f32(1.57079632679489661923))
    a2 = f32(ang * ang)
    sa = f32(ang * _poly(a2, (-2.50521083854417187751e-8, 2.75573192239858906526e-6, -1.98412698412698412698e-4, 8.33333333333333333333e-3,
                              -1.66666666666666666667e-1, 1.0)))
    ca = _poly(a2, (2.08767569878680989792e-9, -2.75573192239858906526e-7, 2.48015873015873015873e-5, -1.38888888888888888889e-3,
                    4.16666666666666666667e-2, -0.5, 1.0))
    s, c = ((sa, ca), (ca, -sa), (-sa, -ca), (-ca, sa))[q & 3]
    return f32(f32(s) / f32(c))


@dataclasses.dataclass
class Camera:
    position: np.ndarray
    right: np.ndarray
    up: np.ndarray
    forward: np.ndarray
    tan_half: np.float32
    xmag: np.float32
    ymag: np.float32
    type: int


def camera_of(packed):
    """a packed camera record (hala_gpu_camera / _abi.GpuCamera) -> what the projection reads"""
    v = lambda a: np.array(a[:3], dtype=f32)  # noqa: E731
    return Camera(v(packed.position), v(packed.right), v(packed.up), v(packed.forward), tan_half(packed.yfov) if packed.type == 0 else f32(0.0),
                  f32(packed.focal_distance_or_xmag), f32(packed.aperture_or_ymag), int(packed.type))


# ---- motion of an instance -------------------------------------------------------------------------------------------------------------
def motion_matrix(w_prev, w_cur):
    """D = W_prev . W_cur^-1 (3 x 4 float32, row-major) and whether W_cur is invertible; w_*: 16 floats, column-major"""
    wp, wc = np.asarray(w_prev, dtype=f32).reshape(16), np.asarray(w_cur, dtype=f32).reshape(16)
    ident = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], dtype=f32)
    if wp.tobytes() == wc.tobytes():
        return ident, True
    a = [[float(wc[4 * c + r]) for c in range(4)] for r in range(3)]
    p = [[float(wp[4 * c + r]) for c in range(4)] for r in range(3)]
    j = [[a[1][1] * a[2][2] - a[1][2] * a[2][1], a[0][2] * a[2][1] - a[0][1] * a[2][2], a[0][1] * a[1][2] - a[0][2] * a[1][1]],
         [a[1][2] * a[2][0] - a[1][0] * a[2][2], a[0][0] * a[2][2] - a[0][2] * a[2][0], a[0][2] * a[1][0] - a[0][0] * a[1][2]],
         [a[1][0] * a[2][1] - a[1][1] * a[2][0], a[0][1] * a[2][0] - a[0][0] * a[2][1], a[0][0] * a[1][1] - a[0][1] * a[1][0]]]
    det = (a[0][0] * j[0][0] + a[0][1] * j[1][0]) + a[0][2] * j[2][0]
    s = 1.0
    for c in range(3):
        s = s * math.sqrt((a[0][c] * a[0][c] + a[1][c] * a[1][c]) + a[2][c] * a[2][c])
    if not (abs(det) > 1e-12 * s):
        return ident, False
    inv = [[j[r][c] / det for c in range(3)] for r in range(3)]
    out = np.empty((3, 4), dtype=f32)
    with np.errstate(over="ignore"):
        for r in range(3):
            row = [(p[r][0] * inv[0][c] + p[r][1] * inv[1][c]) + p[r][2] * inv[2][c] for c in range(3)]
            t = p[r][3] - ((row[0] * a[0][3] + row[1] * a[1][3]) + row[2] * a[2][3])
            out[r] = [f32(row[0]), f32(row[1]), f32(row[2]), f32(t)]
    if not np.isfinite(out).all():
        return ident, False
    return out, True


# ---- projection ------------------------------------------------------------------------------------------------------------------------
def project(cam, P, W, H):
    """RENDER_SPEC 16 "Projection" for points P [N, 3] float32 -> u, v, z [N] float32 and ok [N]"""
    Wf, Hf = f32(W), f32(H)
    aspect = f32(Wf / Hf)
    bc = lambda a: np.broadcast_to(a, P.shape)  # noqa: E731
    with np.errstate(all="ignore"):
        d = (P - cam.position).astype(f32)
        ff = dot(cam.forward, cam.forward)
        vf = dot(d, bc(cam.forward))
        a = (dot(d, bc(cam.right)) / dot(cam.right, cam.right)).astype(f32)
        b = (dot(d, bc(cam.up)) / dot(cam.up, cam.up)).astype(f32)
        z = (vf * (f32(1.0) / np.sqrt(ff))).astype(f32)
        if cam.type == 0:
            c = (vf / ff).astype(f32)
            nx = ((a / c) / f32(aspect * cam.tan_half)).astype(f32)
            ny = ((b / c) / cam.tan_half).astype(f32)
            ok = z > f32(0.0)
        else:
            nx = (a / cam.xmag).astype(f32)
            ny = (b / cam.ymag).astype(f32)
            ok = np.ones(P.shape[0], bool)
        u = (((nx + f32(1.0)) * f32(0.5)) * Wf - f32(0.5)).astype(f32)
        v = (((f32(1.0) - ny) * f32(0.5)) * Hf - f32(0.5)).astype(f32)
    return u, v, z, ok


# ---- history, capture, resolve -----------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class History:
    Hc: np.ndarray      # [H, W, 4] float32: rgb, history length
    Hp: np.ndarray      # image 4 as captured
    Hi: np.ndarray      # image 5 as captured, uint32
    cam: Camera
    world: np.ndarray   # [instances, 16] float32, column-major


def resolve(C, Pm, I, n, hist, cam_cur, world_cur, inst_marked=None, mat_marked=None, material_count=None, params=Params()):
    """-> (temporal, motion) [H, W, 4] float32.  C: accum, Pm: image 4, I: image 5 (uint32), n: samples folded; hist: History or None;
    world_cur [instances, 16]; the marks: bool per instance / per material (None: none)"""
    H, W = C.shape[:2]
    N = H * W
    Cf = np.ascontiguousarray(C, dtype=f32).reshape(N, 4)
    Pf = np.ascontiguousarray(Pm, dtype=f32).reshape(N, 4)
    If = np.ascontiguousarray(I).view(np.uint32).reshape(N, 4)
    nf = f32(n)
    T = np.concatenate([Cf[:, :3], np.full((N, 1), nf, f32)], axis=1)
    M = np.zeros((N, 4), f32)
    world_cur = np.asarray(world_cur, dtype=f32).reshape(-1, 16)
    if hist is None or hist.world.shape != world_cur.shape:
        return T.reshape(H, W, 4), M.reshape(H, W, 4)
    ni = world_cur.shape[0]
    nm = int(material_count) if material_count is not None else (len(mat_marked) if mat_marked is not None else int(1 << 31))
    D = np.empty((ni, 3, 4), f32)
    imark = np.zeros(ni, bool) if inst_marked is None else np.asarray(inst_marked, bool).copy()
    for i in range(ni):
        D[i], ok = motion_matrix(hist.world[i], world_cur[i])
        imark[i] |= not ok
    mmark = np.zeros(0, bool) if mat_marked is None else np.asarray(mat_marked, bool)
    inst, mat = If[:, 1], If[:, 2]
    with np.errstate(all="ignore"):
        live = (inst != ABSENT) & (Pf[:, 3] > f32(0.0)) & (inst < ni) & (mat < nm)
        live[live] &= ~imark[inst[live]]
        if mmark.size:
            k = live & (mat < mmark.size)
            live[k] &= ~mmark[mat[k]]
        idx = np.nonzero(live)[0]
        if idx.size == 0:
            return T.reshape(H, W, 4), M.reshape(H, W, 4)
        Pw = (Pf[idx, :3] / Pf[idx, 3:4]).astype(f32)
        Di = D[inst[idx]]
        Pprev = np.stack([fma(Di[:, r, 2], Pw[:, 2], fma(Di[:, r, 1], Pw[:, 1], fma(Di[:, r, 0], Pw[:, 0], Di[:, r, 3]))) for r in range(3)], axis=-1)
        au, av, az, aok = project(hist.cam, Pprev, W, H)
        bu, bv, _, bok = project(cam_cur, Pw, W, H)
        ok = aok & bok
        idx, Pprev, au, av, az, bu, bv = idx[ok], Pprev[ok], au[ok], av[ok], az[ok], bu[ok], bv[ok]
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
        one = f32(1.0)
        for k in range(4):
            qx, qy = x0 + (k & 1), y0 + (k >> 1)
            wx = tx if (k & 1) else (one - tx).astype(f32)
            wy = ty if (k >> 1) else (one - ty).astype(f32)
            w = (wx * wy).astype(f32)
            valid = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H) & (w > f32(0.0))
            q = np.where(valid, qy * W + qx, 0)
            qc, qp, qi = Hc[q], Hp[q], Hi[q]
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
        T[idx] = np.concatenate([rgb, tw[:, None]], axis=1)
    return T.reshape(H, W, 4), M.reshape(H, W, 4)


def capture(C, Pm, I, n, hist, cam_cur, world_cur, inst_marked=None, mat_marked=None, material_count=None, params=Params()):
    """RENDER_SPEC 16 "Capture": the new history (n = 0: the old one, untouched)"""
    if n == 0:
        return hist
    T, _ = resolve(C, Pm, I, n, hist, cam_cur, world_cur, inst_marked, mat_marked, material_count, params)
    return History(T, np.array(Pm, dtype=f32), np.ascontiguousarray(I).view(np.uint32).copy(), cam_cur,
                   np.asarray(world_cur, dtype=f32).reshape(-1, 16).copy())


# ---- marks from a list of scene_edits operations ------------------------------------------------------------------------------------------
def marks_of(scene, ops):
    """(instance marks, material marks) the renderer sets for the operations of tests/scene_edits.py on `scene`"""
    INVALID = 0xFFFFFFFF
    inst_prim = [(nd.mesh_index, p) for nd in scene.nodes if nd.mesh_index != INVALID for p in range(len(scene.meshes[nd.mesh_index].primitives))]
    im, mm = np.zeros(len(inst_prim), bool), np.zeros(len(scene.materials), bool)
    for op in ops:
        if op[0] == "vertices":
            for i, mp in enumerate(inst_prim):
                im[i] |= mp == (op[1], op[2])
        elif op[0] == "material":
            mm[op[1]] = True
    return im, mm


# ---- the float64 geometric model ----------------------------------------------------------------------------------------------------------
def _project64(cam, yfov, P, W, H):
    pos, right, up, fwd = (np.array(getattr(cam, k)[:3], dtype=f64) for k in ("position", "right", "up", "forward"))
    d = P - pos
    a, b, c = d @ right / (right @ right), d @ up / (up @ up), d @ fwd / (fwd @ fwd)
    if cam.type == 0:
        th = math.tan(0.5 * float(yfov))
        nx, ny = a / c / (W / H * th), b / c / th
    else:
        nx, ny = a / float(cam.focal_distance_or_xmag), b / float(cam.aperture_or_ymag)
    return np.stack([(nx + 1.0) * 0.5 * W - 0.5, (1.0 - ny) * 0.5 * H - 0.5], axis=-1)


def surface_points(scene, node_world, prim, u, v):
    """float64 world positions of the surface points (global triangle id `prim`, barycentrics u, v) of `scene` under the node world
    transforms node_world [nodes, 16] (column-major): P = W . ((1 - u - v) v0 + u v1 + v v2)"""
    inst_node, _, first = aov_ref.instance_table(scene)
    prims = [p for nd in scene.nodes if nd.mesh_index != 0xFFFFFFFF for p in scene.meshes[nd.mesh_index].primitives]
    inst = np.searchsorted(first[:-1], prim.astype(np.uint64), side="right") - 1
    out = np.empty((prim.size, 3), f64)
    for i in np.unique(inst):
        sel = inst == i
        p = prims[i]
        tri = np.asarray(p.indices, dtype=np.int64).reshape(-1, 3)[prim[sel].astype(np.int64) - int(first[i])]
        vp = p.vertices["position"].astype(f64)
        uu, vv = u[sel].astype(f64)[:, None], v[sel].astype(f64)[:, None]
        obj = (1.0 - uu - vv) * vp[tri[:, 0]] + uu * vp[tri[:, 1]] + vv * vp[tri[:, 2]]
        Wm = np.asarray(node_world[inst_node[i]], dtype=f64).reshape(4, 4).T  # column-major -> rows
        out[sel] = obj @ Wm[:3, :3].T + Wm[:3, 3]
    return out


def model_motion(scene_prev, scene_cur, world_prev, world_cur, cam_prev, cam_cur, hits, W, H):
    """float64 motion [N, 2] and the current mean surface point [N, 3] of the pixels whose samples all hit one triangle (mask [N]).
    hits: per sample a (prim, u, v) triple of [N] arrays from the oracle's trace of the EDITED scene's camera rays; world_*: node world
    transforms [nodes, 16]; cam_*: packed camera records (their yfov is read for a perspective camera)"""
    prim0 = hits[0][0]
    same = prim0 != ABSENT
    for prim, _, _ in hits[1:]:
        same &= prim == prim0
    sel = np.nonzero(same)[0]
    cur = np.mean([surface_points(scene_cur, world_cur, prim[sel], u[sel], v[sel]) for prim, u, v in hits], axis=0)
    prev = np.mean([surface_points(scene_prev, world_prev, prim[sel], u[sel], v[sel]) for prim, u, v in hits], axis=0)
    m = _project64(cam_prev, cam_prev.yfov, prev, W, H) - _project64(cam_cur, cam_cur.yfov, cur, W, H)
    motion = np.zeros((same.size, 2), f64)
    motion[sel] = m
    points = np.zeros((same.size, 3), f64)
    points[sel] = cur
    return motion, points, same
