"""numpy-float32 twin of docs/RENDER_SPEC.md 17 (deformers): rest vertices + morph targets + skin -> posed vertices, with every `*` and
`+` of the spec as one float32 operation (numpy has no float32 fma).  k_deform must reproduce deform() bit for bit; deform64() evaluates
the same formulas in float64 (tests/test_deformers.py pins the twin against it), and strip() / random_rig() make the procedural
inputs the tests share."""
import numpy as np

from hala_renderer_amd._abi import VERTEX_DTYPE

f32 = np.float32
IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], dtype=f32)


def identity_palette(joint_count):
    return np.tile(IDENTITY, (joint_count, 1, 1))


def _pose(dt, p, n, t, targets, normal_targets, tangent_targets, morph_weights, joints, weights, joint_matrices):
    """the arithmetic of RENDER_SPEC 17 in dtype `dt`, one rounding per operation"""
    p, n, t = p.astype(dt), n.astype(dt), t.astype(dt)
    if targets is not None:
        for k in range(len(targets)):
            w = dt(morph_weights[k])
            if w == 0:
                continue  # a target whose weight is exactly 0 is skipped
            p = p + w * targets[k].astype(dt)
            if normal_targets is not None:
                n = n + w * normal_targets[k].astype(dt)
            if tangent_targets is not None:
                t = t + w * tangent_targets[k].astype(dt)
    if joints is not None:
        J = np.asarray(joint_matrices).reshape(-1, 12).astype(dt)
        W = np.asarray(weights).astype(dt)
        M = np.zeros((len(p), 12), dtype=dt)
        for k in range(4):
            M = M + W[:, k:k + 1] * J[np.asarray(joints)[:, k].astype(np.int64)]

        def linear(a, r):
            return (M[:, 4 * r] * a[:, 0] + M[:, 4 * r + 1] * a[:, 1]) + M[:, 4 * r + 2] * a[:, 2]

        p = np.stack([linear(p, r) + M[:, 4 * r + 3] for r in range(3)], axis=1)
        n = np.stack([linear(n, r) for r in range(3)], axis=1)
        t = np.stack([linear(t, r) for r in range(3)], axis=1)
    return p, n, t


def deform(rest, targets=None, normal_targets=None, tangent_targets=None, morph_weights=None, joints=None, weights=None, joint_matrices=None):
    """rest: VERTEX_DTYPE records; targets / normal_targets / tangent_targets: [T, V, 3] or None; morph_weights: [T]; joints: [V, 4]
    integers, weights: [V, 4], joint_matrices: [J, 3, 4] row-major, or all three None -> posed VERTEX_DTYPE records (tex_coord copied)"""
    rest = np.ascontiguousarray(rest, dtype=VERTEX_DTYPE)
    as32 = lambda a: None if a is None else np.asarray(a, dtype=f32)  # noqa: E731
    p, n, t = _pose(f32, rest["position"], rest["normal"], rest["tangent"], as32(targets), as32(normal_targets), as32(tangent_targets),
                    None if morph_weights is None else np.asarray(morph_weights, dtype=f32), joints, as32(weights), as32(joint_matrices))
    assert p.dtype == f32 and n.dtype == f32 and t.dtype == f32
    out = rest.copy()
    out["position"], out["normal"], out["tangent"] = p, n, t
    return out


def deform64(rest, targets=None, normal_targets=None, tangent_targets=None, morph_weights=None, joints=None, weights=None, joint_matrices=None,
             magnitudes=False):
    """the same formulas in float64 on the float32 inputs -> (position, normal, tangent) [V, 3] float64.  magnitudes: every input replaced by
    its absolute value, which gives the sum of the absolute values of all terms of each component"""
    g = (lambda a: None if a is None else np.abs(np.asarray(a, dtype=f32).astype(np.float64))) if magnitudes else \
        (lambda a: None if a is None else np.asarray(a, dtype=f32).astype(np.float64))
    return _pose(np.float64, g(rest["position"]), g(rest["normal"]), g(rest["tangent"]), g(targets), g(normal_targets), g(tangent_targets),
                 None if morph_weights is None else g(morph_weights), joints, g(weights), g(joint_matrices))


# ---- procedural inputs ----------------------------------------------------------------------------------------------------------------
def strip(vertex_count, seed=0, origin=(0.0, 0.0, 0.0)):
    """a zigzag triangle strip of `vertex_count` vertices -> (indices uint32, VERTEX_DTYPE records); fewer than three vertices give one
    degenerate triangle"""
    rs = np.random.RandomState(1000 + seed)
    k = np.arange(vertex_count)
    v = np.zeros(vertex_count, dtype=VERTEX_DTYPE)
    v["position"] = (np.stack([0.5 * k, (k % 2) * 1.0, 0.05 * np.sin(0.7 * k)], axis=1) + np.asarray(origin)).astype(f32)
    nrm = rs.normal(size=(vertex_count, 3)) + np.array([0.0, 0.0, 3.0])
    v["normal"] = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(f32)
    tan = rs.normal(size=(vertex_count, 3)) + np.array([3.0, 0.0, 0.0])
    v["tangent"] = (tan / np.linalg.norm(tan, axis=1, keepdims=True)).astype(f32)
    v["tex_coord"] = rs.uniform(0.0, 1.0, (vertex_count, 2)).astype(f32)
    if vertex_count >= 3:
        idx = np.stack([k[:-2], k[1:-1], k[2:]], axis=1).reshape(-1)
    else:
        idx = np.zeros(3, dtype=np.int64)
    return idx.astype(np.uint32), v


def random_rig(vertex_count, targets=0, joint_count=0, normals=False, tangents=False, seed=0, scale=1.0, dyadic=False):
    """random tables for a primitive of `vertex_count` vertices -> dict(targets, normal_targets, tangent_targets, joints, weights,
    joint_count) as set_deformer takes them.  The highest joint index is used.  dyadic: every vertex's weights are multiples of 1/4
    that sum to 1 exactly, so that the identity palette gives the rest pose back bit for bit"""
    rs = np.random.RandomState(2000 + seed)
    out = dict(targets=None, normal_targets=None, tangent_targets=None, joints=None, weights=None, joint_count=joint_count)
    if targets:
        out["targets"] = (rs.normal(size=(targets, vertex_count, 3)) * 0.3 * scale).astype(f32)
        if normals:
            out["normal_targets"] = (rs.normal(size=(targets, vertex_count, 3)) * 0.2).astype(f32)
        if tangents:
            out["tangent_targets"] = (rs.normal(size=(targets, vertex_count, 3)) * 0.2).astype(f32)
    if joint_count:
        j = rs.randint(0, joint_count, (vertex_count, 4)).astype(np.uint16)
        j[rs.randint(0, vertex_count), rs.randint(0, 4)] = joint_count - 1
        if dyadic:
            w = np.array([[0.5, 0.25, 0.25, 0.0], [1.0, 0.0, 0.0, 0.0], [0.25, 0.25, 0.25, 0.25], [0.0, 0.75, 0.0, 0.25]], dtype=f32)[rs.randint(0, 4, vertex_count)]
        else:
            w = rs.uniform(0.0, 1.0, (vertex_count, 4))
            w[rs.uniform(size=w.shape) < 0.3] = 0.0
            w = (w / np.maximum(w.sum(axis=1, keepdims=True), 1e-3)).astype(f32)  # (close to 1 in sum, not renormalised by the library)
        out["joints"], out["weights"] = j, w
    return out


def random_pose(rig, seed=0, zero_some=True, centre=(0.0, 0.0, 0.0), scale=1.0):
    """-> dict(morph_weights, joint_matrices) for update_deformer: weights in [-1, 1.5] with some exactly 0, joints rotating by up to ~0.5
    rad about `centre` with a small translation and a non-uniform scale"""
    rs = np.random.RandomState(3000 + seed)
    out = dict(morph_weights=None, joint_matrices=None)
    if rig["targets"] is not None:
        w = rs.uniform(-1.0, 1.5, len(rig["targets"])).astype(f32)
        if zero_some and len(w) > 1:
            w[rs.uniform(size=len(w)) < 0.4] = 0.0
            w[0] = w[0] if w[0] != 0.0 else f32(0.625)
        out["morph_weights"] = w
    if rig["joint_count"]:
        c = np.asarray(centre, dtype=np.float64)
        mats = np.zeros((rig["joint_count"], 3, 4), dtype=f32)
        for k in range(rig["joint_count"]):
            a = rs.uniform(-0.5, 0.5, 3)
            rx = np.array([[1, 0, 0], [0, np.cos(a[0]), -np.sin(a[0])], [0, np.sin(a[0]), np.cos(a[0])]])
            ry = np.array([[np.cos(a[1]), 0, np.sin(a[1])], [0, 1, 0], [-np.sin(a[1]), 0, np.cos(a[1])]])
            rz = np.array([[np.cos(a[2]), -np.sin(a[2]), 0], [np.sin(a[2]), np.cos(a[2]), 0], [0, 0, 1]])
            m = rz @ ry @ rx @ np.diag(rs.uniform(0.8, 1.2, 3))
            mats[k, :, :3] = m
            mats[k, :, 3] = c - m @ c + rs.uniform(-0.1, 0.1, 3) * scale
        out["joint_matrices"] = mats
    return out


def pose_vertices(rest, rig, pose):
    """deform() with a rig and a pose as random_rig / random_pose make them (a missing part of the pose: weights 0 / the identity)"""
    mw = pose.get("morph_weights")
    jm = pose.get("joint_matrices")
    if rig["targets"] is not None and mw is None:
        mw = np.zeros(len(rig["targets"]), dtype=f32)
    if rig["joint_count"] and jm is None:
        jm = identity_palette(rig["joint_count"])
    return deform(rest, rig["targets"], rig["normal_targets"], rig["tangent_targets"], mw,
                  rig["joints"] if rig["joint_count"] else None, rig["weights"] if rig["joint_count"] else None, jm if rig["joint_count"] else None)
