"""numpy-float32 twin of docs/RENDER_SPEC.md 17 "Recomputed normals": the classes of a primitive's rest vertices, their incidence lists,
and the normal / tangent of every posed vertex from the posed triangles around it, with every `*`, `+`, `-`, `/` and sqrt of the spec as
one float32 operation (numpy has no float32 fma).  k_deform_faces / k_deform_vertex_normals (csrc/deform_normals.hip) must reproduce
recompute() bit for bit; recompute64() evaluates the same formulas in float64; the meshes the tests share are made here."""
import numpy as np

from hala_renderer_amd._abi import VERTEX_DTYPE

f32 = np.float32


def classes(rest, indices):
    """rest: VERTEX_DTYPE records, indices: flat uint32 -> dict(class_of [V], offsets [classes + 1], entries [3 T]).  Two vertices are one
    class when the 24 bytes of rest position and rest normal are equal as bit patterns; classes are numbered by their lowest member;
    entries holds the triangle of every (triangle, corner) pair of a class in ascending 3 * triangle + corner"""
    rest = np.ascontiguousarray(rest, dtype=VERTEX_DTYPE)
    idx = np.asarray(indices, dtype=np.int64).reshape(-1)
    idx = idx[:len(idx) - len(idx) % 3]
    nv = len(rest)
    key = np.concatenate([np.ascontiguousarray(rest["position"]).view(np.uint32).reshape(nv, 3),
                          np.ascontiguousarray(rest["normal"]).view(np.uint32).reshape(nv, 3)], axis=1) if nv else np.zeros((0, 6), np.uint32)
    seen, class_of = {}, np.zeros(nv, dtype=np.uint32)
    for v in range(nv):
        class_of[v] = seen.setdefault(key[v].tobytes(), len(seen))
    nc = len(seen)
    cls = class_of[idx].astype(np.int64) if len(idx) else np.zeros(0, np.int64)
    order = np.argsort(cls, kind="stable")  # corners by class, ascending corner number within one
    offsets = np.zeros(nc + 1, dtype=np.uint32)
    offsets[1:] = np.cumsum(np.bincount(cls, minlength=nc)) if nc else 0
    return dict(class_of=class_of, offsets=offsets, entries=(order // 3).astype(np.uint32))


def _faces(dt, p, idx):
    tri = idx.reshape(-1, 3)
    a = p[tri[:, 1]] - p[tri[:, 0]]
    b = p[tri[:, 2]] - p[tri[:, 0]]
    return np.stack([(a[:, 1] * b[:, 2]) - (a[:, 2] * b[:, 1]),
                     (a[:, 2] * b[:, 0]) - (a[:, 0] * b[:, 2]),
                     (a[:, 0] * b[:, 1]) - (a[:, 1] * b[:, 0])], axis=1).astype(dt)


def _sums(dt, faces, cl):
    """per class: s = 0; s = s + f for the class's entries in order"""
    off, ent = cl["offsets"].astype(np.int64), cl["entries"].astype(np.int64)
    nc = len(off) - 1
    s = np.zeros((nc, 3), dtype=dt)
    count = off[1:] - off[:-1]
    for k in range(int(count.max()) if nc else 0):  # the k-th entry of every class that has one: each class still sums in its own order
        has = np.nonzero(count > k)[0]
        s[has] = s[has] + faces[ent[off[has] + k]]
    return s, count


def _recompute(dt, posed, indices, cl):
    p = posed["position"].astype(dt)
    n0, t = posed["normal"].astype(dt), posed["tangent"].astype(dt)
    idx = np.asarray(indices, dtype=np.int64).reshape(-1)
    idx = idx[:len(idx) - len(idx) % 3]
    with np.errstate(all="ignore"):
        s_c, count_c = _sums(dt, _faces(dt, p, idx), cl)
        c = cl["class_of"].astype(np.int64)
        s, count = s_c[c], count_c[c]
        q = (s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]
        keep = (count == 0) | (q == 0) | ~np.isfinite(q)
        n = s / np.sqrt(q)[:, None]
        d = (t[:, 0] * n[:, 0] + t[:, 1] * n[:, 1]) + t[:, 2] * n[:, 2]
        u = t - n * d[:, None]
        g = (u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]
        keep_t = keep | (g == 0) | ~np.isfinite(g)
        un = u / np.sqrt(g)[:, None]
    assert n.dtype == dt and un.dtype == dt
    return keep, n, keep_t, un, s_c


def recompute(posed, indices, cl):
    """posed: VERTEX_DTYPE records as k_deform wrote them (tests/deform_ref.py), cl: classes(rest, indices) -> the records with normal and
    tangent of RENDER_SPEC 17 "Recomputed normals"; position and tex_coord, and every vertex the rule leaves alone, bit for bit as given"""
    posed = np.ascontiguousarray(posed, dtype=VERTEX_DTYPE)
    keep, n, keep_t, un, _ = _recompute(f32, posed, indices, cl)
    out = posed.copy()
    nw, tw = out["normal"].view(np.uint32).reshape(-1, 3).copy(), out["tangent"].view(np.uint32).reshape(-1, 3).copy()
    nw[~keep] = np.ascontiguousarray(n).view(np.uint32).reshape(-1, 3)[~keep]
    tw[~keep_t] = np.ascontiguousarray(un).view(np.uint32).reshape(-1, 3)[~keep_t]
    out["normal"], out["tangent"] = nw.view(f32), tw.view(f32)
    return out


def recompute64(posed, indices, cl):
    """the same formulas in float64 on the float32 inputs -> (normal [V, 3], tangent [V, 3], class sums [classes, 3]) float64; kept vertices
    carry the given values"""
    posed = np.ascontiguousarray(posed, dtype=VERTEX_DTYPE)
    keep, n, keep_t, un, s_c = _recompute(np.float64, posed, indices, cl)
    n = np.where(keep[:, None], posed["normal"].astype(np.float64), n)
    un = np.where(keep_t[:, None], posed["tangent"].astype(np.float64), un)
    return n, un, s_c


def conditioning(posed, indices, cl):
    """per class, in float64: (|sum of f|, sum of |f|) over its list, |.| the Euclidean length — a sum that nearly cancels has no bounded
    relative error"""
    p = posed["position"].astype(np.float64)
    idx = np.asarray(indices, dtype=np.int64).reshape(-1)
    f = _faces(np.float64, p, idx)
    s, _ = _sums(np.float64, f, cl)
    mag = np.zeros(len(s))
    np.add.at(mag, np.repeat(np.arange(len(s)), np.diff(cl["offsets"].astype(np.int64))), np.linalg.norm(f[cl["entries"].astype(np.int64)], axis=1))
    return np.linalg.norm(s, axis=1), mag


# ---- procedural meshes ------------------------------------------------------------------------------------------------------------------
def _records(position, normal, tangent=None, uv=None, seed=0):
    rs = np.random.RandomState(7000 + seed)
    nv = len(position)
    v = np.zeros(nv, dtype=VERTEX_DTYPE)
    v["position"] = np.asarray(position, dtype=f32)
    v["normal"] = np.asarray(normal, dtype=f32)
    if tangent is None:
        tangent = rs.normal(size=(nv, 3)) + np.array([3.0, 0.5, 0.25])
        tangent = tangent / np.linalg.norm(tangent, axis=1, keepdims=True)
    v["tangent"] = np.asarray(tangent, dtype=f32)
    v["tex_coord"] = rs.uniform(0.0, 1.0, (nv, 2)).astype(f32) if uv is None else np.asarray(uv, dtype=f32)
    return v


def grid(nx, ny, height=None, seed=0, spacing=1.0):
    """an nx x ny vertex grid in the xy plane, two counter-clockwise triangles per cell; height(x, y) -> z (None: flat), rest normal +z"""
    x, y = np.meshgrid(np.arange(nx) * spacing, np.arange(ny) * spacing)
    z = np.zeros_like(x, dtype=np.float64) if height is None else height(x, y)
    pos = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)
    k = (np.arange(ny - 1)[:, None] * nx + np.arange(nx - 1)[None, :]).ravel()
    idx = np.stack([k, k + 1, k + nx, k + 1, k + nx + 1, k + nx], axis=1).reshape(-1)
    return idx.astype(np.uint32), _records(pos, np.tile([0.0, 0.0, 1.0], (len(pos), 1)), seed=seed)


def fan(valence, seed=0, radius=2.0):
    """a closed fan: the hub (vertex 0, slightly raised) and `valence` rim vertices, `valence` triangles around the hub"""
    a = 2.0 * np.pi * np.arange(valence) / valence
    pos = np.concatenate([[[0.0, 0.0, 0.5]], np.stack([radius * np.cos(a), radius * np.sin(a), 0.1 * np.sin(3.0 * a)], axis=1)])
    r = 1 + np.arange(valence)
    idx = np.stack([np.zeros(valence, dtype=np.int64), r, 1 + (np.arange(valence) + 1) % valence], axis=1).reshape(-1)
    return idx.astype(np.uint32), _records(pos, np.tile([0.0, 0.0, 1.0], (len(pos), 1)), seed=seed)


def cylinder(columns, rows, seed=0, radius=1.0, height=2.0):
    """a tube of `columns` quads around and `rows` vertex rings, unwrapped: column `columns` repeats column 0 (same position and normal,
    another tex_coord) -> (indices, vertices, seam duplicates); V = (columns + 1) * rows"""
    a = 2.0 * np.pi * (np.arange(columns + 1) % columns) / columns  # (the duplicate gets the very same angle: equal bits)
    ring = np.stack([radius * np.cos(a), radius * np.sin(a)], axis=1).astype(f32)
    pos = np.concatenate([np.concatenate([ring, np.full((columns + 1, 1), height * j / max(rows - 1, 1), dtype=f32)], axis=1) for j in range(rows)])
    nrm = np.concatenate([np.concatenate([(ring / f32(radius)).astype(f32), np.zeros((columns + 1, 1), dtype=f32)], axis=1) for _ in range(rows)])
    uv = np.stack([np.tile(np.arange(columns + 1) / columns, rows), np.repeat(np.arange(rows) / max(rows - 1, 1), columns + 1)], axis=1)
    w = columns + 1
    k = (np.arange(rows - 1)[:, None] * w + np.arange(columns)[None, :]).ravel()
    idx = np.stack([k, k + 1, k + w, k + 1, k + w + 1, k + w], axis=1).reshape(-1)
    tan = np.concatenate([np.stack([-np.sin(a), np.cos(a), np.zeros_like(a)], axis=1) for _ in range(rows)])
    return idx.astype(np.uint32), _records(pos, nrm, tangent=tan, uv=uv, seed=seed), rows


def cube(size=1.0, seed=0):
    """24 vertices: four per face, each with its face's normal (hard edges), two triangles per face, outward"""
    pos, nrm, tan, idx = [], [], [], []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            n = np.zeros(3); n[axis] = sign
            u = np.zeros(3); u[(axis + 1) % 3] = 1.0
            w = np.cross(n, u)
            base = len(pos)
            for cu, cw in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
                pos.append(0.5 * size * (n + cu * u + cw * w)); nrm.append(n); tan.append(u)
            idx += [base, base + 1, base + 2, base, base + 2, base + 3]
    return np.asarray(idx, dtype=np.uint32), _records(np.asarray(pos), np.asarray(nrm), tangent=np.asarray(tan), seed=seed)


def with_oddities(indices, vertices):
    """the mesh plus an isolated vertex (in no triangle) and a triangle that names one index twice (zero area, two list entries)"""
    extra = vertices[:1].copy()
    extra["position"] = extra["position"] + f32(7.5)
    v = np.concatenate([vertices, extra])
    idx = np.concatenate([np.asarray(indices, dtype=np.uint32), np.array([1, 1, 2], dtype=np.uint32)])
    return idx, v
