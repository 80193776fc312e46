"""float64 numpy reference of the deterministic half of the shade path: from the scene description to the first hit of every camera
ray and the surface found there.  Written from docs/RENDER_SPEC.md (sections 2.3, 3, 5, 6, 7.2-7.4, 8, 13) and from the scene model
alone: it calls neither the oracle nor the product and reads no packed record.  Conventions that come from the original renderer are
cited where they are used.

What is computed: world transforms, world-space triangles, the instance / node / material / light tables, the camera rays of any scene
camera (perspective, thin lens, orthographic), the nearest hit over all triangles (Moeller-Trumbore, brute force) and the hittable
lights, the surface (shading normal through sign(det)-cofactors, uv and tangent interpolation, texture LOD, mip choice, trilinear fetch
of all four texel formats, base-colour / emission / normal maps, the medium a ray from behind has crossed: 7.1e), the miss radiance (sky
gradient or env map), and the running means of albedo, normal, position, ids and the first vertex's radiance.

True tan, sin, cos, atan2, acos, exp and sqrt in `dtype` take the place of the spec's polynomials, and plain sums of products that of
its fma sequences.  Two decisions of the spec are
integer-valued and reproduced exactly: the RNG (uint64 arithmetic masked to 32 bits; float(x >> 8) * 2^-24 is exact in every float type)
and the byte an 8-bit mip level stores (`mip_level_f32`: float32 emulation).  `log2a` (exponent + mantissa - 1 of the float32 value) is
the spec's definition of the level of detail and is implemented as defined.

Every stage takes `dtype`: the test runs the same code in float32 to measure how much float32 rounding alone moves each output, which
sets its tolerances.  `fragile` marks the pixels whose discrete decisions (which triangle, which side of an edge, light or surface) are
within DELTA of flipping; they are left out of comparisons.

Still unpinned by any independent reference: opacity skipping (7.1d; every scene of these tests keeps opacity 1 and texture alpha 255,
since skipping changes which surface is first), the metallic-roughness map (not observable at the first hit), the BSDF and light
sampling."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
M32 = np.uint64(0xFFFFFFFF)
ABSENT = 0xFFFFFFFF
MAX_LIGHTS, MAX_CAMERAS = 32, 8  # gpu_uploader.rs:99-111, :142-147, :290
DELTA = 1e-4
FMT_UNORM, FMT_SRGB, FMT_FLOAT, FMT_BGRA = 0, 1, 2, 3
QUAD, SPHERE = 3, 4
MISS, LIGHT, SURFACE = 0, 1, 2


def _a(x, dt):
    """an input of the scene (a float32 quantity in every record) as an array of the working type"""
    return np.asarray(x, dtype=f32).astype(dt)


def _dot(a, b):
    return np.sum(a * b, axis=-1)


def _norm(v):
    return v / np.sqrt(_dot(v, v))[..., None]


class Settings:
    def __init__(self, env=None, env_rotation=0.0, env_intensity=1.0, ground=(1.0, 1.0, 1.0), sky=(0.5, 0.7, 1.0)):
        self.env = None if env is None else np.asarray(env, dtype=f32)[..., :3]
        self.env_rotation, self.env_intensity, self.ground, self.sky = env_rotation, env_intensity, ground[:3], sky[:3]


# ---- 1. world transforms (cpu/scene.rs:99-114: world = parent's world * local) ----------------------------------------------------
def world_transforms(scene, dt=f64):
    out = [None] * len(scene.nodes)

    def world(i):
        if out[i] is None:
            nd = scene.nodes[i]
            m = _a(nd.local_transform, dt)
            out[i] = m if nd.parent is None else world(nd.parent) @ m
        return out[i]
    return [world(i) for i in range(len(scene.nodes))]


# ---- 2. / 3. triangles and tables (RENDER_SPEC 3; gpu_uploader.rs:843-875: nodes in order, primitives of the node's mesh in order) ----
class Geometry:
    pass


def _has_mesh(nd):
    return nd.mesh_index != ABSENT


def tables(scene):
    """(node, material, first triangle) per instance — first has one more entry, the triangle count — and the node of every packed light"""
    node, material, first, total = [], [], [], 0
    for k, nd in enumerate(scene.nodes):
        if not _has_mesh(nd):
            continue
        for p in scene.meshes[nd.mesh_index].primitives:
            node.append(k); material.append(p.material_index); first.append(total)
            total += len(p.indices) // 3
    lights = [k for k, nd in enumerate(scene.nodes) if nd.light_index != ABSENT][:MAX_LIGHTS]
    return np.array(node, np.int64), np.array(material, np.int64), np.array(first + [total], np.int64), np.array(lights, np.int64)


def triangles(scene, world, dt=f64):
    """world-space triangles in instance order, then index order, with the local vertex attributes of their corners"""
    g = Geometry()
    g.inst_node, g.inst_mat, g.inst_first, g.light_node = tables(scene)
    pos, nrm, tan, uv, inst = [], [], [], [], []
    k = 0
    for nd in scene.nodes:
        if not _has_mesh(nd):
            continue
        for p in scene.meshes[nd.mesh_index].primitives:
            m = world[g.inst_node[k]]
            idx = np.asarray(p.indices, np.int64).reshape(-1, 3)
            local = _a(p.vertices["position"], dt)
            wp = local @ m[:3, :3].T + m[:3, 3]
            pos.append(wp[idx]); nrm.append(_a(p.vertices["normal"], dt)[idx]); tan.append(_a(p.vertices["tangent"], dt)[idx])
            uv.append(_a(p.vertices["tex_coord"], dt)[idx]); inst.append(np.full(len(idx), k, np.int64))
            k += 1
    g.v, g.n, g.tg, g.uv, g.inst = (np.concatenate(x) for x in (pos, nrm, tan, uv, inst))
    g.A = np.stack([world[n][:3, :3] for n in g.inst_node])
    lo, hi = g.v.reshape(-1, 3).min(axis=0), g.v.reshape(-1, 3).max(axis=0)
    g.extent = float(np.sqrt(_dot(hi - lo, hi - lo)))
    return g


def lights(scene, world, dt=f64):
    """the hittable form of every packed light (gpu_uploader.rs:150-293): intensity = colour * intensity; QUAD: corner = origin of the node
    minus half of each side, sides u, v = the node's x and y axes times the two params (:226-235); SPHERE: centre, radius = param 0 (:260-263)"""
    res = []
    nodes = [k for k, nd in enumerate(scene.nodes) if nd.light_index != ABSENT][:MAX_LIGHTS]
    for k in nodes:
        l = scene.lights[scene.nodes[k].light_index]
        m = world[k]
        L = Geometry()
        L.type = l.light_type
        L.intensity = _a(l.color, dt) * _a(l.intensity, dt)
        p0, p1 = _a(l.params[0], dt), _a(l.params[1], dt)
        if l.light_type == QUAD:
            L.u, L.v = m[:3, 0] * p0, m[:3, 1] * p1
            L.pos = m[:3, 3] - m[:3, 0] * p0 * dt(0.5) - m[:3, 1] * p1 * dt(0.5)
        else:
            L.pos, L.radius = m[:3, 3], p0
        res.append(L)
    return res


# ---- 4. camera rays (RENDER_SPEC 2.3, 5) ---------------------------------------------------------------------------------------------
def pcg(v):
    v = np.asarray(v, np.uint64)
    s = (v * np.uint64(747796405) + np.uint64(2891336453)) & M32
    w = (((s >> ((s >> np.uint64(28)) + np.uint64(4))) ^ s) * np.uint64(277803737)) & M32
    return ((w >> np.uint64(22)) ^ w) & M32


def rng_init(w, h, frame):
    pixel = np.arange(w * h, dtype=np.uint64)  # y * W + x
    key = pcg((np.uint64(frame) * np.uint64(0x9E3779B9) + np.uint64(0x85EBCA6B)) & M32)
    return pcg((pixel + key) & M32)


def rand(state, dt):
    x = pcg(state)
    return ((x >> np.uint64(8)).astype(f64) * 2.0 ** -24).astype(dt), (state + np.uint64(1)) & M32


def camera_rays(scene, world, c, w, h, frame, dt=f64):
    """origins, directions [W*H, 3] of camera c (row 0 = top row) and the camera's pixel_spread (7.4).  position / right / up / forward are
    columns 3, 0, 1 and minus column 2 of the world matrix of the first node that names the camera (gpu/camera.rs:29-32, gpu_uploader.rs:112)."""
    cam = scene.cameras[c]
    m = world[next(i for i, nd in enumerate(scene.nodes) if nd.camera_index == c)]
    right, up, fwd, pos = m[:3, 0], m[:3, 1], -m[:3, 2], m[:3, 3]
    state = rng_init(w, h, frame)
    r1, state = rand(state, dt); r2, state = rand(state, dt); r3, state = rand(state, dt); r4, state = rand(state, dt)
    y, x = np.divmod(np.arange(w * h), w)
    fx, fy = (x.astype(dt) + r1) / dt(w), (y.astype(dt) + r2) / dt(h)
    ndc_x, ndc_y = dt(2) * fx - dt(1), dt(1) - dt(2) * fy
    if hasattr(cam, "yfov"):
        tan_half = np.tan(_a(cam.yfov, dt) / dt(2))
        aspect = dt(w) / dt(h)
        d = _norm(fwd + right * (ndc_x * aspect * tan_half)[:, None] + up * (ndc_y * tan_half)[:, None])
        o = np.broadcast_to(pos, d.shape).copy()
        aperture = _a(cam.aperture, dt)
        if aperture > 0:
            focus = pos + d * (_a(cam.focal_distance, dt) / _dot(d, fwd))[:, None]
            r, ang = aperture * np.sqrt(r3), dt(2 * math.pi) * r4
            o = pos + right * (r * np.cos(ang))[:, None] + up * (r * np.sin(ang))[:, None]
            d = _norm(focus - o)
        return o, d, dt(2) * tan_half / dt(h)
    o = pos + right * (ndc_x * _a(cam.xmag, dt))[:, None] + up * (ndc_y * _a(cam.ymag, dt))[:, None]
    return o, np.broadcast_to(_norm(fwd), o.shape).copy(), dt(0)


# ---- 5. nearest hit (RENDER_SPEC 4.2, 6.1, 7.2) -------------------------------------------------------------------------------------
def light_hits(ls, o, d, dt):
    """t [L, N] (inf: not hit), the margin of the acceptance terms [L, N] (how far the nearest of them is from flipping) and the distance
    at which the ray meets the light's plane, or passes the sphere, whether accepted or not [L, N]"""
    n = o.shape[0]
    t_all, margin, reach = (np.full((len(ls), n), np.inf, dt) for _ in range(3))
    with np.errstate(all="ignore"):
        for k, L in enumerate(ls):
            if L.type == QUAD:  # hit from the front only: the side n = normalize(cross(u, v)) points to
                nrm = _norm(np.cross(L.u, L.v))
                dn = _dot(d, nrm)
                t = _dot(L.pos - o, nrm) / dn
                hp = o + d * t[:, None] - L.pos
                a, b = _dot(hp, L.u) / _dot(L.u, L.u), _dot(hp, L.v) / _dot(L.v, L.v)
                ok = (dn < 0) & (t > 0) & (a >= 0) & (a <= 1) & (b >= 0) & (b <= 1)
                mg = np.minimum.reduce([np.abs(a), np.abs(a - 1), np.abs(b), np.abs(b - 1)])
                t_plane, mg = np.where(np.isfinite(t), t, np.inf), np.where(np.abs(dn) <= DELTA, 0.0, mg)
            elif L.type == SPHERE:  # hit from outside only: the nearer root, in front of the origin
                oc = o - L.pos
                b = _dot(oc, d)
                c = _dot(oc, oc) - L.radius * L.radius
                disc = b * b - c
                t = -b - np.sqrt(disc)
                ok = (disc > 0) & (t > 0) & (c > 0)
                mg = np.abs(disc) / np.maximum(b * b, np.finfo(dt).tiny)
                t_plane = np.where(disc > 0, t, -b)  # the closest approach stands for t while the ray passes just outside
            else:
                continue
            t_all[k] = np.where(ok, t, np.inf)
            margin[k] = np.where(t_plane > 0, mg, np.inf)
            margin[k] = np.where(np.isnan(margin[k]), 0.0, margin[k])
            reach[k] = t_plane
    return t_all, margin, reach


def nearest_hit(g, ls, o, d, dt=f64, chunk=256):
    """per ray: kind, t, u, v, triangle id (-1), light index (-1), fragile (RENDER_SPEC 4.2: no culling, t > 0, ties to the lower id; then
    the hittable lights, the nearest of all wins, a light only when strictly nearer than the surface and than every lower-numbered light)"""
    n = o.shape[0]
    v0, e1, e2 = g.v[:, 0], g.v[:, 1] - g.v[:, 0], g.v[:, 2] - g.v[:, 0]
    lt, lmargin, lreach = light_hits(ls, o, d, dt)
    t_light = lt.min(axis=0) if len(ls) else np.full(n, np.inf, dt)
    i_light = lt.argmin(axis=0) if len(ls) else np.zeros(n, np.int64)  # first minimum: the lower index
    t_tri, uu, vv, prim = np.full(n, np.inf, dt), np.zeros(n, dt), np.zeros(n, dt), np.full(n, -1, np.int64)
    fragile = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for s in range(0, n, chunk):
            oo, dd = o[s:s + chunk, None, :], d[s:s + chunk, None, :]
            p = np.cross(dd, e2[None])
            det = _dot(e1[None], p)
            inv = dt(1) / det
            tv = oo - v0[None]
            u = _dot(tv, p) * inv
            q = np.cross(tv, e1[None])
            v = _dot(dd, q) * inv
            t = _dot(e2[None], q) * inv
            ok = (det != 0) & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (t > 0)
            tt = np.where(ok, t, np.inf)
            best = tt.argmin(axis=1)  # first minimum: ties go to the lower id
            rows = np.arange(tt.shape[0])
            tb = tt[rows, best]
            hit = np.isfinite(tb)
            t_tri[s:s + chunk] = tb
            prim[s:s + chunk] = np.where(hit, best, -1)
            uu[s:s + chunk], vv[s:s + chunk] = u[rows, best], v[rows, best]
            # fragile: an edge within DELTA (in barycentric units) on a triangle's plane in front of, or just behind, the hit; a second
            # accepted triangle within DELTA (relative) of the first
            t_hit = np.minimum(tb, t_light[s:s + chunk])
            reach = t_hit * (1 + DELTA)
            edge = np.abs(np.minimum(np.minimum(u, v), dt(1) - u - v)) <= DELTA
            fr = np.any((det != 0) & (t > 0) & (t <= reach[:, None]) & edge, axis=1)
            if tt.shape[1] > 1:
                second = np.partition(tt, 1, axis=1)[:, 1]
                fr |= hit & (second <= tb * (1 + DELTA))
            fragile[s:s + chunk] = fr
    is_light = t_light < t_tri
    t_hit = np.minimum(t_tri, t_light)
    kind = np.where(is_light, LIGHT, np.where(prim >= 0, SURFACE, MISS))
    # lights: an acceptance term within DELTA of flipping on a light in reach; two candidates (light / light, light / surface) within DELTA
    for k in range(len(ls)):
        in_reach = lreach[k] <= t_hit * (1 + DELTA)
        fragile |= in_reach & (lmargin[k] <= DELTA)
        others = np.minimum(t_tri, np.delete(lt, k, axis=0).min(axis=0)) if len(ls) > 1 else t_tri
        with np.errstate(all="ignore"):
            fragile |= np.isfinite(lt[k]) & np.isfinite(others) & (np.abs(lt[k] - others) <= DELTA * np.minimum(lt[k], others))
    fragile |= np.isfinite(t_hit) & (t_hit <= DELTA * g.extent)
    return dict(kind=kind, t=t_hit, u=uu, v=vv, prim=np.where(is_light, -1, prim), light=np.where(is_light, i_light, -1), fragile=fragile)


# ---- textures (RENDER_SPEC 7.4) ------------------------------------------------------------------------------------------------------
def srgb_lut():
    """the sRGB EOTF of every byte code: evaluated in double, rounded to float"""
    c = np.arange(256, dtype=f64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4).astype(f32)


def decode_level0(img, lut):
    """texel VALUES of level 0 as float32 [h, w, 4]"""
    d = np.asarray(img.data)
    if img.format == FMT_FLOAT:
        return d.astype(f32).reshape(img.height, img.width, 4)
    d = d.reshape(img.height, img.width, 4)
    out = (d.astype(f32) / f32(255)).astype(f32)
    if img.format == FMT_SRGB:
        out[..., :3] = lut[d[..., :3]]
    elif img.format == FMT_BGRA:  # the B8G8R8A8_UNORM tag of cpu/image_data.rs:39-43: red and blue change places
        out = out[..., [2, 1, 0, 3]]
    return out


def mip_level_f32(prev, w, h, level, fmt, lut):
    """level `level` of a w x h image from the level below it (`prev`, float32 VALUES), in the spec's float32 arithmetic: the 2 x 2 box of
    the edge-clamped block, and for 8-bit formats the VALUE of the byte the level stores — UNORM floor(box * 255 + 0.5), sRGB rgb the
    nearest code (the number of midpoints between neighbouring codes of `lut` that lie below box)"""
    sh, sw = prev.shape[:2]
    dh, dw = max(1, h >> level), max(1, w >> level)
    ys0 = np.minimum(2 * np.arange(dh), sh - 1); ys1 = np.minimum(2 * np.arange(dh) + 1, sh - 1)
    xs0 = np.minimum(2 * np.arange(dw), sw - 1); xs1 = np.minimum(2 * np.arange(dw) + 1, sw - 1)
    a, b = prev[ys0][:, xs0], prev[ys0][:, xs1]
    c, dd = prev[ys1][:, xs0], prev[ys1][:, xs1]
    exp = (((a + b).astype(f32) + (c + dd).astype(f32)).astype(f32) * f32(0.25)).astype(f32)
    if fmt != FMT_FLOAT:
        un = (np.clip(np.floor(exp * f32(255) + f32(0.5)), 0, 255).astype(np.uint32).astype(f32) / f32(255)).astype(f32)
        if fmt == FMT_SRGB:
            thr = ((lut[:-1] + lut[1:]) * f32(0.5)).astype(f32)  # midpoints between neighbouring codes
            code = np.searchsorted(thr, exp[..., :3], side="left")
            exp = np.concatenate([lut[code], un[..., 3:]], -1).astype(f32)
        else:
            exp = un
    return exp.astype(f32)


def mip_chain(img, dt=f64):
    """all ceil(log2(max(w, h))) + 1 levels (gpu_uploader.rs:366) as arrays of the working type; the bytes are decided in float32"""
    lut = srgb_lut()
    levels = [decode_level0(img, lut)]
    count = int(math.ceil(math.log2(max(img.width, img.height)))) + 1
    for l in range(1, count):
        levels.append(mip_level_f32(levels[-1], img.width, img.height, l, img.format, lut))
    return [x.astype(dt) for x in levels]


def bilinear(level, u, v, dt):
    """linear filter with REPEAT on both axes (gpu_uploader.rs:341-353; the env map's sampler envmap.rs:201-211 is the same)"""
    h, w = level.shape[:2]
    x, y = u * dt(w) - dt(0.5), v * dt(h) - dt(0.5)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[:, None], (y - y0)[:, None]
    ix0, iy0 = np.mod(x0.astype(np.int64), w), np.mod(y0.astype(np.int64), h)
    ix1, iy1 = (ix0 + 1) % w, (iy0 + 1) % h
    one = dt(1)
    return (level[iy0, ix0] * (one - fx) + level[iy0, ix1] * fx) * (one - fy) + (level[iy1, ix0] * (one - fx) + level[iy1, ix1] * fx) * fy


def log2a(x, dt):
    """exponent + (mantissa - 1) of x as a float32: the spec's definition of log2 for the level of detail"""
    m, e = np.frexp(np.asarray(x, dtype=dt).astype(f32))  # x = m * 2^e, m in [0.5, 1)
    return (e - 1).astype(dt) + (m.astype(dt) * dt(2) - dt(1))


def texture_lod(lod_base, levels, dt):
    h, w = levels[0].shape[:2]
    return np.clip(lod_base + dt(0.5) * log2a(dt(w) * dt(h), dt), dt(0), dt(len(levels) - 1))


def trilinear(levels, u, v, lod, dt):
    l0 = np.floor(lod).astype(np.int64)
    fl = (lod - l0.astype(dt))[:, None]
    out = np.zeros((len(u), levels[0].shape[-1]), dt)
    for l in np.unique(l0):
        m = l0 == l
        a = bilinear(levels[l], u[m], v[m], dt)
        b = bilinear(levels[min(l + 1, len(levels) - 1)], u[m], v[m], dt)
        out[m] = a * (dt(1) - fl[m]) + b * fl[m]
    return out


def texture_of(scene, index):
    """the image a material's map index names: index < texture count, through texture -> image -> data; else None"""
    if index >= len(scene.texture2image_mapping) or index not in scene.texture2image_mapping:
        return None
    return scene.image_data[scene.image2data_mapping[scene.texture2image_mapping[index]]]


# ---- 6. surface (RENDER_SPEC 6.4, 7.4) ------------------------------------------------------------------------------------------------
def surface(scene, g, chains, o, d, hit, pixel_spread, dt=f64):
    """at the surface pixels `sel`: base, emission, ns, P, the base-colour map's lod (nan without one) and the normal-map fragility"""
    sel = np.flatnonzero(hit["kind"] == SURFACE)
    out = dict(sel=sel, base=np.zeros((len(sel), 3), dt), emission=np.zeros((len(sel), 3), dt), ns=np.zeros((len(sel), 3), dt),
               P=np.zeros((len(sel), 3), dt), lod=np.full(len(sel), np.nan), fragile=np.zeros(len(sel), bool))
    if not len(sel):
        return out
    tri, t, u, v = hit["prim"][sel], hit["t"][sel], hit["u"][sel], hit["v"][sel]
    o, d = o[sel], d[sel]
    w0 = dt(1) - u - v

    def lerp(x):  # fma(c, v, fma(b, u, a * w0)) for a per-corner attribute
        return x[tri, 0] * w0[:, None] + x[tri, 1] * u[:, None] + x[tri, 2] * v[:, None]
    A = g.A[g.inst[tri]]
    c0, c1, c2 = A[:, :, 0], A[:, :, 1], A[:, :, 2]
    k0, k1, k2 = np.cross(c1, c2), np.cross(c2, c0), np.cross(c0, c1)  # the columns of the cofactor matrix
    det = _dot(c0, k0)
    nl = lerp(g.n)
    ns = _norm(np.sign(det)[:, None] * (k0 * nl[:, 0:1] + k1 * nl[:, 1:2] + k2 * nl[:, 2:3]))
    e1, e2 = g.v[tri, 1] - g.v[tri, 0], g.v[tri, 2] - g.v[tri, 0]
    gcross = np.cross(e1, e2)
    world_area = np.sqrt(_dot(gcross, gcross))
    ng = gcross / world_area[:, None]
    out["P"] = o + d * t[:, None]
    mats = g.inst_mat[g.inst[tri]]
    base, emission = np.zeros((len(sel), 3), dt), np.zeros((len(sel), 3), dt)
    uv = lerp(g.uv)
    d1, d2 = g.uv[tri, 1] - g.uv[tri, 0], g.uv[tri, 2] - g.uv[tri, 0]
    uv_area = np.abs(d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0])
    foot = t * pixel_spread / np.maximum(np.abs(_dot(d, ng)), dt(0.1))
    with np.errstate(all="ignore"):
        ratio = (foot * foot * uv_area / world_area).astype(f32).astype(dt)
        lod_base = np.where((ratio > 0) & (ratio < 3.0e38), dt(0.5) * log2a(np.where(ratio > 0, ratio, 1), dt), dt(0))
    for mi in np.unique(mats):
        mat = scene.materials[mi]
        m = mats == mi
        base[m], emission[m] = _a(mat.base_color, dt), _a(mat.emission, dt)
        maps = [texture_of(scene, i) for i in (mat.base_color_map_index, mat.emission_map_index, mat.normal_map_index)]
        fetch = [None if img is None else trilinear(chains[id(img)], uv[m, 0], uv[m, 1], texture_lod(lod_base[m], chains[id(img)], dt), dt) for img in maps]
        if fetch[0] is not None:
            base[m] = base[m] * fetch[0][:, :3]
            out["lod"][m] = texture_lod(lod_base[m], chains[id(maps[0])], dt)
        if fetch[1] is not None:
            emission[m] = emission[m] * fetch[1][:, :3]
        if fetch[2] is not None:
            # tangent through the upper 3 x 3, Gram-Schmidt against ns, B = cross(ns, T), n = 2 rgb - 1
            tl = lerp(g.tg)[m]
            tw = c0[m] * tl[:, 0:1] + c1[m] * tl[:, 1:2] + c2[m] * tl[:, 2:3]
            n0 = ns[m]
            tw = tw - n0 * _dot(n0, tw)[:, None]
            t2 = _dot(tw, tw)
            with np.errstate(all="ignore"):
                T = tw / np.sqrt(t2)[:, None]
                B = np.cross(n0, T)
                nts = fetch[2][:, :3] * dt(2) - dt(1)
                nn = T * nts[:, 0:1] + B * nts[:, 1:2] + n0 * nts[:, 2:3]
                n2 = _dot(nn, nn)
                good = (t2 > 0) & (n2 > 0)
                ns[m] = np.where(good[:, None], nn / np.sqrt(n2)[:, None], n0)
            out["fragile"][m] = (t2 < DELTA) | (n2 < DELTA)
    # ng to the (mapped) shading normal's side, then both to face the ray
    ng = np.where((_dot(ns, ng) < 0)[:, None], -ng, ng)
    behind = _dot(ng, d) > 0
    ns = np.where(behind[:, None], -ns, ns)
    # 7.1e: a ray that arrives from behind has run its segment through the object's medium — EMISSIVE adds colour * density * t,
    # ABSORB dims what the vertex emits by exp(-density * t * (1 - colour)).  (This is where the sign of det in the normal transform
    # shows at a first hit: without it a mirrored object is entered from "behind".)
    for mi in np.unique(mats):
        md = scene.materials[mi].medium
        m = (mats == mi) & behind
        dist = (_a(md.density, dt) * t[m])[:, None]
        if md.type == 3:
            emission[m] = emission[m] + _a(md.color, dt) * dist
        elif md.type == 1:
            emission[m] = emission[m] * np.exp(-(dist * (dt(1) - _a(md.color, dt))))
    out["base"], out["emission"], out["ns"] = base, emission, ns
    return out


# ---- 7. miss (RENDER_SPEC 6.3, 7.3) ---------------------------------------------------------------------------------------------------
def miss_radiance(settings, d, dt=f64):
    k = _a(settings.env_intensity, dt)
    if settings.env is None:
        t = ((d[:, 1] + dt(1)) / dt(2))[:, None]
        return (_a(settings.ground, dt) * (dt(1) - t) + _a(settings.sky, dt) * t) * k
    env = settings.env.astype(dt)
    rotation = _a(settings.env_rotation, dt) / dt(360)  # the uniform carries degrees / 360 (rt_renderer.rs:420)
    u = (dt(math.pi) + np.arctan2(d[:, 2], d[:, 0])) / dt(2 * math.pi) + rotation
    v = np.arccos(np.clip(d[:, 1], dt(-1), dt(1))) / dt(math.pi)
    return bilinear(env, u, v, dt) * k


# ---- 8. outputs, folded over frames (RENDER_SPEC 8, 13) ------------------------------------------------------------------------------
class Result:
    pass


def render(scene, w, h, frames, settings=None, camera=0, dtype=f64):
    """images of frames 0 .. frames-1: albedo, normal, radiance [h, w, 3], position [h, w, 4], ids [h, w, 4] uint32 (frame 0), and per
    pixel: fragile in any frame, kinds [frames, h, w], lod of the base-colour map in frame 0"""
    dt = dtype
    settings = settings or Settings()
    world = world_transforms(scene, dt)
    g = triangles(scene, world, dt)
    ls = lights(scene, world, dt)
    chains = {id(img): mip_chain(img, dt) for img in scene.image_data}
    n = w * h
    r = Result()
    r.extent = g.extent
    r.fragile = np.zeros(n, bool)
    r.kinds = np.zeros((frames, n), np.int64)
    mean = dict(albedo=np.zeros((n, 3), dt), normal=np.zeros((n, 3), dt), radiance=np.zeros((n, 3), dt), position=np.zeros((n, 4), dt))
    for f in range(frames):
        o, d, spread = camera_rays(scene, world, camera, w, h, f, dt)
        hit = nearest_hit(g, ls, o, d, dt)
        sf = surface(scene, g, chains, o, d, hit, spread, dt)
        x = dict(albedo=np.zeros((n, 3), dt), normal=np.zeros((n, 3), dt), radiance=np.zeros((n, 3), dt), position=np.zeros((n, 4), dt))
        ids = np.full((n, 4), ABSENT, np.uint32)
        missed, lit, sel = hit["kind"] == MISS, np.flatnonzero(hit["kind"] == LIGHT), sf["sel"]
        # a miss and a light show min(radiance, 1) as albedo and no normal (RENDER_SPEC 6.2, 6.3)
        x["radiance"][missed] = miss_radiance(settings, d[missed], dt)
        for k, L in enumerate(ls):
            x["radiance"][lit[hit["light"][lit] == k]] = L.intensity
        x["albedo"] = np.minimum(x["radiance"], dt(1))
        x["albedo"][sel], x["normal"][sel], x["radiance"][sel] = sf["base"], sf["ns"], sf["emission"]
        x["position"][sel, :3], x["position"][sel, 3] = sf["P"], 1
        x["position"][lit, :3], x["position"][lit, 3] = o[lit] + d[lit] * hit["t"][lit][:, None], 1
        inst = g.inst[hit["prim"][sel]]
        ids[sel] = np.stack([g.inst_node[inst], inst, g.inst_mat[inst], hit["prim"][sel]], axis=-1).astype(np.uint32)
        ids[lit, 0] = g.light_node[hit["light"][lit]].astype(np.uint32)
        ids[lit, 3] = (0x80000000 | hit["light"][lit]).astype(np.uint32)
        r.fragile |= hit["fragile"]
        r.fragile[sel] |= sf["fragile"]
        r.kinds[f] = hit["kind"]
        for key in mean:  # mean_new = (mean_old * n + x) / (n + 1)
            mean[key] = (mean[key] * dt(f) + x[key]) / dt(f + 1)
        if f == 0:
            r.ids = ids.reshape(h, w, 4)
            r.lod = np.full(n, np.nan); r.lod[sel] = sf["lod"]
            r.lod = r.lod.reshape(h, w)
    for key, val in mean.items():
        setattr(r, key, val.reshape(h, w, -1))
    r.fragile = r.fragile.reshape(h, w)
    r.kinds = r.kinds.reshape(frames, h, w)
    return r
