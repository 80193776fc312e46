"""numpy twin of the Cryptomatte ID mattes (docs/RENDER_SPEC.md 15): the MurmurHash3 name ids, the per-sample keys, the fold of the
per-pixel (id, count) records, the ranked output and the layer manifests.  The first hit of every sample comes from the oracle's camera rays
and closest hits through aov_ref.first_hits, the instance / light node tables from aov_ref.instance_table / light_nodes.

The fold is written differently from the kernel on purpose: a present id counts once more, a new one goes to the FIRST empty entry, then
every record is sorted again (count descending, id ascending, empty entries last); the kernel keeps the order with one bubble pass."""
import numpy as np

import aov_ref as A

f32, u32 = np.float32, np.uint32
LAYERS = ("object", "material", "asset")
LAYER_NAMES = ("CryptoObject", "CryptoMaterial", "CryptoAsset")
ENTRIES, RANKS = 7, 6


def murmur3_32(data: bytes, seed: int = 0) -> int:
    """MurmurHash3_x86_32"""
    m = 0xFFFFFFFF
    c1, c2 = 0xCC9E2D51, 0x1B873593

    def rotl(x, r):
        return ((x << r) | (x >> (32 - r))) & m

    h = seed & m
    n = len(data) // 4
    for i in range(n):
        k = int.from_bytes(data[4 * i:4 * i + 4], "little")
        k = (rotl((k * c1) & m, 15) * c2) & m
        h = (rotl(h ^ k, 13) * 5 + 0xE6546B64) & m
    tail = data[4 * n:]
    k = 0
    if len(tail) >= 3:
        k ^= tail[2] << 16
    if len(tail) >= 2:
        k ^= tail[1] << 8
    if len(tail) >= 1:
        k ^= tail[0]
        h ^= (rotl((k * c1) & m, 15) * c2) & m
    h ^= len(data) & m
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & m
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & m
    return h ^ (h >> 16)


def crypto_id(raw: int) -> int:
    """the stored id: bit 23 flipped when the exponent bits are 0 or 255"""
    return raw ^ (1 << 23) if ((raw >> 23) & 0xFF) in (0, 255) else raw


def name_id(name: str) -> int:
    return crypto_id(murmur3_32(name.encode("utf-8")))


def layer_key(layer_name: str) -> str:
    """<key> of the EXR attributes cryptomatte/<key>/...: the first 7 hex digits of the raw hash of the layer name"""
    return f"{murmur3_32(layer_name.encode('utf-8')):08x}"[:7]


def object_names(scene):
    return [nd.name if nd.name else f"node{k}" for k, nd in enumerate(scene.nodes)]


def root(scene, k):
    while scene.nodes[k].parent is not None and scene.nodes[k].parent >= 0:
        k = scene.nodes[k].parent
    return k


def material_names(scene, names=None):
    names = list(names or [])
    return [names[m] if m < len(names) and names[m] else f"material{m}" for m in range(len(scene.materials))]


def tables(scene, names=None):
    """(object id per node, asset id per node, material id per material), uint32"""
    obj = np.array([name_id(n) for n in object_names(scene)], u32)
    asset = np.array([obj[root(scene, k)] for k in range(len(scene.nodes))], u32)
    mat = np.array([name_id(n) for n in material_names(scene, names)], u32)
    return obj, asset, mat


def keys(ids, tabs, layer):
    """(has, key) of every sample's first-hit record ids [..., 4] (RENDER_SPEC 13) in `layer`"""
    obj, asset, mat = tabs
    node, material = ids[..., 0], ids[..., 2]
    if layer == "material":
        has = material != A.ABSENT
        return has, np.where(has, mat[np.where(has, material, 0)], 0).astype(u32)
    has = node != A.ABSENT
    t = obj if layer == "object" else asset
    return has, np.where(has, t[np.where(has, node, 0)], 0).astype(u32)


def empty(shape):
    return np.zeros(tuple(shape) + (16,), u32)


def fold(rec, has, key):
    """one sample per record: rec [..., 16], has / key [...]"""
    rec = rec.copy()
    ids, cnt = rec[..., 2::2].copy(), rec[..., 3::2].copy()
    rec[..., 0] += 1
    present = has[..., None] & (cnt > 0) & (ids == key[..., None])
    cnt += present.astype(u32)
    new = has & ~present.any(-1)
    free = cnt == 0
    room = new & free.any(-1)
    first = np.argmax(free, axis=-1)
    sel = np.nonzero(room)
    ids[sel + (first[sel],)] = key[sel]
    cnt[sel + (first[sel],)] = 1
    rec[..., 1] += (new & ~room).astype(u32)
    order = np.lexsort((ids, -cnt.astype(np.int64)), axis=-1)
    rec[..., 2::2] = np.take_along_axis(ids, order, -1)
    rec[..., 3::2] = np.take_along_axis(cnt, order, -1)
    return rec


def records(oracle, scene, w, h, frames, layers=LAYERS, names=None, snapshots=False):
    """{layer: [H, W, 16] uint32} after frames 0 .. frames-1 of camera 0 (snapshots: a list with the records after every frame)"""
    lights, _ = oracle.pack_lights(scene)
    osc = oracle.OracleScene(scene)
    tabs = tables(scene, names)
    rec = {layer: empty((h, w)) for layer in layers}
    out = []
    try:
        for f in range(frames):
            _, ids = A.first_hits(osc, scene, lights, w, h, f)
            for layer in layers:
                has, key = keys(ids, tabs, layer)
                rec[layer] = fold(rec[layer], has, key)
            if snapshots:
                out.append({k: v.copy() for k, v in rec.items()})
    finally:
        osc.close()
    return out if snapshots else rec


def rank(rec):
    """(ids float32 [..., 6], coverage float32 [..., 6]): rank r = (id_r as float bits, float(count_r) / float(n)), (0, 0) when empty"""
    n = rec[..., 0].astype(f32)
    ids = rec[..., 2:2 + 2 * RANKS:2]
    cnt = rec[..., 3:3 + 2 * RANKS:2]
    full = cnt > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        cov = np.where(full, cnt.astype(f32) / n[..., None], f32(0.0)).astype(f32)
    return np.where(full, ids, 0).astype(u32).view(f32), cov


def manifest(scene, layer, names=None):
    """{name: 8 hex digits} of every name the layer can produce: the nodes of the packed instances and lights (object), their roots
    (asset), every material (material)"""
    if layer == "material":
        ns = material_names(scene, names)
    else:
        inst_node, _, _ = A.instance_table(scene)
        nodes = [int(k) for k in inst_node] + [int(k) for k in A.light_nodes(scene)]
        obj = object_names(scene)
        ns = [obj[k if layer == "object" else root(scene, k)] for k in nodes]
    return {n: f"{name_id(n):08x}" for n in sorted(set(ns), key=lambda s: s.encode("utf-8"))}
