"""The numpy twin of docs/RENDER_SPEC.md 4.6 "Tree cost": the two integer sums of a tree, from the downloaded nodes and nothing else.
float32 throughout, every product and every sum a numpy operation of its own (no fused multiply-add), the sums in uint64."""
import numpy as np

f32 = np.float32
ABSENT = np.uint32(0xFFFFFFFF)
ONE = 1 << 32


def _quanta(exps):
    """[n] uint32 -> [n, 3] float32: 2^e per axis, the float whose exponent field is the axis's byte"""
    b = np.stack([(exps >> np.uint32(8 * a)) & np.uint32(0xFF) for a in range(3)], axis=-1).astype(np.uint32)
    return (b << np.uint32(23)).view(f32)


def _planes(words):
    """[n, 3] uint32 -> [n, 4 (child), 3 (axis)] int32: byte c of word a"""
    return np.stack([(words >> np.uint32(8 * c)) & np.uint32(0xFF) for c in range(4)], axis=1).astype(np.int32)


def _half_area(d):
    """[..., 3] float32 -> (dx * dy + dy * dz) + dz * dx, each operation rounded to float32"""
    xy = d[..., 0] * d[..., 1]
    yz = d[..., 1] * d[..., 2]
    zx = d[..., 2] * d[..., 0]
    return (xy + yz) + zx


def tree_cost(nodes, tree):
    """nodes: uint32 [n, 16] as hala_rt_download_bvh gives them; tree: (first, count).  -> (valid, node_q, tri_q) as Python ints"""
    first, count = int(tree[0]), int(tree[1])
    nd = np.ascontiguousarray(nodes, dtype=np.uint32).reshape(-1, 16)[first:first + count]
    assert len(nd) == count and count >= 1
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        quanta = _quanta(nd[:, 3])
        qlo, qhi = _planes(nd[:, 4:7]), _planes(nd[:, 7:10])
        ref = nd[:, 12:16]
        present = ref != ABSENT
        # the root: the extent of its present children's planes
        rp = present[0]
        if not rp.any():
            return 0, 0, 0
        D = (qhi[0][rp].max(axis=0) - qlo[0][rp].min(axis=0)).astype(f32) * quanta[0]
        h_root = _half_area(D)
        if not (h_root > 0):
            return 0, 0, 0
        d = (qhi - qlo).astype(f32) * quanta[:, None, :]
        h = _half_area(d)
        rho = h / f32(h_root)
        ok = present & (rho >= 0)  # (false for NaN)
        scaled = np.minimum(rho, f32(4.0)) * f32(4294967296.0)
        q = np.where(ok, scaled, f32(0.0)).astype(np.uint64)  # truncation
    leaf = present & ((ref & np.uint32(0x80000000)) != 0)
    inner = present & ~leaf
    counts = (((ref >> np.uint32(28)) & np.uint32(7)) + np.uint32(1)).astype(np.uint64)
    node_q = np.uint64(ONE) + q[inner].sum(dtype=np.uint64)
    tri_q = (q[leaf] * counts[leaf]).sum(dtype=np.uint64)
    return 1, int(node_q), int(tri_q)


def cost(nodes, tree):
    v, a, b = tree_cost(nodes, tree)
    return a + b
