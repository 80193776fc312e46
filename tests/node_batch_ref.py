"""The node hierarchy of RENDER_SPEC 20 restated in numpy float32: world = mul(parent.world, local) in the operation order of
csrc/host_scene.cpp::mul (column c of the product = ((A.x * b.x + A.y * b.y) + A.z * b.z) + A.w * b.w, no fused multiply-add), one pass
in node order with parents before their children.  tests/test_node_batch.py pins it against the oracle's orc_update_node_hierarchies
byte for byte and reads its GPU expectations off it."""
import numpy as np

f32 = np.float32


def mul(a, b):
    """[4, 4] x [4, 4], row-major views of the column-major matrices: element (row, c) summed over k = 0..3 in that order, in float32"""
    a = np.asarray(a, dtype=f32)
    b = np.asarray(b, dtype=f32)
    acc = a[:, 0:1] * b[0:1, :]
    for k in (1, 2, 3):
        acc = (acc + a[:, k:k + 1] * b[k:k + 1, :]).astype(f32)
    return acc


def worlds(parents, locals_):
    """parents: per node the parent's index, or -1 / None for a root; locals_: [n, 4, 4] row-major -> [n, 4, 4] row-major world matrices"""
    locals_ = np.asarray(locals_, dtype=f32)
    out = np.empty_like(locals_)
    for k, p in enumerate(parents):
        if p is None or p < 0:
            out[k] = locals_[k]
        else:
            assert p < k, "parents come before their children"
            out[k] = mul(out[p], locals_[k])
    return out


def column_major(m):
    """[n, 4, 4] row-major -> [n, 16] column-major floats, as the C ABI and a device array hold them"""
    return np.ascontiguousarray(np.asarray(m, dtype=f32).transpose(0, 2, 1)).reshape(-1, 16)
