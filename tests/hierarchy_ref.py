"""Plain numpy references of the three hierarchy builders (csrc/bvh_sah.hip, csrc/bvh_ploc.hip, and k_morton, the radix sort,
k_hierarchy and k_fit of csrc/bvh_build.hip), each written from the rule the builder states, not from the way its kernels work.

check_contract() is what every builder owes the collapse (bvh_build_impl.h: HierarchyJob), boxes bit for bit.  check_sah() takes every
node's ids from the tree under test and asks that the node was split at the cheapest (cost, axis, position) of a full sweep, with a
float64 guard that shares no rounding with it.  ploc_twin() and lbvh_twin() build the one tree their rule allows, serially and top-down.
All binary32 arithmetic is one numpy operation per rounding (numpy fuses nothing, like a build with -ffp-contract=off).

A deliberate change to a builder's rule changes this file in the same commit ("Hierarchy builders")."""
import numpy as np

f32 = np.float32
LEAF = 0x80000000
ABSENT = 0xFFFFFFFF

# mirrored from the sources; test_hierarchy_builders.py::test_constants_mirror_the_source says which one moved
SAH_QUANT = 4          # bvh_sah.hip: kSahQuant
SWEEP_ROUNDS = 64      # bvh_sah.hip: kSweepRounds
PLOC_RADIUS = 16       # bvh_ploc.hip: kPlocRadius
PLOC_TAIL = 512        # bvh_ploc.hip: kPlocTail
CLASS_RATIO2 = (f32(1.0) / f32(64.0), f32(1.0) / f32(1024.0), f32(1.0) / f32(16384.0))  # bvh_build.hip: k_morton's size classes
AXIS_BITS = 20         # bvh_build.hip: k_morton, bits per axis


def as_boxes(boxes):
    b = np.ascontiguousarray(boxes, dtype=f32)
    assert b.ndim == 2 and b.shape[1] == 6
    return b


def f2ord(x):
    """float32 -> uint32 that orders like the floats"""
    u = np.ascontiguousarray(x, dtype=f32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def bits(x):
    return np.ascontiguousarray(x, dtype=f32).view(np.uint32)


def half_area(b):
    """[..., 6] float32 -> (dx * dy + dy * dz) + dz * dx, every operation rounded to float32"""
    b = np.asarray(b, dtype=f32)
    dx, dy, dz = b[..., 3] - b[..., 0], b[..., 4] - b[..., 1], b[..., 5] - b[..., 2]
    return (dx * dy + dy * dz) + dz * dx


def half_area64(b):
    b = np.asarray(b, dtype=np.float64)
    dx, dy, dz = b[..., 3] - b[..., 0], b[..., 4] - b[..., 1], b[..., 5] - b[..., 2]
    return dx * dy + dy * dz + dz * dx


def union(a, b):
    a, b = np.asarray(a, dtype=f32), np.asarray(b, dtype=f32)
    return np.concatenate([np.minimum(a[..., :3], b[..., :3]), np.maximum(a[..., 3:], b[..., 3:])], axis=-1)


def union_of(boxes):
    """[k, 6] -> [6]: min and max are exact, the order does not matter"""
    return np.concatenate([boxes[:, :3].min(axis=0), boxes[:, 3:].max(axis=0)])


def widen(b, pad):
    """one float32 addition per component"""
    b = np.asarray(b, dtype=f32)
    return np.concatenate([b[..., :3] - f32(pad), b[..., 3:] + f32(pad)], axis=-1).astype(f32)


def build_pad(boxes):
    """the pad a build takes for these boxes (RENDER_SPEC 4.1b): 2^-19 of the largest coordinate"""
    return f32(np.abs(as_boxes(boxes)).max() * f32(1.9073486328125e-06))


# ---- the contract -------------------------------------------------------------------------------------------------------------------------
class Tree:
    """the arrays hala_rt_selftest_hierarchy returns"""
    FIELDS = ("sorted_ids", "left", "right", "first", "last", "node_parent", "leaf_parent", "node_boxes")

    def __init__(self, arrays):
        for k in self.FIELDS:
            setattr(self, k, np.array(arrays[k]))
        self.n = len(self.sorted_ids)

    def arrays(self):
        return {k: getattr(self, k).copy() for k in self.FIELDS}

    def span(self, ref):
        ref = int(ref)
        return (ref & ~LEAF, ref & ~LEAF) if ref & LEAF else (int(self.first[ref]), int(self.last[ref]))

    def depths(self):
        """depth of every inner node, the root at 0 (after check_contract: parents have been followed)"""
        d = np.full(self.n - 1, -1, dtype=np.int64)
        d[0] = 0
        todo = [0]
        while todo:
            i = todo.pop()
            for c in (int(self.left[i]), int(self.right[i])):
                if not c & LEAF:
                    d[c] = d[i] + 1
                    todo.append(c)
        return d

    def canonical(self):
        """the tree without its numbering: the ids in depth-first order and the sorted positions of the inner nodes in pre-order, with the
        node each came from.  Two trees nest the same ids the same way, left and right, exactly when both lists agree."""
        ids, spans, names = [], [], []
        todo = [0]
        while todo:
            r = todo.pop()
            if r & LEAF:
                ids.append(int(self.sorted_ids[r & ~LEAF]))
                continue
            spans.append((len(ids), int(self.last[r]) - int(self.first[r]) + 1))
            names.append(r)
            todo.append(int(self.right[r]))
            todo.append(int(self.left[r]))
        return ids, spans, names


def check_contract(tree, boxes, pad):
    """HierarchyJob's "out": node 0 is the root; every other node and every sorted position is some node's child exactly once and names
    that node as its parent; a node's sorted positions are its left child's followed by its right child's; sorted_ids is a permutation;
    node_boxes are the unions of the boxes below, widened, bit for bit.  The message of a failure names the node."""
    t, n = tree, tree.n
    boxes = as_boxes(boxes)
    assert n == len(boxes) >= 2
    for k in Tree.FIELDS:
        assert len(getattr(t, k)) == (n if k in ("sorted_ids", "leaf_parent") else n - 1), k
    ids = t.sorted_ids.astype(np.int64)
    assert ids.min() >= 0 and ids.max() < n and len(np.unique(ids)) == n, "sorted_ids is not a permutation of the ids"
    assert int(t.node_parent[0]) == ABSENT, "node 0 is not the root: it has a parent"
    node_refs, leaf_refs = np.zeros(n - 1, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for i in range(n - 1):
        sp = []
        for side, ref in (("left", int(t.left[i])), ("right", int(t.right[i]))):
            c = ref & ~LEAF
            if ref & LEAF:
                assert c < n, f"node {i}: {side} leaf {c} out of range"
                assert int(t.leaf_parent[c]) == i, f"node {i}: its {side} leaf {c} names parent {int(t.leaf_parent[c])}"
                leaf_refs[c] += 1
            else:
                assert 0 < c < n - 1, f"node {i}: {side} child {c} out of range (or the root)"
                assert int(t.node_parent[c]) == i, f"node {i}: its {side} child {c} names parent {int(t.node_parent[c])}"
                node_refs[c] += 1
            sp.append(t.span(ref))
        (lf, ll), (rf, rl) = sp
        f, l = int(t.first[i]), int(t.last[i])
        assert 0 <= f <= l < n, f"node {i}: range {f} .. {l}"
        assert lf <= ll and rf <= rl and f == lf and ll + 1 == rf and l == rl, \
            f"node {i}: range {f} .. {l} is not left {lf} .. {ll} followed by right {rf} .. {rl}"
    assert (int(t.first[0]), int(t.last[0])) == (0, n - 1), "the root does not hold every sorted position"
    bad = np.nonzero(node_refs[1:] != 1)[0]
    assert len(bad) == 0, f"node {bad[0] + 1 if len(bad) else 0} is the child of {node_refs[bad[0] + 1] if len(bad) else 0} nodes"
    bad = np.nonzero(leaf_refs != 1)[0]
    assert len(bad) == 0, f"sorted position {bad[0] if len(bad) else 0} is the child of {leaf_refs[bad[0]] if len(bad) else 0} nodes"
    # ranges shrink strictly towards the leaves, so every node referenced once hangs below the root: nothing is detached
    by_pos = boxes[ids]
    for i in range(n - 1):
        want = widen(union_of(by_pos[int(t.first[i]):int(t.last[i]) + 1]), pad)
        got = np.asarray(t.node_boxes[i], dtype=f32)
        assert bits(got).tolist() == bits(want).tolist(), f"node {i}: box {got.tolist()} is not the widened union {want.tolist()} of its boxes"


# ---- SAH: every node split at the optimum of the full sweep ---------------------------------------------------------------------------------
def sah_orders(boxes):
    """per axis: the ordered-integer key of twice the centroid, in float32"""
    b = as_boxes(boxes)
    return [f2ord(b[:, a] + b[:, 3 + a]) for a in range(3)]


def sah_candidates(boxes, keys, ids, quant=SAH_QUANT):
    """Every split of the id set: per axis the ids ordered by (key, id), and for i = 1 .. m - 1 the boxes of the first i and of the
    rest.  -> list per axis of (order [m], L [m - 1, 6], R [m - 1, 6], nl [m - 1], nr [m - 1]): nl, nr = the counts in units of quant,
    rounded up"""
    ids = np.asarray(ids, dtype=np.int64)
    m = len(ids)
    i = np.arange(1, m)
    nl, nr = (i + quant - 1) // quant, (m - i + quant - 1) // quant
    out = []
    for a in range(3):
        order = ids[np.lexsort((ids, keys[a][ids]))]
        bx = boxes[order]
        lo = np.minimum.accumulate(bx[:, :3], axis=0)
        hi = np.maximum.accumulate(bx[:, 3:], axis=0)
        rlo = np.minimum.accumulate(bx[::-1, :3], axis=0)[::-1]
        rhi = np.maximum.accumulate(bx[::-1, 3:], axis=0)[::-1]
        out.append((order, np.concatenate([lo[:-1], hi[:-1]], axis=1), np.concatenate([rlo[1:], rhi[1:]], axis=1), nl, nr))
    return out


def sah_cost32(L, R, nl, nr):
    """area(L) * ceil(|L| / q) + area(R) * ceil(|R| / q) in float32: two products, one sum"""
    return half_area(L) * nl.astype(f32) + half_area(R) * nr.astype(f32)


def sah_cost64(L, R, nl, nr):
    return half_area64(L) * nl + half_area64(R) * nr


def sah_best(boxes, keys, ids, quant=SAH_QUANT):
    """-> (axis, i, left ids as the axis orders them, cost float32, cheapest float64 cost of any split): the minimum of
    (cost bits, axis, i)"""
    best, low64 = None, np.inf
    for a, (order, L, R, nl, nr) in enumerate(sah_candidates(boxes, keys, ids, quant)):
        c = sah_cost32(L, R, nl, nr)
        cb = bits(c)
        k = int(np.argmin(cb))  # the first of equal costs: the lowest i
        if best is None or int(cb[k]) < best[0]:
            best = (int(cb[k]), a, k + 1, order[:k + 1], c[k])
        low64 = min(low64, float(sah_cost64(L, R, nl, nr).min()))
    return best[1], best[2], best[3], best[4], low64


def sah_halving(boxes, keys, ids):
    """past the sweep rounds: the first half (rounded down) of the ids in axis-0 (key, id) order"""
    ids = np.asarray(ids, dtype=np.int64)
    order = ids[np.lexsort((ids, keys[0][ids]))]
    return order[:len(ids) // 2]


GUARD = 1.0 + 2.0 ** -20


def check_sah(tree, boxes, quant=SAH_QUANT, sweep_rounds=SWEEP_ROUNDS):
    """After check_contract.  Every inner node is judged on its own ids (sorted_ids[first .. last] of the tree under test), so that a
    wrong node does not condemn its subtree.  Above depth sweep_rounds: its left child holds exactly the ids the cheapest
    (cost bits, axis, i) puts there, and the split it took costs, in float64, no more than (1 + 2^-20) times the cheapest float64 cost
    of any split (a float32 cost is two products of a three-term sum, one more sum: under eight roundings of 2^-24 each on terms
    that are all >= 0, twice over for the two costs compared).  From that depth on: the first half in axis-0 order, and since
    every split below is along axis 0 too, the node's positions are literally in axis-0 (key, id) order in the finished sorted_ids.
    Above that depth the ids inside a range stand left child first at every level below, so the sets fix sorted_ids altogether: no
    order inside a range is asked there (a later split along another axis re-orders what axis 0 ordered).  -> the deepest node's depth"""
    boxes = as_boxes(boxes)
    keys = sah_orders(boxes)
    ids_at = tree.sorted_ids.astype(np.int64)
    depth = tree.depths()
    by_pos = boxes[ids_at]
    for i in range(tree.n - 1):
        f, l = int(tree.first[i]), int(tree.last[i])
        k = tree.span(tree.left[i])[1] + 1  # first position of the right child
        ids = ids_at[f:l + 1]
        got = np.sort(ids_at[f:k])
        where = f"node {i} (depth {int(depth[i])}, positions {f} .. {l}, split at {k})"
        if depth[i] >= sweep_rounds:
            assert k == f + (l + 1 - f) // 2, f"{where}: past the sweep rounds a node is halved"
            want = np.sort(sah_halving(boxes, keys, ids))
            assert np.array_equal(got, want), f"{where}: the left half is not the first half in axis-0 order"
            in_order = ids[np.lexsort((ids, keys[0][ids]))]
            assert np.array_equal(ids, in_order), f"{where}: its positions are not in axis-0 (key, id) order"
            continue
        axis, at, left, cost, low64 = sah_best(boxes, keys, ids, quant)
        nl, nr = np.array([(k - f + quant - 1) // quant]), np.array([(l + 1 - k + quant - 1) // quant])
        took64 = float(sah_cost64(union_of(by_pos[f:k])[None], union_of(by_pos[k:l + 1])[None], nl, nr)[0])
        assert took64 <= low64 * GUARD, f"{where}: the split costs {took64!r}, the cheapest split {low64!r} (float64)"
        assert k - f == at and np.array_equal(got, np.sort(left)), \
            f"{where}: the cheapest (cost, axis, i) is ({float(cost)!r}, {axis}, {at}) with left ids {np.sort(left)[:8].tolist()}..., the node has i = {k - f} and {got[:8].tolist()}..."
    return int(depth.max())


def sah_enumerate64(boxes, ids, quant=SAH_QUANT):
    """every split of every axis, one by one, in float64 from the float32 boxes -> [(cost, axis, i, left ids)] (tiny sets only)"""
    b = as_boxes(boxes)
    out = []
    for a in range(3):
        order = sorted((int(x) for x in ids), key=lambda t: (float(f32(b[t, a] + b[t, 3 + a])), t))
        for i in range(1, len(order)):
            L, R = b[order[:i]].astype(np.float64), b[order[i:]].astype(np.float64)

            def area(x):
                d = x[:, 3:].max(axis=0) - x[:, :3].min(axis=0)
                return d[0] * d[1] + d[1] * d[2] + d[2] * d[0]
            out.append((area(L) * -(-i // quant) + area(R) * -(-(len(order) - i) // quant), a, i, order[:i]))
    return out


# ---- Morton order ---------------------------------------------------------------------------------------------------------------------------
def spread(v, bits_per_axis=AXIS_BITS):
    """bit k of v -> bit 3 k"""
    v = np.asarray(v, dtype=np.uint64)
    out = np.zeros_like(v)
    for k in range(bits_per_axis + 1):
        out |= ((v >> np.uint64(k)) & np.uint64(1)) << np.uint64(3 * k)
    return out


def morton_keys(boxes):
    """-> (keys uint64, size class uint32).  The scene bounds are the exact union of the boxes.  Per axis, all in float32:
    t = clamp((0.5 * (mn + mx) - lo) / (hi - lo), 0, 1), 0 where the axis has no extent; q = min(trunc(t * 2^20), 2^20 - 1); x in bits
    3 k + 2, y in 3 k + 1, z in 3 k.  The class (bits 60 ..) compares the squared diagonals of box and scene: 0 above 1/64, 1 above 1/1024,
    2 above 1/16384, else 3; 3 when the scene has no extent at all."""
    b = as_boxes(boxes)
    n = len(b)
    lo, hi = b[:, :3].min(axis=0), b[:, 3:].max(axis=0)
    key = np.zeros(n, dtype=np.uint64)
    scene_d2, box_d2 = f32(0.0), np.zeros(n, dtype=f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        for a in range(3):
            c = f32(0.5) * (b[:, a] + b[:, 3 + a])
            ext = f32(hi[a] - lo[a])
            t = (c - lo[a]) / ext if ext > 0 else np.zeros(n, dtype=f32)
            t = np.minimum(np.maximum(t, f32(0.0)), f32(1.0))
            q = np.minimum((t * f32(1 << AXIS_BITS)).astype(np.uint32), np.uint32((1 << AXIS_BITS) - 1))
            key |= spread(q) << np.uint64(2 - a)
            scene_d2 = f32(scene_d2 + ext * ext)
            side = b[:, 3 + a] - b[:, a]
            box_d2 = box_d2 + side * side
        ratio2 = box_d2 / scene_d2 if scene_d2 > 0 else np.zeros(n, dtype=f32)
    cls = np.where(ratio2 > CLASS_RATIO2[0], 0, np.where(ratio2 > CLASS_RATIO2[1], 1, np.where(ratio2 > CLASS_RATIO2[2], 2, 3))).astype(np.uint32)
    return key | (cls.astype(np.uint64) << np.uint64(60)), cls


def morton_order(boxes):
    """-> (ids in Morton order, their keys): a stable sort by key, ties in id order"""
    keys, _ = morton_keys(boxes)
    order = np.argsort(keys, kind="stable")
    return order.astype(np.uint32), keys[order]


# ---- LBVH: Karras' hierarchy, top-down ----------------------------------------------------------------------------------------------------------
def lbvh_from_keys(keys):
    """Sorted keys -> (left, right, first, last) as lists.  A range first .. last splits at the highest bit in which its first and last
    augmented key differ (the key, then the position: equal keys differ in their positions): the left part is every entry that has
    that bit clear.  Its parts are node `split` (the last position of the left part) and node split + 1, or those leaves."""
    keys = [int(k) for k in keys]
    n = len(keys)
    left, right, first, last = ([0] * (n - 1) for _ in range(4))
    todo = [(0, 0, n - 1)]
    while todo:
        node, f, l = todo.pop()
        if keys[f] != keys[l]:
            bit = (keys[f] ^ keys[l]).bit_length() - 1
            split = max(p for p in range(f, l + 1) if not (keys[p] >> bit) & 1) if l - f < 8 else _last_clear(keys, f, l, bit)
        else:
            bit = (f ^ l).bit_length() - 1
            split = ((l >> bit) << bit) - 1
        assert f <= split < l
        first[node], last[node] = f, l
        for side, (a, b, name) in ((left, (f, split, split)), (right, (split + 1, l, split + 1))):
            if a == b:
                side[node] = LEAF | a
            else:
                side[node] = name
                todo.append((name, a, b))
    return left, right, first, last


def _last_clear(keys, f, l, bit):
    """the last position in f .. l whose key has `bit` clear; the keys are sorted and agree above it, so the clear ones come first"""
    while f < l:
        mid = (f + l + 1) // 2
        if (keys[mid] >> bit) & 1:
            l = mid - 1
        else:
            f = mid
    return f


def lbvh_twin(boxes, pad=0.0):
    """-> Tree: what LBVH must return, numbering included"""
    order, keys = morton_order(boxes)
    left, right, first, last = lbvh_from_keys(keys)
    return complete(dict(sorted_ids=order, left=left, right=right, first=first, last=last), boxes, pad)


# ---- PLOC, serially -------------------------------------------------------------------------------------------------------------------------------
def ploc_nearest(cl_boxes, radius=PLOC_RADIUS):
    """[m, 6] -> [m]: for every cluster the one within `radius` positions whose union with it has the smallest float32 half area, the
    lowest position among equals (m >= 2)"""
    m = len(cl_boxes)
    off = np.array([d for d in range(-radius, radius + 1) if d != 0])
    j = np.arange(m)[:, None] + off[None, :]
    ok = (j >= 0) & (j < m)
    jc = np.clip(j, 0, m - 1)
    area = half_area(union(cl_boxes[:, None, :], cl_boxes[jc]))
    assert np.isfinite(area).all()
    area = np.where(ok, area, np.inf)
    return jc[np.arange(m), np.argmin(area, axis=1)]  # argmin: the first of equals, positions ascend along the row


def ploc_nearest_brute(cl_boxes, radius):
    """the same by a search over all pairs"""
    m = len(cl_boxes)
    out = []
    for i in range(m):
        cand = [(float(half_area(union(cl_boxes[i], cl_boxes[j]))), j) for j in range(m) if j != i and abs(i - j) <= radius]
        out.append(min(cand)[1])
    return np.array(out)


def ploc_twin(boxes, pad=0.0, radius=PLOC_RADIUS):
    """-> Tree in a numbering of its own (compare canonical()): clusters start as the boxes in Morton order; every round each finds
    its nearest, mutual pairs merge at the lower position (lower = left child) and the upper leaves the list; until one is left.
    sorted_ids is the depth-first order of the finished tree."""
    b = as_boxes(boxes)
    n = len(b)
    order, _ = morton_order(b)
    refs = [LEAF | k for k in range(n)]  # leaves by Morton position, inner nodes numbered as they are made
    cl = b[order].copy()
    left, right = [], []
    while len(refs) > 1:
        nn = ploc_nearest(cl, radius)
        i = np.arange(len(refs))
        mutual = nn[nn] == i
        lower = np.nonzero(mutual & (i < nn))[0]
        assert len(lower) >= 1  # the closest pair of all is mutual
        for p in lower.tolist():
            left.append(refs[p]); right.append(refs[int(nn[p])])
            refs[p] = len(left) - 1
        cl[lower] = union(cl[lower], cl[nn[lower]])
        keep = ~(mutual & (i > nn))
        cl = cl[keep]
        refs = [r for r, k in zip(refs, keep.tolist()) if k]
    # renumber: the root becomes node 0 (pre-order), leaves take their depth-first positions
    root = refs[0]
    size, post, stack = {}, [], [root]
    while stack:  # sizes bottom-up without recursion
        r = stack.pop()
        post.append(r)
        if not r & LEAF:
            stack += [left[r], right[r]]
    for r in reversed(post):
        size[r] = 1 if r & LEAF else size[left[r]] + size[right[r]]
    new_id, made, sorted_ids = {}, [], np.zeros(n, dtype=np.uint32)
    L, R, F, La = ([0] * (n - 1) for _ in range(4))
    todo = [(root, 0)]
    while todo:
        r, at = todo.pop()
        if r & LEAF:
            sorted_ids[at] = order[r & ~LEAF]
            continue
        i = new_id.setdefault(r, len(new_id))
        F[i], La[i] = at, at + size[r] - 1
        made.append((i, r))
        todo.append((right[r], at + size[left[r]]))
        todo.append((left[r], at))
    for i, r in made:
        L[i] = LEAF | F[i] if left[r] & LEAF else new_id[left[r]]
        R[i] = LEAF | La[i] if right[r] & LEAF else new_id[right[r]]
    return complete(dict(sorted_ids=sorted_ids, left=L, right=R, first=F, last=La), b, pad)


def ploc_chain(boxes, pad=0.0):
    """What ploc_twin gives where every box is the same box, in closed form (n - 1 rounds of the twin are too many for thousands of
    boxes).  All Morton keys are equal, so the stable sort leaves the ids as they are.  Every union has the same area, so every
    cluster's nearest is the lowest position of its window: position 1 for cluster 0, position 0 for clusters 1 .. radius, position
    i - radius beyond, whatever the radius.  Only 0 and 1 choose each other: each round merges exactly them, the merged cluster
    stays at position 0 with the same box, and the next round is the same with one cluster fewer.  The tree is the left-deep chain
    ((((0, 1), 2), 3), ...) and its depth-first order is 0 .. n - 1."""
    b = as_boxes(boxes)
    n = len(b)
    assert (bits(b) == bits(b[0])).all(), "ploc_chain: the boxes differ"
    # pre-order from the root: node k holds positions 0 .. n - 1 - k; its left child is node k + 1 (the leaf 0 below the last), its right the leaf n - 1 - k
    left = [k + 1 if k + 1 < n - 1 else LEAF | 0 for k in range(n - 1)]
    right = [LEAF | (n - 1 - k) for k in range(n - 1)]
    return complete(dict(sorted_ids=np.arange(n), left=left, right=right, first=[0] * (n - 1), last=[n - 1 - k for k in range(n - 1)]), b, pad)


def complete(d, boxes, pad):
    """sorted_ids, left, right, first, last -> Tree: the parents and the widened boxes follow from them"""
    b = as_boxes(boxes)
    n = len(b)
    u = lambda x: np.array(x, dtype=np.uint32)  # noqa: E731
    P, LP = [ABSENT] * (n - 1), [0] * n
    for i in range(n - 1):
        for c in (int(d["left"][i]), int(d["right"][i])):
            if c & LEAF:
                LP[c & ~LEAF] = i
            else:
                P[c] = i
    by_pos = b[np.asarray(d["sorted_ids"]).astype(np.int64)]
    node_boxes = np.array([widen(union_of(by_pos[int(f):int(l) + 1]), pad) for f, l in zip(d["first"], d["last"])], dtype=f32)
    return Tree(dict(sorted_ids=u(d["sorted_ids"]), left=u(d["left"]), right=u(d["right"]), first=u(d["first"]), last=u(d["last"]),
                     node_parent=u(P), leaf_parent=u(LP), node_boxes=node_boxes))


def same_nesting(got, want):
    """the two trees hold the same ids nested the same way; the message names the first node of `got` (pre-order) that does not"""
    gi, gs, gn = got.canonical()
    wi, ws, _ = want.canonical()
    for k, (a, b) in enumerate(zip(gs, ws)):
        assert a == b, f"node {gn[k]}: it holds {a[1]} ids from depth-first position {a[0]}, the reference's node there {b[1]} from {b[0]}"
    assert len(gs) == len(ws)
    bad = [k for k, (a, b) in enumerate(zip(gi, wi)) if a != b]
    assert not bad, f"depth-first position {bad[0]}: id {gi[bad[0]]}, the reference has {wi[bad[0]]} ({len(bad)} positions differ)"
