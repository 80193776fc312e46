"""Plain-Python reference of the collapse of a binary hierarchy into 4-wide nodes (csrc/bvh_build.hip: k_collapse_cost, k_collapse_level).

costs() is the kernel's programme in binary32 with the kernel's order of operations; enumerate_cuts() lists every cut of at most
four elements of a small tree and prices each by the same sums, so the two minima must be the same bits (binary32 addition is
monotone: the minimum of the sums is the sum of the minima).  walk() fills the 4-nodes from the recorded choices as the level
launches do; check_tree() is what any correct collapse must satisfy, whatever it chose."""
import numpy as np

f32 = np.float32
LEAF = 0x80000000
ABSENT = 0xFFFFFFFF
C_NODE = f32(1.0)  # csrc/bvh_build.hip: kCollapseNodeCost
C_LEAF = f32(8.0)  # csrc/bvh_build.hip: RT_COLLAPSE_LEAF_COST (test_collapse_cost.py::test_constants_mirror_the_source)
INNER, SHIFT2, SHIFT3, SHIFT4 = 1, 2, 4, 6  # the choice word


def half_area(box):
    b = np.asarray(box, dtype=f32)
    dx, dy, dz = b[3] - b[0], b[4] - b[1], b[5] - b[2]
    return f32(f32(f32(dx * dy) + f32(dy * dz)) + f32(dz * dx))


class Tree:
    """A binary tree from a nested shape: an int is a leaf (its value is ignored), a pair (a, b) an inner node.  Leaves take the sorted
    positions 0 .. n - 1 from left to right, inner nodes are numbered in pre-order (the root is node 0: a parent's index is below its
    children's).  leaf_boxes [n, 6]; an inner node's box is the union of the leaf boxes below it unless node_boxes gives others."""

    def __init__(self, shape, leaf_boxes, node_boxes=None):
        self.left, self.right, self.first, self.last, self.node_parent = [], [], [], [], []
        self.leaf_parent = []
        self._build(shape, ABSENT)
        self.n = len(self.leaf_parent)
        self.leaf_boxes = np.ascontiguousarray(leaf_boxes, dtype=f32).reshape(self.n, 6)
        if node_boxes is None:
            node_boxes = np.array([np.concatenate([self.leaf_boxes[f:l + 1, :3].min(axis=0), self.leaf_boxes[f:l + 1, 3:].max(axis=0)])
                                   for f, l in zip(self.first, self.last)], dtype=f32)
        self.node_boxes = np.ascontiguousarray(node_boxes, dtype=f32).reshape(self.n - 1, 6)

    def _build(self, shape, parent):
        if not isinstance(shape, tuple):
            self.leaf_parent.append(parent)
            return LEAF | (len(self.leaf_parent) - 1)
        i = len(self.left)
        for a in (self.left, self.right, self.first, self.last):
            a.append(0)
        self.node_parent.append(parent)
        self.first[i] = len(self.leaf_parent)
        self.left[i] = self._build(shape[0], i)
        self.right[i] = self._build(shape[1], i)
        self.last[i] = len(self.leaf_parent) - 1
        return i

    def arrays(self):
        """the arguments of hala_renderer_amd.selftest_collapse, but for leaf_max"""
        return (self.left, self.right, self.node_parent, self.leaf_parent, self.first, self.last, self.node_boxes, self.leaf_boxes)

    def span(self, ref):
        return (ref & ~LEAF, ref & ~LEAF) if ref & LEAF else (self.first[ref], self.last[ref])

    def area(self, ref):
        return half_area(self.leaf_boxes[ref & ~LEAF]) if ref & LEAF else half_area(self.node_boxes[ref])


def costs(t, leaf_max):
    """-> (cost [n - 1, 3] float32 = C(node, 1 .. 3), choice [n - 1] uint32, keep [n - 1] uint32)"""
    ni = t.n - 1
    cost = np.zeros((ni, 3), dtype=f32)
    choice, keep = np.zeros(ni, dtype=np.uint32), np.zeros(ni, dtype=np.uint32)

    def of(ref):
        if ref & LEAF:
            return [f32(t.area(ref) * C_LEAF)] * 3
        return list(cost[ref])

    for p in range(ni - 1, -1, -1):  # pre-order numbering: children before parents
        L, R = of(t.left[p]), of(t.right[p])
        d2 = f32(L[0] + R[0])
        d3, k3 = f32(L[0] + R[1]), 1
        v = f32(L[1] + R[0])
        if v < d3:
            d3, k3 = v, 2
        d4, k4 = f32(L[0] + R[2]), 1
        v = f32(L[1] + R[1])
        if v < d4:
            d4, k4 = v, 2
        v = f32(L[2] + R[0])
        if v < d4:
            d4, k4 = v, 3
        area = t.area(p)
        as_leaf, as_inner = f32(area * C_LEAF), f32(f32(area * C_NODE) + d4)
        inner = not (t.last[p] - t.first[p] + 1 <= leaf_max and as_leaf <= as_inner)
        c1 = as_inner if inner else as_leaf
        open2 = d2 <= c1
        c2 = d2 if open2 else c1
        open3 = d3 <= c2
        c3 = d3 if open3 else c2
        cost[p] = (c1, c2, c3)
        choice[p] = (INNER if inner else 0) | ((1 if open2 else 0) << SHIFT2) | ((k3 if open3 else 0) << SHIFT3) | (k4 << SHIFT4)
        keep[p] = 1 if inner else 0
    return cost, choice, keep


def enumerate_cuts(t, leaf_max):
    """Every way to stand every subtree in at most j slots, listed one by one -> (cost of the root as a 4-node, number of cuts of the
    root looked at).  For tiny trees only: the lists grow with the number of cuts."""
    memo = {}

    def slot(ref):  # ref in one slot: a leaf where it may be one, else a 4-node over its cheapest cut
        if ref & LEAF:
            return f32(t.area(ref) * C_LEAF)
        if ("slot", ref) not in memo:
            opened = min(c for c, _ in cuts_opened(ref, 4))
            best = f32(f32(t.area(ref) * C_NODE) + opened)
            if t.last[ref] - t.first[ref] + 1 <= leaf_max:
                best = min(best, f32(t.area(ref) * C_LEAF))
            memo["slot", ref] = best
        return memo["slot", ref]

    def cuts_opened(ref, j):  # ref's children share j slots
        out = []
        for k in range(1, j):
            for cl, a in cuts(t.left[ref], k):
                for cr, b in cuts(t.right[ref], j - k):
                    out.append((f32(cl + cr), a + b))
        return out

    def cuts(ref, j):  # at most j slots
        if (ref, j) not in memo:
            out = [(slot(ref), (ref,))]
            if not ref & LEAF and j >= 2:
                out += cuts_opened(ref, j)
            memo[ref, j] = out
        return memo[ref, j]

    root = cuts_opened(0, 4)
    return f32(f32(t.area(0) * C_NODE) + min(c for c, _ in root)), len(set(cut for _, cut in root))


def walk(t, choice, keep):
    """-> refs4 [node_count, 4], breadth-first: the cut recorded for every 4-node, slots ordered as k_collapse_level orders them (kept
    inner children by descending area, stable; then the leaves as the walk left them)"""
    roots, rows = [0], []
    q = 0
    while q < len(roots):
        i = roots[q]
        q += 1
        out = []

        def stand(ref, slots):  # a child of an opened node in `slots` <= 3 slots
            while True:
                if ref & LEAF or slots == 1:
                    out.append(ref)
                    return
                k = (int(choice[ref]) >> {2: SHIFT2, 3: SHIFT3}[slots]) & 3
                if k == 0:  # as with one slot fewer
                    slots -= 1
                    continue
                stand(t.left[ref], k)
                ref, slots = t.right[ref], slots - k

        k4 = (int(choice[i]) >> SHIFT4) & 3
        stand(t.left[i], k4)
        stand(t.right[i], 4 - k4)
        assert 2 <= len(out) <= 4
        weight = [f32(-1.0) if (r & LEAF or not keep[r]) else half_area(t.node_boxes[r]) for r in out]
        for a in range(1, len(out)):  # the kernel's insertion sort
            b = a
            while b > 0 and weight[b] > weight[b - 1]:
                weight[b], weight[b - 1] = weight[b - 1], weight[b]
                out[b], out[b - 1] = out[b - 1], out[b]
                b -= 1
        rows.append(out + [ABSENT] * (4 - len(out)))
        roots += [r for r in out if not r & LEAF and keep[r]]
    return np.array(rows, dtype=np.uint32)


def check_tree(t, refs4, keep, leaf_max):
    """What every collapse must give: each 4-node a cut of its root (its children's sorted positions partition the root's), leaves of at
    most leaf_max triangles, every inner child the root of exactly one later 4-node, breadth-first.  -> children per 4-node"""
    roots, seen, leaves, children = [0], set(), [], 0
    assert len(refs4) >= 1
    for q, row in enumerate(np.asarray(refs4).tolist()):
        assert q < len(roots), "a 4-node no inner child leads to"
        present = [r for r in row if r != ABSENT]
        assert 2 <= len(present) <= 4 and row[len(present):] == [ABSENT] * (4 - len(present))
        children += len(present)
        spans = []
        for r in present:
            assert (r & ~LEAF) < (t.n if r & LEAF else t.n - 1)
            f, l = t.span(r)
            spans.append((f, l))
            if r & LEAF or not keep[r]:
                assert l - f + 1 <= leaf_max
                leaves.append((f, l))
            else:
                assert r not in seen, "an inner child referenced twice"
                seen.add(r)
                roots.append(r)
        spans.sort()
        f, l = t.span(roots[q])
        assert spans[0][0] == f and spans[-1][1] == l and all(a[1] + 1 == b[0] for a, b in zip(spans, spans[1:])), "not a cut of the root"
    assert len(roots) == len(refs4)
    leaves.sort()
    assert leaves[0][0] == 0 and leaves[-1][1] == t.n - 1 and all(a[1] + 1 == b[0] for a, b in zip(leaves, leaves[1:]))
    return children / len(refs4)


def tree_cost(t, refs4, keep):
    """the cost of a collapsed tree, summed in float64: an independent look at what the root cost says"""
    total = 0.0
    for row in np.asarray(refs4).tolist():
        for r in row:
            if r == ABSENT:
                continue
            total += float(t.area(r)) * float(C_LEAF if (r & LEAF or not keep[r]) else C_NODE)
    return total + float(t.area(0)) * float(C_NODE)


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------
def chain(n):
    """right-leaning: every inner node has a leaf on the left"""
    return (0, chain(n - 1)) if n > 2 else (0, 0)


def perfect(n):
    return 0 if n == 1 else (perfect(n // 2), perfect(n - n // 2))


def random_shape(rng, n):
    if n == 1:
        return 0
    k = int(rng.randint(1, n))
    return (random_shape(rng, k), random_shape(rng, n - k))


def random_boxes(rng, n, extent=0.3):
    """leaf boxes strung along x with some overlap, so that neighbours in sorted order are neighbours in space"""
    lo = np.stack([np.arange(n) * 0.2 + rng.rand(n) * 0.1, rng.rand(n), rng.rand(n)], axis=1)
    return np.concatenate([lo, lo + 0.02 + rng.rand(n, 3) * extent], axis=1).astype(f32)
