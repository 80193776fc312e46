"""The three hierarchy builders behind HierarchyJob (csrc/bvh_sah.hip, csrc/bvh_ploc.hip, and k_morton + radix sort + k_hierarchy + k_fit of
csrc/bvh_build.hip) against the references of hierarchy_ref.py, through hala_rt_selftest_hierarchy.

Without a GPU: the references against brute force on tiny inputs, the contract checker against mutants of a valid tree, the refusals
and the declarations of the entry point.  On the GPU: every builder at the sizes where its paths change, on box sets that are random,
coincident, flat, of every Morton size class, and deeper than the SAH sweep goes: the contract, the exact tree (LBVH, PLOC) or the
per-node optimum (SAH), the same bytes from a second call, and the tree accepted by hala_rt_selftest_collapse."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hierarchy_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hala-renderer_amd", "csrc")
gpu = pytest.mark.gpu
f32 = np.float32
SAH, PLOC, LBVH = 1, 2, 3
NAMES = {SAH: "sah", PLOC: "ploc", LBVH: "lbvh"}


# ---- box sets ---------------------------------------------------------------------------------------------------------------------------------
def soup_triangles(n):
    """n random triangles inside the unit cube (the recipe of test_gpu_parity.py::small_scene) -> [n, 3, 3] float32"""
    rs = np.random.RandomState(7000 + n)
    return (rs.uniform(0.15, 0.85, (n, 1, 3)) + rs.uniform(-0.15, 0.15, (n, 3, 3))).astype(f32)


def soup(n):
    pos = soup_triangles(n)
    return np.concatenate([pos.min(axis=1), pos.max(axis=1)], axis=1)


def coincident(n):
    return np.tile(np.array([0.25, 0.5, 0.75, 0.5, 1.0, 1.25], dtype=f32), (n, 1))


def flat_grid(n):
    """quarter-unit squares of no thickness, edge to edge in the plane z = 0: one axis without extent, every area equal"""
    w = int(np.ceil(np.sqrt(n)))
    k = np.arange(n)
    x, y, z = (k % w) * 0.25, (k // w) * 0.25, np.zeros(n)
    return np.stack([x, y, z, x + 0.25, y + 0.25, z], axis=1).astype(f32)


def size_classes(n):
    """box 0 is the scene's size; the others are cubes inside it whose edge, as a fraction of the scene's, falls into class 1, 2, 3, 0, 1, ..."""
    rs = np.random.RandomState(9100 + n)
    edge = np.array([0.06, 0.015, 0.003, 0.2])[np.arange(n) % 4] * rs.uniform(0.8, 1.2, n)
    c = rs.uniform(0.15, 0.85, (n, 3))
    b = np.concatenate([c - edge[:, None] / 2, c + edge[:, None] / 2], axis=1)
    b[0] = (0, 0, 0, 1, 1, 1)
    return b.astype(f32)


def pile():
    """500 coincident boxes among 100 random ones: the SAH sweep peels the pile kSahQuant at a time until kSweepRounds, then halves.
    The pile's extents are powers of two: its area times a small count is exact, so every split at a multiple of kSahQuant costs the
    same bits and the lowest wins (with an area that rounds, the products break the tie and the sweep takes larger bites)"""
    rs = np.random.RandomState(77)
    b = np.concatenate([soup(100), np.tile(np.array([0.375, 0.375, 0.375, 0.625, 0.5, 0.5], dtype=f32), (500, 1))])
    return b[rs.permutation(len(b))]


SETS = {"soup": soup, "coincident": coincident, "flat_grid": flat_grid, "size_classes": size_classes}
# one node | PLOC's radius and its double, +- 1 | a wave | a block | kPlocTail, +- 1 | several blocks and several SAH rounds
SIZES = (2, 3, 5, 17, 18, 33, 34, 64, 65, 256, 257, 512, 513, 1030, 4100)
CASES = [(s, n, b) for s in SETS for n in SIZES for b in (SAH, PLOC, LBVH)]
# PLOC merges ONE pair per round where every box is the same (each cluster's nearest is the lowest position in its window: only 0 and 1
# are mutual): n coincident boxes take n - 1 rounds, PLOC's longest path, and too many for the serial twin from here on.  Its tree is
# known in closed form (R.ploc_chain, held to the twin at the smaller sizes by test_ploc_chain_is_the_twin_of_coincident_boxes)
CHAIN_FROM = 1030
MAX_LEVELS = 96  # bvh_build_impl.h: kMaxLevels
_REF = {}


def reference(name, n):
    """boxes, pad and the twins of one box set: computed once, shared by the builders, never changed"""
    if (name, n) not in _REF:
        boxes = pile() if name == "pile" else SETS[name](n)
        _REF[name, n] = dict(boxes=boxes, pad=R.build_pad(boxes))
    return _REF[name, n]


def twin(name, n, which):
    ref = reference(name, n)
    if which not in ref:
        chain = which == "ploc" and name == "coincident" and n > CHAIN_FROM
        ref[which] = (R.ploc_chain if chain else R.ploc_twin if which == "ploc" else R.lbvh_twin)(ref["boxes"], ref["pad"])
    return ref[which]


# ---- without a GPU: the constants ----------------------------------------------------------------------------------------------------------------
def test_constants_mirror_the_source():
    sah = open(os.path.join(CSRC, "bvh_sah.hip")).read()
    ploc = open(os.path.join(CSRC, "bvh_ploc.hip")).read()
    build = open(os.path.join(CSRC, "bvh_build.hip")).read()
    found = {
        "kSahQuant": int(re.search(r"constexpr int kSahQuant = (\d+);", sah).group(1)),
        "kSweepRounds": int(re.search(r"constexpr uint32_t kSweepRounds = (\d+);", sah).group(1)),
        "kPlocRadius": int(re.search(r"constexpr int kPlocRadius = (\d+);", ploc).group(1)),
        "kPlocTail": int(re.search(r"constexpr uint32_t kPlocTail = (\d+);", ploc).group(1)),
    }
    assert found == {"kSahQuant": R.SAH_QUANT, "kSweepRounds": R.SWEEP_ROUNDS, "kPlocRadius": R.PLOC_RADIUS, "kPlocTail": R.PLOC_TAIL}
    assert int(re.search(r"constexpr uint32_t kMaxLevels = (\d+);", open(os.path.join(CSRC, "bvh_build_impl.h")).read()).group(1)) == MAX_LEVELS
    m = re.search(r"cls = ratio2 > \(1\.0f / ([0-9.]+)f\) \? 0u : \(ratio2 > \(1\.0f / ([0-9.]+)f\) \? 1u : \(ratio2 > \(1\.0f / ([0-9.]+)f\) \? 2u : 3u\)\)", build)
    assert m, "k_morton's size classes"
    assert [f32(1.0) / f32(x) for x in m.groups()] == list(R.CLASS_RATIO2), "k_morton's size class thresholds"
    assert re.search(r"t \* (\d+)\.0f\), (\d+)u\);  // 20 bits per axis", build).groups() == (str(1 << R.AXIS_BITS), str((1 << R.AXIS_BITS) - 1))
    assert "<< 60" in build and "-ffp-contract=off" in open(os.path.join(CSRC, "Makefile")).read()
    # the sizes the GPU cases run at stand around these constants
    assert {R.PLOC_RADIUS + 1, R.PLOC_RADIUS + 2, 2 * R.PLOC_RADIUS + 1, 2 * R.PLOC_RADIUS + 2, R.PLOC_TAIL, R.PLOC_TAIL + 1} <= set(SIZES)


# ---- without a GPU: the references against brute force -----------------------------------------------------------------------------------------------
def tiny_sets():
    rs = np.random.RandomState(31)
    out = {f"soup{n}": soup(n) for n in (2, 3, 7, 12)}
    out["coincident6"] = coincident(6)
    out["grid9"] = flat_grid(9)
    out["grid12"] = flat_grid(12)
    out["classes12"] = size_classes(12)
    out["pairs10"] = np.repeat(soup(5), 2, axis=0)  # every box twice: ties that only the id breaks
    out["shuffled12"] = soup(12)[rs.permutation(12)]
    return out


TINY = tiny_sets()


@pytest.mark.parametrize("name", list(TINY))
@pytest.mark.parametrize("quant", [1, 4])
def test_sah_optimum_against_every_split(name, quant):
    """the float32 minimum of (cost, axis, i) against all splits listed one by one in float64: it costs what the cheapest costs, and
    where the cheapest is alone by more than the float32 roundings it is that very split"""
    boxes = TINY[name]
    ids = np.arange(len(boxes))
    axis, at, left, cost, low64 = R.sah_best(boxes, R.sah_orders(boxes), ids, quant)
    every = sorted(R.sah_enumerate64(boxes, ids, quant), key=lambda c: c[:3])
    assert len(every) == 3 * (len(boxes) - 1)
    cheapest = every[0]
    assert low64 == pytest.approx(cheapest[0], rel=1e-12, abs=0.0)
    took = [c for c in every if c[1] == axis and c[2] == at]
    assert len(took) == 1 and took[0][3] == [int(x) for x in left]
    assert took[0][0] <= cheapest[0] * R.GUARD
    assert float(cost) == pytest.approx(took[0][0], rel=2.0 ** -20, abs=0.0)
    rivals = [c for c in every if set(c[3]) != set(cheapest[3])]
    if all(c[0] > cheapest[0] * (1.0 + 2.0 ** -18) for c in rivals):
        assert set(int(x) for x in left) == set(cheapest[3])
    # equal costs: the lowest axis, then the lowest position.  Equal means the same float32 bits, listed split by split
    listed = [(int(cb), a, k + 1) for a, (_, L, Rt, nl, nr) in enumerate(R.sah_candidates(boxes, R.sah_orders(boxes), ids, quant))
              for k, cb in enumerate(R.bits(R.sah_cost32(L, Rt, nl, nr)))]
    low = min(c[0] for c in listed)
    ties = [c[1:] for c in listed if c[0] == low]
    assert (axis, at) == min(ties) and R.bits(cost) == low
    if name in ("coincident6", "grid9", "pairs10"):
        assert len(ties) > 1, "this set was chosen for its ties"


def test_sah_halving_and_orders():
    boxes = TINY["pairs10"]
    keys = R.sah_orders(boxes)
    ids = np.array([9, 3, 4, 8, 2, 0, 1])
    half = R.sah_halving(boxes, keys, ids)
    want = sorted(ids.tolist(), key=lambda t: (float(f32(boxes[t, 0] + boxes[t, 3])), t))[:3]
    assert half.tolist() == want
    x = np.array([-2.5, -0.0, 0.0, 1e-30, 3.0], dtype=f32)
    assert np.all(np.diff(R.f2ord(x).astype(np.int64)) >= 0) and R.f2ord(x)[0] < R.f2ord(x)[-1]


@pytest.mark.parametrize("name", list(TINY))
@pytest.mark.parametrize("radius", [1, 2, 3, R.PLOC_RADIUS])
def test_ploc_nearest_against_all_pairs(name, radius):
    boxes = TINY[name]
    assert R.ploc_nearest(boxes, radius).tolist() == R.ploc_nearest_brute(boxes, radius).tolist()


@pytest.mark.parametrize("name", list(TINY))
def test_twins_satisfy_the_contract(name):
    boxes = TINY[name]
    pad = R.build_pad(boxes)
    for t in (R.ploc_twin(boxes, pad), R.lbvh_twin(boxes, pad), R.ploc_twin(boxes, pad, radius=2)):
        R.check_contract(t, boxes, pad)
        R.same_nesting(t, t)
    # PLOC with a window that holds everything and two boxes far from the rest: the two are each other's nearest from the first round on
    if name == "soup7":
        far = boxes.copy()
        far[[2, 5]] += f32(100.0)
        t = R.ploc_twin(far, 0.0)
        together = [i for i in range(t.n - 1) if sorted(t.sorted_ids[int(t.first[i]):int(t.last[i]) + 1].tolist()) == [2, 5]]
        assert len(together) == 1


@pytest.mark.parametrize("n", [2, 3, 5, 17, 18, 33, 34, 65, 257])
def test_ploc_chain_is_the_twin_of_coincident_boxes(n):
    boxes = coincident(n)
    pad = R.build_pad(boxes)
    chain = R.ploc_chain(boxes, pad)
    R.check_contract(chain, boxes, pad)
    for radius in (R.PLOC_RADIUS, 2):
        t = R.ploc_twin(boxes, pad, radius=radius)
        R.same_nesting(chain, t)
        assert np.array_equal(chain.sorted_ids, t.sorted_ids) and chain.node_boxes.tobytes() == t.node_boxes.tobytes()
    assert int(chain.depths().max()) == n - 2
    with pytest.raises(AssertionError, match="differ"):
        R.ploc_chain(soup(5))


L_ = R.LEAF


def test_lbvh_twin_on_hand_written_keys():
    # the eight keys of Karras 2012, figure 3
    got = R.lbvh_from_keys([0b00001, 0b00010, 0b00100, 0b00101, 0b10011, 0b11000, 0b11001, 0b11110])
    assert got == ([3, L_ | 0, L_ | 2, 1, L_ | 4, 6, L_ | 5], [4, L_ | 1, L_ | 3, 2, 5, L_ | 7, L_ | 6], [0, 0, 2, 0, 4, 5, 5], [7, 1, 3, 3, 7, 7, 6])
    # equal keys split by their positions
    got = R.lbvh_from_keys([5, 5, 5, 5, 5])
    assert got == ([3, L_ | 0, L_ | 2, 1], [L_ | 4, L_ | 1, L_ | 3, 2], [0, 0, 2, 0], [4, 1, 3, 3])
    # a run of equal keys (positions 1 .. 6) between two others
    got = R.lbvh_from_keys([1, 3, 3, 3, 3, 3, 3, 8])
    assert got == ([6, 3, L_ | 2, L_ | 1, 5, L_ | 4, L_ | 0], [L_ | 7, 4, L_ | 3, 2, L_ | 6, L_ | 5, 1], [0, 1, 2, 1, 4, 4, 0], [7, 6, 3, 3, 6, 5, 6])
    assert R.lbvh_from_keys([7, 7]) == ([L_ | 0], [L_ | 1], [0], [1])


def test_lbvh_twin_against_the_definition():
    """every range splits where the highest differing bit of (key, position) of its two ends changes, found by looking at every entry"""
    rs = np.random.RandomState(5)
    for n in (2, 3, 9, 12, 40):
        keys = np.sort(rs.randint(0, 6 if n < 40 else 1 << 62, n).astype(np.uint64))
        left, right, first, last = R.lbvh_from_keys(keys)
        aug = [(int(k) << 32) | p for p, k in enumerate(keys)]
        for i in range(n - 1):
            f, l = first[i], last[i]
            bit = (aug[f] ^ aug[l]).bit_length() - 1
            clear = [p for p in range(f, l + 1) if not (aug[p] >> bit) & 1]
            assert clear == list(range(f, clear[-1] + 1)) and clear[-1] < l
            s = clear[-1]
            assert left[i] == (L_ | s if s == f else s) and right[i] == (L_ | (s + 1) if s + 1 == l else s + 1), i
            assert i == 0 or i in (f, l)  # Karras: a node stands at one end of its range


def test_morton_keys_by_hand():
    boxes = np.array([[0, 0, 0, 0, 0, 0], [1, 1, 0, 1, 1, 0], [0.5, 0, 0, 0.5, 0, 0], [0, 0, 0, 1, 1, 0]], dtype=f32)
    keys, cls = R.morton_keys(boxes)
    assert cls.tolist() == [3, 3, 3, 0]
    top = (1 << 20) - 1
    x, y = int(R.spread(np.array([top]))[0]) << 2, int(R.spread(np.array([top]))[0]) << 1
    half = int(R.spread(np.array([1 << 19]))[0])
    assert [int(k) & ((1 << 60) - 1) for k in keys] == [0, x | y, half << 2, (half << 2) | (half << 1)]  # z has no extent: 0
    assert int(R.spread(np.array([0b101]))[0]) == 0b1000001
    order, sorted_keys = R.morton_order(np.concatenate([boxes, boxes]))
    assert order.tolist() == [3, 7, 0, 4, 2, 6, 1, 5]  # classes first, equal keys in id order


# ---- without a GPU: the contract checker against mutants ------------------------------------------------------------------------------------------------
def mutants(t):
    """name -> a copy of the valid tree with one thing wrong"""
    inner = [i for i in range(1, t.n - 1) if not (int(t.left[i]) | int(t.right[i])) & R.LEAF]
    assert inner
    i = inner[0]

    def swapped(a):
        a["left"][i], a["right"][i] = a["right"][i], a["left"][i]

    def range_off(a):
        a["last"][i] -= 1

    def first_off(a):
        a["first"][i] += 1

    def parent_elsewhere(a):
        a["node_parent"][i] = (int(a["node_parent"][i]) + 1) % (t.n - 1)

    def leaf_parent_elsewhere(a):
        a["leaf_parent"][3] = (int(a["leaf_parent"][3]) + 1) % (t.n - 1)

    def box_ulp(a):
        a["node_boxes"].view(np.uint32)[i, 4] += 1

    def box_ulp_root(a):
        a["node_boxes"].view(np.uint32)[0, 0] -= 1

    def repeated_id(a):
        a["sorted_ids"][2] = a["sorted_ids"][6]

    def child_twice(a):
        a["right"][i] = a["left"][i]

    def root_has_parent(a):
        a["node_parent"][0] = 1

    out = {}
    for f in (swapped, range_off, first_off, parent_elsewhere, leaf_parent_elsewhere, box_ulp, box_ulp_root, repeated_id, child_twice, root_has_parent):
        a = t.arrays()
        f(a)
        out[f.__name__] = R.Tree(a)
    return out


@pytest.mark.parametrize("which", ["ploc", "lbvh"])
def test_contract_checker_rejects_mutants(which):
    boxes = soup(12)
    pad = R.build_pad(boxes)
    t = (R.ploc_twin if which == "ploc" else R.lbvh_twin)(boxes, pad)
    R.check_contract(t, boxes, pad)
    with pytest.raises(AssertionError):
        R.check_contract(t, boxes, f32(0.0))  # the widening is part of the contract
    ms = mutants(t)
    assert {"swapped", "range_off", "parent_elsewhere", "box_ulp", "repeated_id"} <= set(ms)
    for name, m in ms.items():
        try:
            R.check_contract(m, boxes, pad)
        except AssertionError:
            continue
        raise AssertionError(f"the mutant '{name}' was accepted")
    # what the exact comparisons say of a tree that is valid but another: swapping two boxes' ids changes the nesting
    other = t.arrays()
    other["sorted_ids"][[0, 11]] = other["sorted_ids"][[11, 0]]
    with pytest.raises(AssertionError, match="position"):
        R.same_nesting(R.Tree(other), t)


def test_sah_check_rejects_a_worse_split():
    """a valid tree that is not the sweep's: check_sah names the first node that is not at its optimum"""
    boxes = soup(12)
    pad = R.build_pad(boxes)
    t = R.lbvh_twin(boxes, pad)
    R.check_contract(t, boxes, pad)
    with pytest.raises(AssertionError, match=r"node \d+ \(depth"):
        R.check_sah(t, boxes)


# ---- without a GPU: the entry point -------------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared():
    header = open(os.path.join(ROOT, "include", "halart.h")).read()
    assert re.search(r"\*/\s*int hala_rt_selftest_hierarchy\(uint32_t count, const float\* boxes, float pad, uint32_t builder,", header)
    import hala_renderer_amd as H
    assert "hala_rt_selftest_hierarchy" in H._abi.EXPORTS and "hala_rt_selftest_hierarchy" in H._abi.PROTOTYPES
    assert len(H._abi.PROTOTYPES["hala_rt_selftest_hierarchy"][0]) == 14
    rust = open(os.path.join(ROOT, "rust", "hala-renderer-halart", "src", "lib.rs")).read()
    assert "pub fn hala_rt_selftest_hierarchy(count: u32, boxes: *const f32, pad: f32, builder: u32," in rust
    assert "hala_rt_selftest_hierarchy" in open(os.path.join(CSRC, "rt_selftest.hip")).read()


def test_entry_point_refuses(halart):
    """every refusal comes before the first device call (this test runs without a GPU) and names the function"""
    good = soup(8)
    Err = halart.HalaRendererError
    for boxes, pad, builder, drive, what in [
        (good[:1], 0.0, SAH, {}, "2 .. 2\\^20"),
        (np.zeros((0, 6), f32), 0.0, PLOC, {}, "2 .. 2\\^20"),
        (np.zeros(((1 << 20) + 1, 6), f32), 0.0, LBVH, {}, "2 .. 2\\^20"),
        (good, -1e-6, SAH, {}, "pad"),
        (good, float("inf"), SAH, {}, "pad"),
        (good, float("nan"), SAH, {}, "pad"),
        (good, 0.0, 0, {}, "builder"),
        (good, 0.0, 4, {}, "builder"),
        (good, 0.0, PLOC, dict(ploc_tail=3), "ploc_tail"),
        (good, 0.0, PLOC, dict(ploc_look_every=65), "ploc_look_every"),
    ]:
        with pytest.raises(Err, match="hala_rt_selftest_hierarchy.*" + what):
            halart.selftest_hierarchy(boxes, pad, builder, **drive)
    for at, value, what in [((3, 1), np.nan, "not finite"), ((0, 5), np.inf, "not finite"), ((7, 0), -np.inf, "not finite"), ((4, 2), 5.0, "min > max")]:
        bad = good.copy()
        bad[at] = value
        with pytest.raises(Err, match="hala_rt_selftest_hierarchy.*" + what):
            halart.selftest_hierarchy(bad, 0.0, SAH)
    lib = halart.load_library()
    arrays = [good] + [np.zeros(8, np.uint32) for _ in range(7)] + [np.zeros((7, 6), f32)]  # boxes, then the eight outputs
    for missing in range(len(arrays)):
        args = [None if k == missing else C.c_void_p(x.ctypes.data) for k, x in enumerate(arrays)]
        assert lib.hala_rt_selftest_hierarchy(8, args[0], C.c_float(0.0), SAH, 0, 0, *args[1:]) != 0
        assert "hala_rt_selftest_hierarchy" in halart.last_error() and "null" in halart.last_error()


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------------------------------------
def build_twice(halart, boxes, pad, builder, **drive):
    """the tree of one builder: the same bytes from two calls, the contract, and hala_rt_selftest_collapse's own validation of it"""
    got = halart.selftest_hierarchy(boxes, pad, builder, **drive)
    again = halart.selftest_hierarchy(boxes, pad, builder, **drive)
    for k in R.Tree.FIELDS:
        assert got[k].tobytes() == again[k].tobytes(), f"{k} differs between two identical calls"
    t = R.Tree(got)
    R.check_contract(t, boxes, pad)
    n = len(boxes)
    leaf_boxes = R.widen(boxes[t.sorted_ids.astype(np.int64)], pad)
    # The collapse first follows every reference, parent and range itself, then runs.  Along one path a 4-node takes in at most three
    # binary nodes and at least one, and a leaf of leaf_max triangles swallows at most leaf_max - 1 more: a tree of D binary levels
    # has between (D - (leaf_max - 1)) / 3 and D 4-wide levels, of which the collapse allows MAX_LEVELS.  Up to MAX_LEVELS binary
    # levels it must accept the tree, with a level count inside those bounds; where the lower bound exceeds MAX_LEVELS it cannot;
    # and wherever it refuses the reason must be the depth, never the tree's form
    levels, leaf_max = int(t.depths().max()) + 1, min(4, n - 1)
    fewest = max(1, -(-(levels - (leaf_max - 1)) // 3))
    try:
        packed = halart.selftest_collapse(t.left, t.right, t.node_parent, t.leaf_parent, t.first, t.last, t.node_boxes, leaf_boxes, leaf_max)
    except halart.HalaRendererError as e:
        assert levels > MAX_LEVELS and "4-wide levels" in str(e), f"a tree of {levels} binary levels was refused: {e}"
    else:
        assert 1 <= len(packed["refs4"]) <= n - 1
        assert fewest <= packed["levels"] <= min(levels, MAX_LEVELS), f"{levels} binary levels became {packed['levels']} 4-wide levels"
    return t


def check_builder(t, name, n, builder):
    """the builder's reference; the message of a failure names the node"""
    ref = reference(name, n)
    if builder == SAH:
        return R.check_sah(t, ref["boxes"])
    if builder == PLOC:
        want = twin(name, n, "ploc")
        R.same_nesting(t, want)
        assert np.array_equal(t.sorted_ids, want.sorted_ids)
        return None
    want = twin(name, n, "lbvh")
    for k in ("sorted_ids", "left", "right", "first", "last", "node_parent", "leaf_parent"):
        bad = np.nonzero(getattr(t, k) != getattr(want, k))[0]
        what = "sorted position" if k in ("sorted_ids", "leaf_parent") else "node"
        assert len(bad) == 0, f"{what} {bad[0]}: {k} is {getattr(t, k)[bad[0]]:#x}, Karras' hierarchy has {getattr(want, k)[bad[0]]:#x} ({len(bad)} differ)"
    assert t.node_boxes.tobytes() == want.node_boxes.tobytes()
    return None


@gpu
@pytest.mark.parametrize("name,n,builder", CASES, ids=[f"{s}-{n}-{NAMES[b]}" for s, n, b in CASES])
def test_builder_equals_its_reference(halart, name, n, builder):
    ref = reference(name, n)
    if name == "size_classes" and n >= 5:
        assert set(R.morton_keys(ref["boxes"])[1].tolist()) == {0, 1, 2, 3}
    t = build_twice(halart, ref["boxes"], ref["pad"], builder)
    check_builder(t, name, n, builder)


@gpu
@pytest.mark.parametrize("builder", [SAH, PLOC, LBVH], ids=lambda b: NAMES[b])
def test_pile_deeper_than_the_sweep(halart, builder):
    ref = reference("pile", 600)
    t = build_twice(halart, ref["boxes"], ref["pad"], builder)
    if builder == SAH:
        deepest = int(t.depths().max())
        assert deepest > R.SWEEP_ROUNDS, f"the deepest node is at depth {deepest}: the halving rule did not run"
        # ... and the sweep rule was not given up early: some node just above the limit took an uneven split
        assert R.check_sah(t, ref["boxes"]) == deepest
        d = t.depths()
        swept = [i for i in np.nonzero(d == R.SWEEP_ROUNDS - 1)[0] if t.span(t.left[i])[1] + 1 != int(t.first[i]) + (int(t.last[i]) + 1 - int(t.first[i])) // 2]
        assert swept, "no node at the last sweep depth was split unevenly"
    else:
        check_builder(t, "pile", 600, builder)


@gpu
@pytest.mark.parametrize("n", [513, 4100])
@pytest.mark.parametrize("drive", [dict(ploc_look_every=1), dict(ploc_tail=2), dict(ploc_look_every=7)], ids=lambda d: "-".join(f"{k}{v}" for k, v in d.items()))
def test_ploc_drivers_return_the_default_bytes(halart, n, drive):
    ref = reference("soup", n)
    want = halart.selftest_hierarchy(ref["boxes"], ref["pad"], PLOC)
    got = build_twice(halart, ref["boxes"], ref["pad"], PLOC, **drive).arrays()
    for k in R.Tree.FIELDS:
        assert got[k].tobytes() == want[k].tobytes(), k


def soup_scene(halart, n):
    """soup_triangles(n) as one primitive under an identity transform: commit() flattens it to exactly the boxes of soup(n)"""
    from hala_renderer_amd import scenes
    pos = soup_triangles(n)
    nrm = np.cross(pos[:, 1] - pos[:, 0], pos[:, 2] - pos[:, 0]).astype(np.float64)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    s = halart.HalaScene()
    s.materials = [halart.HalaMaterial(type=0, base_color=(0.7, 0.7, 0.7))]
    prim = halart.HalaPrimitive(indices=np.arange(3 * n, dtype=np.uint32), vertices=scenes._vertices(pos.reshape(-1, 3), np.repeat(nrm, 3, axis=0)))
    prim.material_index = 0
    s.meshes = [halart.HalaMesh([prim])]
    s.nodes = [halart.HalaNode(name="soup", mesh_index=0),
               halart.HalaNode(name="camera", camera_index=0, local_transform=scenes.look_at_node_transform((0.4, 0.6, 3.0), (0.5, 0.5, 0.5)))]
    s.cameras = [halart.HalaPerspectiveCamera(aspect=1.0, yfov=0.7, znear=0.1)]
    return s


@gpu
@pytest.mark.parametrize("n", [1030, 4100])
@pytest.mark.parametrize("builder", [SAH, PLOC, LBVH], ids=lambda b: NAMES[b])
def test_commit_runs_the_same_hierarchy(halart, n, builder):
    """the triangles commit() stores are in the order the self-test returns: it runs the hierarchy a build runs"""
    ref = reference("soup", n)
    r = halart.HalaRenderer("hierarchy", 16, 16, 5, 3, False, False, False, 0)
    try:
        r.set_build_options(builder=NAMES[builder], instancing=False)
        r.set_scene(soup_scene(halart, n))
        r.commit()
        _, tris = r.download_bvh()
    finally:
        r.close()
    stored = tris.reshape(-1, 12)[:, 3]
    assert len(stored) == n
    got = halart.selftest_hierarchy(ref["boxes"], ref["pad"], builder)
    bad = np.nonzero(stored != got["sorted_ids"])[0]
    assert len(bad) == 0, f"sorted position {bad[0]}: commit() stores triangle {stored[bad[0]]}, the self-test {got['sorted_ids'][bad[0]]}"
