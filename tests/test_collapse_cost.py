"""The collapse of the binary hierarchy into 4-wide nodes picks the cheapest cut (csrc/bvh_build.hip: k_collapse_cost, k_collapse_level).

Without a GPU: the reference programme of collapse_ref.py against the enumeration of every cut.  On the GPU: the library's kernels,
through hala_rt_selftest_collapse, against that reference bit for bit, and the properties any collapse must have on built trees."""
import os
import re

import numpy as np
import pytest

import collapse_ref as R
from hala_renderer_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
f32 = np.float32


def same_boxes(n):
    return np.tile(np.array([0, 0, 0, 1, 2, 3], dtype=f32), (n, 1))


def four_leaf_subtree(spread):
    """16 leaves, leaf_max = 4; node `sub` holds exactly the four leaves 4 .. 7.  spread: they are specks far apart (their leaf costs
    8 x the area of a box that is nearly empty: dearer than a 4-node over four specks); else four boxes that nearly coincide (a 4-node
    would pay the box once more and then every child)."""
    rng = np.random.RandomState(5)
    boxes = R.random_boxes(rng, 16)
    lo = boxes[4:8, :3].copy()
    if spread:
        boxes[4:8, 3:] = lo + f32(1e-3)
    else:
        boxes[4:8, :3] = lo[0] + (rng.rand(4, 3) * 1e-3).astype(f32)
        boxes[4:8, 3:] = boxes[4:8, :3] + f32(0.3)
    t = R.Tree(R.perfect(16), boxes)
    sub = [i for i in range(t.n - 1) if (t.first[i], t.last[i]) == (4, 7)][0]
    return t, sub


def cases():
    """name -> (tree, leaf_max): the shapes of the issue.  Small enough to enumerate: up to 9 leaves."""
    rng = np.random.RandomState(20261)
    out = {
        "two_leaves": (R.Tree((0, 0), R.random_boxes(rng, 2)), 1),
        "three_leaves": (R.Tree((0, (0, 0)), R.random_boxes(rng, 3)), 1),
        "three_leaves_leaf2": (R.Tree(((0, 0), 0), R.random_boxes(rng, 3)), 2),
        "chain9": (R.Tree(R.chain(9), R.random_boxes(rng, 9)), 4),
        "chain9_items": (R.Tree(R.chain(9), R.random_boxes(rng, 9)), 1),
        "perfect16": (R.Tree(R.perfect(16), R.random_boxes(rng, 16)), 4),
        "perfect16_leaf8": (R.Tree(R.perfect(16), R.random_boxes(rng, 16)), 8),
        "same_area9": (R.Tree(R.random_shape(rng, 9), same_boxes(9)), 4),
        "same_area16": (R.Tree(R.perfect(16), same_boxes(16)), 4),
        "same_area16_items": (R.Tree(R.perfect(16), same_boxes(16)), 1),
        "flat_boxes": (R.Tree(R.perfect(8), np.tile(np.array([0, 0, 0, 1, 0, 0], dtype=f32), (8, 1))), 2),  # every area is 0: all ties
        "leaf_dearer": (four_leaf_subtree(True)[0], 4),
        "leaf_cheaper": (four_leaf_subtree(False)[0], 4),
        "items17": (R.Tree(R.random_shape(rng, 17), R.random_boxes(rng, 17)), 1),
    }
    for n in (5, 6, 7, 9, 13, 31, 64):
        for leaf_max in (1, 4):
            out[f"random{n}_leaf{leaf_max}"] = (R.Tree(R.random_shape(rng, n), R.random_boxes(rng, n)), leaf_max)
    return out


CASES = cases()


# ---- without a GPU ----------------------------------------------------------------------------------------------------------------------
def test_constants_mirror_the_source():
    src = open(os.path.join(ROOT, "hala-renderer_amd", "csrc", "bvh_build.hip")).read()
    leaf = re.search(r"#define RT_COLLAPSE_LEAF_COST ([0-9.]+)f", src).group(1)
    node = re.search(r"kCollapseNodeCost = ([0-9.]+)f", src).group(1)
    assert f32(leaf) == R.C_LEAF and f32(node) == R.C_NODE
    assert "k_keep_flags" not in src  # one rule: the greedy opening is gone, not kept beside the new one
    rust = open(os.path.join(ROOT, "rust", "hala-renderer-halart", "src", "lib.rs")).read()
    assert "pub fn hala_rt_selftest_collapse(" in rust


@pytest.mark.parametrize("name", [k for k, (t, _) in CASES.items() if t.n <= 9])
def test_the_programme_finds_the_cheapest_of_all_cuts(name):
    t, leaf_max = CASES[name]
    cost, choice, keep = R.costs(t, leaf_max)
    best, looked_at = R.enumerate_cuts(t, leaf_max)
    assert looked_at >= 1
    assert f32(cost[0, 0]).tobytes() == f32(best).tobytes()
    refs4 = R.walk(t, choice, keep)
    R.check_tree(t, refs4, keep, leaf_max)
    # the tree that was walked costs what the programme said (binary32 sums against a float64 sum)
    assert R.tree_cost(t, refs4, keep) == pytest.approx(float(cost[0, 0]), rel=1e-5, abs=1e-30)


@pytest.mark.parametrize("name", list(CASES))
def test_reference_trees_are_valid(name):
    t, leaf_max = CASES[name]
    cost, choice, keep = R.costs(t, leaf_max)
    assert np.all(cost[:, 1] <= cost[:, 0]) and np.all(cost[:, 2] <= cost[:, 1])
    R.check_tree(t, R.walk(t, choice, keep), keep, leaf_max)


def test_leaf_or_split_follows_the_cost():
    for spread in (True, False):
        t, sub = four_leaf_subtree(spread)
        _, _, keep = R.costs(t, 4)
        assert keep[sub] == (1 if spread else 0)
        refs4 = R.walk(t, *R.costs(t, 4)[1:])
        assert (sub in refs4.reshape(-1).tolist()) or spread  # where the leaf is cheaper the subtree is a child as a whole


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_kernels_equal_the_reference(halart, name):
    t, leaf_max = CASES[name]
    got = halart.selftest_collapse(*t.arrays(), leaf_max)
    again = halart.selftest_collapse(*t.arrays(), leaf_max)
    cost, choice, keep = R.costs(t, leaf_max)
    print(name, "root cost", got["costs"][0, 0], "reference", cost[0, 0], "4-nodes", len(got["refs4"]))
    assert got["costs"][0, 0].tobytes() == cost[0, 0].tobytes()
    if t.n <= 9:
        assert got["costs"][0, 0].tobytes() == f32(R.enumerate_cuts(t, leaf_max)[0]).tobytes()
    assert got["costs"].tobytes() == cost.tobytes()
    assert np.array_equal(got["choices"], choice) and np.array_equal(got["keep"], keep)
    per_node = R.check_tree(t, got["refs4"], got["keep"], leaf_max)
    assert 2.0 <= per_node <= 4.0
    assert np.array_equal(got["refs4"], R.walk(t, choice, keep))
    for k in ("costs", "choices", "keep", "refs4"):
        assert got[k].tobytes() == again[k].tobytes(), k
    assert got["levels"] == again["levels"] >= 1


@gpu
def test_kernels_leaf_or_split_follows_the_cost(halart):
    for spread in (True, False):
        t, sub = four_leaf_subtree(spread)
        got = halart.selftest_collapse(*t.arrays(), 4)
        assert got["keep"][sub] == (1 if spread else 0)
        as_child = sub in got["refs4"].reshape(-1).tolist()
        roots = R.check_tree(t, got["refs4"], got["keep"], 4)
        assert roots > 0 and (as_child or spread)


@gpu
def test_hook_refuses_what_is_no_tree(halart):
    t, _ = CASES["perfect16"]
    a = [np.array(x) for x in t.arrays()]
    with pytest.raises(halart.HalaRendererError, match="leaf_max"):
        halart.selftest_collapse(*a, 16)
    bad = [x.copy() for x in a]
    bad[0][3] = 5000  # left child out of range
    with pytest.raises(halart.HalaRendererError, match="node reference"):
        halart.selftest_collapse(*bad, 4)
    bad = [x.copy() for x in a]
    bad[1][2] = bad[0][2]  # a child referenced twice
    with pytest.raises(halart.HalaRendererError):
        halart.selftest_collapse(*bad, 4)
    bad = [x.copy() for x in a]
    bad[5][0] = 3  # the root's range
    with pytest.raises(halart.HalaRendererError, match="sorted positions"):
        halart.selftest_collapse(*bad, 4)


# ---- built trees -----------------------------------------------------------------------------------------------------------------------------
SCENES = {  # test_gpu_parity.py::test_bvh_structure_and_flattening: the smallest trees that go through every level kernel
    "cornell": lambda: scenes.cornell_box(),
    "blob_5k": lambda: scenes.bunny_class(subdivisions=4),
    "sponza_60k": lambda: scenes.sponza_class(target_triangles=60000, disney=False),
}
ABSENT = 0xFFFFFFFF


def committed(halart, scene, two_level):
    r = halart.HalaRenderer("collapse", 16, 16, 5, 3, False, False, False, 0)
    if two_level:
        r.set_build_options(instancing=True)
    r.set_scene(scene)
    r.commit()
    return r


@gpu
@pytest.mark.parametrize("name", list(SCENES) + ["sponza_60k:two_level"])
def test_built_trees(halart, oracle, name):
    two_level = name.endswith(":two_level")
    s = SCENES[name.split(":")[0]]()
    if two_level:
        oracle.set_instancing(True)
    try:
        osc = oracle.OracleScene(s)
    finally:
        oracle.set_instancing(False)
    r = committed(halart, s, two_level)
    try:
        nodes, tris = r.download_bvh()
        refs = r.download_instance_refs()
        assert (len(refs) > 0) == two_level
        rc = (oracle.validate_bvh_two_level(osc, nodes, tris, refs) if two_level else oracle.validate_bvh(nodes, tris, osc.triangles()))[0]
        assert rc == 0
        r.refit()  # nothing moved: the frozen topology packs to the same bytes
        refit_nodes, refit_tris = r.download_bvh()
        assert refit_nodes.tobytes() == nodes.tobytes() and refit_tris.tobytes() == tris.tobytes()
    finally:
        r.close()
    r = committed(halart, s, two_level)
    try:
        again, _ = r.download_bvh()
    finally:
        r.close()
    assert again.tobytes() == nodes.tobytes()
    present = (nodes.reshape(-1, 16)[:, 12:16] != ABSENT).sum(axis=1)
    inner = present[present > 0]  # a two-level node array keeps reserved, empty ranges
    per_node = inner.sum() / len(inner)
    print(f"{name}: {len(inner)} nodes, {per_node:.4f} children per node")
    assert per_node >= 3.0
