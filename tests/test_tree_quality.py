"""Tree cost and the refit policy (docs/RENDER_SPEC.md 4.6; include/halart.h "Tree quality and the refit policy"; csrc/bvh_quality.hip).

CPU tier: the numpy twin (tests/tree_quality_ref.py) on a hand-written tree and on the oracle's tree in the product format, before and
after the scramble; the layouts of the two structs.  GPU tier, every comparison exact: k_tree_cost equals the twin on the downloaded
nodes as integers; a refit that degrades the tree shows in `now` and not in `built`; modes 2 and 1 rebuild to the bytes of a fresh
commit, on both sides of the threshold; images and step counts after the rebuild are the oracle's; two-level scenes; deformers survive
the rebuild; hala_rt_refit_nodes leaves the ordinary sequence's state; a step of the shutter measures nothing.

The scramble: the positions of the blob's vertices permuted among themselves (fixed seed), the topology kept — every triangle then spans
the whole blob, and a refitted tree's boxes with it."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

import deform_ref as D
import hala_renderer_amd as H
import tree_quality_ref as Q
from conftest import ROOT
from hala_renderer_amd import _abi as A
from hala_renderer_amd import scenes
from hala_renderer_amd.scene import INVALID
from test_gpu_parity import make_renderer, validate_tree
from test_instance_levels import _moved, instance_scene, oracle_scene
from test_oracle_render import random_rays

gpu = pytest.mark.gpu
f32 = np.float32
W, HGT = 48, 36
ONE = 1 << 32


# ---- scenes and helpers -----------------------------------------------------------------------------------------------------------------
def blob_scene(subdivisions=3):
    return scenes.bunny_class(subdivisions=subdivisions, aspect=W / HGT)  # mesh 0 primitive 0: the blob (20 * 4^s triangles); a ground quad


def scramble(vertices, seed=4242):
    out = vertices.copy()
    out["position"] = vertices["position"][np.random.RandomState(seed).permutation(len(vertices))]
    return out


def scrambled_scene(s, mesh=0):
    s2 = copy.deepcopy(s)
    s2.meshes[mesh].primitives[0].vertices = scramble(s.meshes[mesh].primitives[0].vertices)
    return s2


def single_triangle_scene():
    s = scenes.cornell_box(aspect=W / HGT)
    s.meshes = [H.HalaMesh([H.HalaPrimitive(indices=np.array([0, 1, 2], np.uint32), vertices=s.meshes[0].primitives[0].vertices[:3], material_index=0)])]
    s.nodes = [H.HalaNode(name="t", mesh_index=0)] + [n for n in s.nodes if n.mesh_index == INVALID]
    return s


def two_level_blob_scene():
    """test_instance_levels.instance_scene(3, world): three instanced instances, a ground and a squashed (flattened) instance in the world
    tree — with the 320-triangle blob in place of the 12-triangle box, so that its object-space tree has something to lose"""
    s = copy.deepcopy(instance_scene(3, True))
    blob = scenes.blob_mesh(subdivisions=2)
    blob.material_index = 0
    s.meshes[0] = H.HalaMesh([blob])
    return s


def nodes_of(r):
    return r.download_bvh()[0].reshape(-1, 16)


def quality(r):
    trees, measured, rebuilt = r.tree_quality()
    return [tuple(getattr(t, n) for n, _ in A.TreeQuality._fields_) for t in trees], measured, rebuilt


def twin(r):
    """the twin's (valid, node_q, tri_q) of every tree the renderer reports, from the download alone"""
    nodes = nodes_of(r)
    return [Q.tree_cost(nodes, (t.first_node, t.node_count)) for t in r.tree_quality()[0]]


def now_of(t):
    return (t.valid, t.node_q_now, t.tri_q_now)


def built_of(t):
    return (t.valid, t.node_q_built, t.tri_q_built)


def images(r, frames=2):
    for _ in range(frames):
        r.update()
    r.render()
    return r.read_image(0).tobytes()


def tree_bytes(r):
    nodes, tris = r.download_bvh()
    return nodes.tobytes(), tris.tobytes()


_REF = {}


def blob_case(oracle):
    """the blob scene, its scramble, the twin's inflation of the scramble on a refitted tree, the oracle's images of the scrambled scene:
    computed once (the GPU part by the first GPU test that asks)"""
    if "blob" not in _REF:
        s = blob_scene()
        s2 = scrambled_scene(s)
        want, _ = oracle.OracleScene(s2).render(W, HGT, frames=2)
        _REF["blob"] = dict(scene=s, scrambled=s2, verts=s2.meshes[0].primitives[0].vertices, image=want[0].tobytes())
    return _REF["blob"]


def refit_reference(halart, oracle):
    """a policy-free renderer's trees after commit and after the scrambling refit, and the fresh commit of the scrambled scene"""
    c = blob_case(oracle)
    if "refit" not in c:
        r = make_renderer(halart, c["scene"], W, HGT)
        try:
            built = Q.cost(nodes_of(r), (0, r.bvh_info().node_count))
            r.update_vertices(0, 0, c["verts"])
            r.refit()
            c["refit"] = tree_bytes(r)
            c["inflation"] = Q.cost(nodes_of(r), (0, r.bvh_info().node_count)) / built
        finally:
            r.close()
        r = make_renderer(halart, c["scrambled"], W, HGT)
        try:
            c["fresh"] = tree_bytes(r)
            c["fresh_cost"] = Q.tree_cost(nodes_of(r), (0, r.bvh_info().node_count))
        finally:
            r.close()
    return c


# ---- CPU tier ---------------------------------------------------------------------------------------------------------------------------
def _node(exps, children):
    """children: up to four (qlo xyz, qhi xyz, ref)"""
    nd = np.zeros(16, dtype=np.uint32)
    nd[3] = (exps[0] + 127) | ((exps[1] + 127) << 8) | ((exps[2] + 127) << 16)
    nd[12:16] = 0xFFFFFFFF
    for c, (lo, hi, ref) in enumerate(children):
        for a in range(3):
            nd[4 + a] |= lo[a] << (8 * c)
            nd[7 + a] |= hi[a] << (8 * c)
        nd[12 + c] = ref
    return nd


def test_twin_on_a_hand_written_tree():
    leaf = lambda first, count: 0x80000000 | ((count - 1) << 28) | first  # noqa: E731
    # root: quanta 2^-2 on every axis.  Child 0 (inner, node 1) spans 0..128 on every axis, child 1 (a leaf of 2) spans 128..255 in x and
    # 0..64 in y and z.  Root extent: 255 quanta in x, 128 in y and z -> D = (63.75, 32, 32), h_root = (63.75*32 + 32*32) + 32*63.75 = 5104.
    #   child 0: d = (32, 32, 32), h = 3072, rho = 3072 / 5104; child 1: d = (31.75, 16, 16), h = (508 + 256) + 508 = 1272, rho = 1272 / 5104
    # node 1: quanta 2^-3; child 0 (a leaf of 1) spans 0..255 in x, 0..0 in y, 0..8 in z: d = (31.875, 0, 1), h = 31.875;
    #   child 1 (a leaf of 3) spans 10..20 on every axis: d = 1.25 each, h = 3 * 1.5625 = 4.6875
    nodes = np.stack([_node((-2, -2, -2), [((0, 0, 0), (128, 128, 128), 1), ((128, 0, 0), (255, 64, 64), leaf(0, 2))]),
                      _node((-3, -3, -3), [((0, 0, 0), (255, 0, 8), leaf(2, 1)), ((10, 10, 10), (20, 20, 20), leaf(3, 3))])])
    q = lambda h: int(f32(f32(h) / f32(5104.0)) * f32(4294967296.0))  # noqa: E731
    valid, node_q, tri_q = Q.tree_cost(nodes, (0, 2))
    assert valid == 1
    assert node_q == ONE + q(3072.0)
    assert tri_q == 2 * q(1272.0) + 1 * q(31.875) + 3 * q(4.6875)
    assert q(3072.0) == int(np.floor(float(f32(3072.0) / f32(5104.0)) * 2.0 ** 32))  # (the scaling by 2^32 is exact)
    # the sub-tree alone is a tree as well: its own root extent (255, 20, 20 quanta of 2^-3 -> 31.875, 2.5, 2.5)
    h1 = f32(f32(f32(31.875) * f32(2.5)) + f32(f32(2.5) * f32(2.5))) + f32(f32(2.5) * f32(31.875))
    q1 = lambda h: int(f32(f32(h) / h1) * f32(4294967296.0))  # noqa: E731
    assert Q.tree_cost(nodes, (1, 1)) == (1, ONE, q1(31.875) + 3 * q1(4.6875))
    # a share above 4 is clamped; a root without area is invalid; so is a node without children
    big = np.stack([_node((0, 0, 0), [((0, 0, 0), (1, 1, 1), 1)]), _node((4, 4, 4), [((0, 0, 0), (255, 255, 255), leaf(0, 1))])])
    assert Q.tree_cost(big, (0, 2)) == (1, ONE + ONE, 4 * ONE)
    flat = _node((0, 0, 0), [((0, 0, 0), (9, 0, 0), leaf(0, 1))])[None]
    assert Q.tree_cost(flat, (0, 1)) == (0, 0, 0)
    assert Q.tree_cost(_node((0, 0, 0), [])[None], (0, 1)) == (0, 0, 0)


def test_twin_on_the_oracles_tree_before_and_after_the_scramble(oracle):
    """the oracle's own builds are both good trees: what the scramble costs a FRESH tree — the geometry's share.  A refitted tree pays more
    (the GPU tier)"""
    c = blob_case(oracle)
    costs = []
    for s in (c["scene"], c["scrambled"]):
        nodes, tris = oracle.OracleScene(s).export_bvh4()
        nodes = nodes.reshape(-1, 16)
        valid, node_q, tri_q = Q.tree_cost(nodes, (0, len(nodes)))
        assert valid == 1 and node_q > ONE and tri_q > 0
        costs.append(node_q + tri_q)
    assert costs[1] > costs[0]


def test_struct_layouts_and_mirrors():
    assert C.sizeof(A.RefitPolicy) == 16
    assert [getattr(A.RefitPolicy, n).offset for n, _ in A.RefitPolicy._fields_] == [0, 4, 8]
    assert C.sizeof(A.TreeQuality) == 48
    assert [getattr(A.TreeQuality, n).offset for n, _ in A.TreeQuality._fields_] == [0, 4, 8, 12, 16, 24, 32, 40]
    for fn in ("hala_rt_set_refit_policy", "hala_rt_get_tree_quality"):
        assert fn in A.EXPORTS and fn in A.PROTOTYPES, fn
    header = open(os.path.join(ROOT, "include", "halart.h")).read()
    for name, value in (("OFF", 0), ("THRESHOLD", 1), ("ALWAYS", 2), ("MEASURE", 3)):
        assert f"#define HALA_REFIT_POLICY_{name} {value}u" in header and getattr(A, f"REFIT_POLICY_{name}") == value
    assert "#define HALA_NODE_REFIT_POLICY_REBUILD 6u" in header and A.NODE_REFIT_POLICY_REBUILD == 6
    body = header[header.index("typedef struct hala_tree_quality {"):header.index("} hala_tree_quality;")]
    assert [w.strip(" ,;") for ln in body.splitlines()[1:] for w in ln.split("/*")[0].replace("unsigned long long", "").replace("uint32_t", "").split(",") if w.strip(" ,;")] == \
        [n for n, _ in A.TreeQuality._fields_]
    rust = open(os.path.join(ROOT, "rust", "hala-renderer-halart", "src", "lib.rs")).read()
    assert "pub struct hala_refit_policy { pub mode: u32, pub max_inflation: f32, pub reserved: [u32; 2] }" in rust
    assert "pub fn hala_rt_get_tree_quality(" in rust and "pub fn hala_rt_set_refit_policy(" in rust


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------------------
@gpu
def test_refused_policies_change_nothing(halart):
    """(a renderer cannot be created without a device, so the refusals are checked here)"""
    r = make_renderer(halart, scenes.cornell_box(aspect=W / HGT), W, HGT)
    try:
        r.set_refit_policy(A.REFIT_POLICY_MEASURE)
        before = quality(r)
        assert len(before[0]) == 1

        def refused(mode, infl=0.0, reserved=0):
            p = A.RefitPolicy(mode=mode, max_inflation=infl)
            p.reserved[1] = reserved
            assert r._lib.hala_rt_set_refit_policy(r._h, C.byref(p)) != 0, (mode, infl, reserved)
            assert "Invalid refit policy" in halart.last_error()
            assert quality(r) == before

        refused(4)
        for bad in (0.5, float("nan"), float("inf"), -2.0):
            refused(1, bad)
        for mode in (0, 2, 3):
            refused(mode, 1.5)
        refused(3, 0.0, reserved=1)
        assert r._lib.hala_rt_set_refit_policy(r._h, None) != 0
        r.update_node_transform(0, _moved(np.eye(4, dtype=f32), 1))
        r.refit()
        assert quality(r)[1:] == (1, 0)  # still mode 3: measured, nothing rebuilt
        r.set_refit_policy(A.REFIT_POLICY_OFF)
        assert quality(r) == ([], 1, 0)
    finally:
        r.close()


def _check_two_level_ranges(r, trees):
    """every tree's range against the instance references' root fields and the instance levels, and its node count against its own links"""
    info = r.bvh_info()
    nodes = nodes_of(r)
    refs = r.download_instance_refs()
    roots = set(int(x) for x in refs[:, 12])
    top_children = nodes[:info.instance_node_count, 12:16].reshape(-1)
    top_inner = set(int(x) for x in top_children if x != 0xFFFFFFFF and not (x & 0x80000000))
    firsts = [t.first_node for t in trees]
    object_roots = set(f for f in firsts if f in roots)
    assert object_roots == roots
    for k, t in enumerate(trees):
        assert t.first_node >= info.instance_node_count and t.node_count >= 1
        assert t.first_node in roots or t.first_node in top_inner, k  # an instanced primitive's tree, or the world tree below the levels
        ch = nodes[t.first_node:t.first_node + t.node_count, 12:16].reshape(-1)
        inner = ch[(ch != 0xFFFFFFFF) & ((ch & 0x80000000) == 0)]
        # breadth-first numbering: the inner references of a tree are exactly the nodes behind its root
        assert sorted(int(x) for x in inner) == list(range(t.first_node + 1, t.first_node + t.node_count)), k
        if k + 1 < len(trees):
            assert t.first_node + t.node_count <= trees[k + 1].first_node


KERNEL_SCENES = {
    "cornell": (lambda: scenes.cornell_box(aspect=W / HGT), {}),
    "blob-sah": (lambda: blob_scene(3), dict(builder="sah")),
    "blob-ploc": (lambda: blob_scene(3), dict(builder="ploc")),
    "blob-lbvh": (lambda: blob_scene(3), dict(builder="lbvh")),
    "blob4-auto": (lambda: blob_scene(4), {}),
    "one-triangle": (single_triangle_scene, {}),
    "two-level": (lambda: instance_scene(5, True), dict(instancing=True, instance_levels="gpu")),
}


@gpu
@pytest.mark.parametrize("name", list(KERNEL_SCENES))
def test_kernel_equals_the_twin(halart, name):
    make, build = KERNEL_SCENES[name]
    r = halart.HalaRenderer("quality", W, HGT, 5, 3, False, False, False, 0)
    try:
        r.set_refit_policy(A.REFIT_POLICY_MEASURE)  # before the commit: the commit measures
        assert quality(r) == ([], 0, 0)
        if build:
            r.set_build_options(**build)
        r.set_scene(make())
        r.commit()
        trees, measured, rebuilt = r.tree_quality()
        want = twin(r)
        info = r.bvh_info()
        print(name, "nodes", info.node_count, "trees", [(t.first_node, t.node_count) for t in trees], "twin", want)
        assert (measured, rebuilt) == (0, 0)
        if name == "two-level":
            assert len(trees) == 3  # the world tree, the box's, the tetrahedron's
            _check_two_level_ranges(r, trees)
        else:
            assert [(t.first_node, t.node_count) for t in trees] == [(0, info.node_count)]
        if name == "one-triangle":
            assert info.node_count == 1  # (1 mod 16, and far from a full wave)
        for t, w in zip(trees, want):
            assert w[0] == 1 and now_of(t) == w and built_of(t) == w and t.rebuilt_last_refit == 0
        # a policy set on a committed renderer measures at once, and gives the same numbers
        r.set_refit_policy(A.REFIT_POLICY_OFF)
        assert quality(r)[0] == []
        r.set_refit_policy(A.REFIT_POLICY_THRESHOLD, 8.0)
        assert [now_of(t) for t in r.tree_quality()[0]] == want
    finally:
        r.close()


@gpu
def test_kernel_equals_the_twin_past_one_pass_of_the_grid(halart):
    """k_tree_cost runs at most 1 024 workgroups of 64 nodes: a tree of more than 65 536 nodes sends them round the grid-stride loop, and
    a refit of it is measured as well"""
    s = scenes.sponza_class(target_triangles=600_000, aspect=W / HGT, disney=False)
    r = make_renderer(halart, s, W, HGT)
    try:
        r.set_refit_policy(A.REFIT_POLICY_MEASURE)
        (t,), _, _ = r.tree_quality()
        print("nodes", t.node_count)
        assert t.node_count > 65536 + 64 and t.node_count == r.bvh_info().node_count
        assert now_of(t) == twin(r)[0] and built_of(t) == now_of(t) and t.valid == 1
        k = [k for k, n in enumerate(s.nodes) if n.mesh_index != INVALID][0]
        r.update_node_transform(k, _moved(s.nodes[k].local_transform, 2))
        r.refit()
        (t2,), measured, _ = r.tree_quality()
        assert measured == 1 and now_of(t2) == twin(r)[0] and built_of(t2) == built_of(t) and now_of(t2) != now_of(t)
    finally:
        r.close()


@gpu
def test_a_degrading_refit_shows_in_now_and_not_in_built(halart, oracle):
    c = refit_reference(halart, oracle)
    print("twin's inflation of the scramble on the refitted tree:", c["inflation"])
    assert c["inflation"] >= 2.0  # the precondition of this and the following tests
    r = make_renderer(halart, c["scene"], W, HGT)
    try:
        r.set_refit_policy(A.REFIT_POLICY_MEASURE)
        built = twin(r)[0]
        r.update_vertices(0, 0, c["verts"])
        r.refit()
        (t,), measured, rebuilt = r.tree_quality()
        assert now_of(t) == twin(r)[0] and built_of(t) == built and t.rebuilt_last_refit == 0
        assert (measured, rebuilt) == (1, 0)
        assert (t.node_q_now + t.tri_q_now) / (t.node_q_built + t.tri_q_built) == c["inflation"]
        assert tree_bytes(r) == c["refit"]  # measuring changes nothing
        # a camera-only refit measures nothing
        cam = [k for k, n in enumerate(c["scene"].nodes) if n.camera_index != INVALID][0]
        r.update_node_transform(cam, scenes.look_at_node_transform((0.5, 0.8, 4.0), (0.0, 0.0, 0.0)))
        r.refit()
        assert quality(r) == ([tuple(getattr(t, n) for n, _ in A.TreeQuality._fields_)], 1, 0)
    finally:
        r.close()


@gpu
def test_mode_2_rebuilds_to_the_bytes_of_a_fresh_commit(halart, oracle):
    c = refit_reference(halart, oracle)
    r = make_renderer(halart, c["scene"], W, HGT)
    try:
        r.set_refit_policy(A.REFIT_POLICY_ALWAYS)
        r.update_vertices(0, 0, c["verts"])
        r.refit()
        got = tree_bytes(r)
        assert got[0] == c["fresh"][0] and got[1] == c["fresh"][1]
        (t,), measured, rebuilt = r.tree_quality()
        assert now_of(t) == c["fresh_cost"] and built_of(t) == c["fresh_cost"] and t.rebuilt_last_refit == 1
        assert (measured, rebuilt) == (1, 1)
    finally:
        r.close()


@gpu
def test_mode_1_on_both_sides_of_the_threshold(halart, oracle):
    c = refit_reference(halart, oracle)
    r = make_renderer(halart, c["scene"], W, HGT)
    try:
        r.set_refit_policy(A.REFIT_POLICY_THRESHOLD, 2.0 * c["inflation"])
        r.update_vertices(0, 0, c["verts"])
        r.refit()
        assert tree_bytes(r) == c["refit"]
        (t,), measured, rebuilt = r.tree_quality()
        assert (measured, rebuilt, t.rebuilt_last_refit) == (1, 0, 0)
    finally:
        r.close()
    r = make_renderer(halart, c["scene"], W, HGT)
    try:
        r.set_refit_policy(A.REFIT_POLICY_THRESHOLD, 1.25)
        r.update_vertices(0, 0, c["verts"])
        r.refit()
        assert tree_bytes(r) == c["fresh"]
        (t,), measured, rebuilt = r.tree_quality()
        assert (measured, rebuilt, t.rebuilt_last_refit) == (1, 1, 1)
        assert now_of(t) == c["fresh_cost"] and built_of(t) == c["fresh_cost"]
        # a second refit with nothing moved rebuilds nothing (and measures nothing: no tree was refitted)
        r.refit()
        (t,), measured, rebuilt = r.tree_quality()
        assert (measured, rebuilt, t.rebuilt_last_refit) == (1, 1, 0)
        assert tree_bytes(r) == c["fresh"]
        # the same vertices again: the tree is refitted to what it was built for, measured, and stays
        r.update_vertices(0, 0, c["verts"])
        r.refit()
        (t,), measured, rebuilt = r.tree_quality()
        assert (measured, rebuilt, t.rebuilt_last_refit) == (2, 1, 0)
        assert now_of(t) == c["fresh_cost"] and tree_bytes(r) == c["fresh"]
    finally:
        r.close()


@gpu
def test_images_and_step_counts_after_the_rebuild(halart, oracle):
    c = refit_reference(halart, oracle)
    r = make_renderer(halart, c["scene"], W, HGT)
    try:
        r.set_refit_policy(A.REFIT_POLICY_THRESHOLD, 1.25)
        r.update_vertices(0, 0, c["verts"])
        r.refit()
        assert r.tree_quality()[2] == 1
        assert images(r) == c["image"]
        osc = oracle.OracleScene(c["scrambled"])
        assert validate_tree(oracle, osc, r)[0] == 0
        mn, mx = osc.bounds()
        pad = (mx - mn) * 0.2
        rays = np.concatenate([random_rays(4096 - W * HGT, mn - pad, mx + pad, 23), osc.camera_rays(W, HGT, 0)])
        assert len(rays) == 4096
        nodes, tris = r.download_bvh()
        for mode in (0, 1):
            hits, cnt = r.trace_rays_host(rays, mode, count_steps=True)
            ohits, ocnt = oracle.trace_on_bvh(nodes, tris, rays, mode)
            assert cnt == ocnt, mode
            assert hits.tobytes() == ohits.tobytes() and hits.tobytes() == osc.trace(rays, mode).tobytes()
    finally:
        r.close()


@gpu
def test_two_level_rebuild(halart, oracle):
    s = two_level_blob_scene()
    s2 = scrambled_scene(s, mesh=0)
    build = dict(instancing=True, instance_levels="gpu")
    fresh = make_renderer(halart, s2, W, HGT, build=build)
    try:
        fresh.set_refit_policy(A.REFIT_POLICY_MEASURE)
        fresh_trees = fresh.tree_quality()[0]
        fresh_nodes = nodes_of(fresh)
        fresh_tris = fresh.download_bvh()[1]
        fresh_cost = twin(fresh)
    finally:
        fresh.close()
    # which tree is the blob's, and what the scramble does to it when it is only refitted (mode 3)
    m = make_renderer(halart, s, W, HGT, build=build)
    try:
        m.set_refit_policy(A.REFIT_POLICY_MEASURE)
        roots = set(int(x) for x in m.download_instance_refs()[:, 12])
        before = m.tree_quality()[0]
        blob_tree = [k for k, t in enumerate(before) if t.first_node in roots and t.node_count > 16]
        assert len(before) == 2 and blob_tree == [1]  # the world tree, then the blob's
        m.update_vertices(0, 0, s2.meshes[0].primitives[0].vertices)
        m.refit()
        after, measured, rebuilt = m.tree_quality()
        assert [now_of(t) for t in after] == twin(m) and (measured, rebuilt) == (1, 0)
        t = after[1]
        inflation = (t.node_q_now + t.tri_q_now) / (t.node_q_built + t.tri_q_built)
        print("two-level: inflation of the blob's tree", inflation)
        assert inflation >= 2.0  # the precondition
    finally:
        m.close()
    r = make_renderer(halart, s, W, HGT, build=build)
    try:
        r.set_refit_policy(A.REFIT_POLICY_THRESHOLD, 1.25)
        r.update_vertices(0, 0, s2.meshes[0].primitives[0].vertices)
        r.refit()
        trees, measured, rebuilt = r.tree_quality()
        assert trees[1].rebuilt_last_refit == 1 and measured == 1 and rebuilt >= 1
        nodes = nodes_of(r)
        for k, t in enumerate(trees):
            if not t.rebuilt_last_refit:
                continue
            f = fresh_trees[k]
            assert (t.first_node, t.node_count) == (f.first_node, f.node_count), k
            assert nodes[t.first_node:t.first_node + t.node_count].tobytes() == fresh_nodes[f.first_node:f.first_node + f.node_count].tobytes(), k
            assert now_of(t) == fresh_cost[k] and built_of(t) == fresh_cost[k], k
        assert r.download_bvh()[1].tobytes() == fresh_tris.tobytes()
        assert [now_of(t) for t in trees] == twin(r)
        osc = oracle_scene(oracle, s2)
        assert validate_tree(oracle, osc, r)[0] == 0 and validate_tree(oracle, osc, r)[2]
        want, _ = osc.render(W, HGT, frames=2)
        assert images(r) == want[0].tobytes()
    finally:
        r.close()


@gpu
def test_a_rebuild_loses_no_deformer_state(halart):
    s = blob_scene()
    rest = s.meshes[0].primitives[0].vertices
    rig = D.random_rig(len(rest), targets=2, joint_count=3, seed=5, scale=6.0)  # morph deltas of about two blob radii
    far = D.random_pose(rig, seed=1, zero_some=False)
    near = D.random_pose(rig, seed=2, zero_some=False)
    near["morph_weights"] = (near["morph_weights"] * f32(0.03125)).astype(f32)
    r = make_renderer(halart, s, W, HGT)
    try:
        r.set_deformer(0, 0, **rig)
        r.set_refit_policy(A.REFIT_POLICY_THRESHOLD, 1.25)
        r.update_deformer(0, 0, **far)
        r.refit()
        (t,), measured, rebuilt = r.tree_quality()
        assert (measured, rebuilt, t.rebuilt_last_refit) == (1, 1, 1)
        assert r.read_vertices(0, 0).tobytes() == D.pose_vertices(rest, rig, far).tobytes()
        assert now_of(t) == twin(r)[0]
        # the next pose still starts from the rest pose
        r.update_deformer(0, 0, **near)
        r.refit()
        assert r.read_vertices(0, 0).tobytes() == D.pose_vertices(rest, rig, near).tobytes()
        (t,), measured, _ = r.tree_quality()
        assert measured == 2 and now_of(t) == twin(r)[0]
    finally:
        r.close()


@gpu
def test_refit_nodes_leaves_the_ordinary_sequences_state(halart, oracle):
    from test_node_batch import DEVICE, HOST, assert_path, assert_same_state, move
    s = copy.deepcopy(instance_scene(17, True))
    idx = list(range(17))
    mk = lambda: make_renderer(halart, s, W, HGT, build=dict(instancing=False))  # noqa: E731  (every instance flattened: one tree)
    a, b = mk(), mk()
    try:
        for r in (a, b):
            r.set_refit_policy(A.REFIT_POLICY_THRESHOLD, 1.0e6)
        a.bind_nodes(idx)
        # below the threshold: the device path, measured behind it
        move(a, b, s, [(k, _moved(s.nodes[k].local_transform, k)) for k in idx])
        assert_path(a, DEVICE)
        assert_same_state(a, b, "below the threshold")
        assert quality(a) == quality(b) and quality(a)[1:] == (1, 0)
        assert now_of(a.tree_quality()[0][0]) == twin(a)[0]
        # the same transforms again: nothing moved, nothing measured, on either side
        move(a, b, s, [(k, s.nodes[k].local_transform) for k in idx])
        assert_path(a, DEVICE)
        assert quality(a) == quality(b) and quality(a)[1:] == (1, 0)
        # any growth is too much now, and the instances trade places far apart
        for r in (a, b):
            r.set_refit_policy(A.REFIT_POLICY_THRESHOLD, 1.0)
        rs = np.random.RandomState(6)
        moves = []
        for k in idx:
            m = np.array(s.nodes[k].local_transform, dtype=f32)
            m[:3, 3] = rs.uniform(-40.0, 40.0, 3).astype(f32)
            moves.append((k, m))
        move(a, b, s, moves)
        assert quality(b)[2] == 1, "precondition: the ordinary sequence rebuilds"
        assert_path(a, HOST, A.NODE_REFIT_POLICY_REBUILD)
        assert_same_state(a, b, "above the threshold")
        assert quality(a) == quality(b) and quality(a)[1:] == (2, 1)
        # and on: the binding still works on the rebuilt tree
        move(a, b, s, [(k, _moved(s.nodes[k].local_transform, k)) for k in idx[:5]] + [(k, s.nodes[k].local_transform) for k in idx[5:]])
        assert_same_state(a, b, "after the rebuild")
        assert quality(a) == quality(b)
        want, _ = oracle.OracleScene(s).render(W, HGT, frames=2)
        assert images(a) == want[0].tobytes() and images(b) == want[0].tobytes()
    finally:
        a.close(); b.close()


@gpu
def test_a_shutter_step_measures_nothing(halart):
    s = copy.deepcopy(instance_scene(5, True))
    r = make_renderer(halart, s, W, HGT, build=dict(instancing=False))
    try:
        r.set_refit_policy(A.REFIT_POLICY_THRESHOLD, 1.0)
        opened = np.array(s.nodes[0].local_transform, dtype=f32)
        closed = opened.copy()
        closed[:3, 3] += f32(25.0)  # far enough that a measuring step would rebuild
        r.set_node_keys(0, opened, closed)
        r.set_shutter(0.0, 1.0, 1)
        r.refit()
        left = quality(r)
        for _ in range(5):
            r.update()
        r.render()
        st = r.shutter_status()
        assert st.enabled and st.steps >= 4
        assert quality(r) == left
    finally:
        r.close()
