"""Node batches (docs/RENDER_SPEC.md 20; include/halart.h "Node batches"): hala_rt_bind_nodes + hala_rt_refit_nodes against the ordinary
sequence — hala_rt_update_node_transform per node, then hala_rt_refit — on a twin renderer, byte for byte: tree nodes and triangles,
InstRef records, scene bounds, packed primitives with their 3x4 copy and two frames of all four images; the images also against the
oracle on a scene built at the new transforms, and the tree through the oracle's structural check.  Every test asserts the path the
call took and its reason, so a silent fallback cannot pass as the device path.  Frames are 32 x 24."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

import hala_renderer_amd as H
import node_batch_ref as NB
from conftest import ROOT
from hala_renderer_amd import _abi as A
from hala_renderer_amd import scenes
from test_gpu_parity import make_renderer, validate_tree
from test_instance_levels import HGT, W, _box, _moved, images, instance_scene, levels_state, oracle_scene, renderer

gpu = pytest.mark.gpu
f32 = np.float32
DEVICE, HOST = A.NODE_REFIT_PATH_DEVICE, A.NODE_REFIT_PATH_HOST


# ---- CPU tier ---------------------------------------------------------------------------------------------------------------------------
def _forest(n=300, seed=5):
    """n nodes, parents before children, chains at least five deep; rotated, scaled and sheared locals"""
    rs = np.random.RandomState(seed)
    parents, depth = [], []
    for k in range(n):
        if k < 5:
            p = k - 1  # one chain five deep for certain
        else:
            p = int(rs.randint(0, k)) if rs.rand() < 0.7 else -1
            if p >= 0 and depth[p] >= 7:
                p = -1
        parents.append(p)
        depth.append(0 if p < 0 else depth[p] + 1)
    locals_ = np.zeros((n, 4, 4), dtype=f32)
    for k in range(n):
        a, b = rs.uniform(-np.pi, np.pi, 2)
        ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        m = np.eye(4)
        m[:3, :3] = ry @ rx @ np.diag(rs.uniform(0.3, 1.7, 3))
        m[0, 1] += rs.uniform(-0.3, 0.3)
        m[:3, 3] = rs.uniform(-4.0, 4.0, 3)
        locals_[k] = m.astype(f32)
    return parents, locals_, max(depth)


def test_reference_worlds_equal_the_oracle(oracle):
    parents, locals_, deepest = _forest()
    assert deepest >= 4
    s = H.HalaScene()
    for p, m in zip(parents, locals_):
        s.nodes.append(H.HalaNode(parent=None if p < 0 else p, local_transform=m))
    want = oracle.world_transforms(s)  # [n, 16] column-major
    got = NB.column_major(NB.worlds(parents, locals_))
    assert got.tobytes() == want.tobytes()


def test_status_layout_exports_and_mirrors():
    S = A.NodeRefitStatus
    assert C.sizeof(S) == 40
    assert [(f, getattr(S, f).offset) for f, _ in S._fields_] == [("bound_nodes", 0), ("affected_nodes", 4), ("affected_instances", 8), ("levels", 12),
                                                                  ("last_path", 16), ("last_reason", 20), ("device_refits", 24), ("host_refits", 32)]
    header = open(os.path.join(ROOT, "include", "halart.h")).read()
    for fn in ("hala_rt_bind_nodes", "hala_rt_refit_nodes", "hala_rt_get_node_refit_status"):
        assert fn in A.EXPORTS and fn in A.PROTOTYPES and f"int {fn}(hala_rt_renderer* r" in header
    body = header[header.index("typedef struct hala_node_refit_status {"):header.index("} hala_node_refit_status;")]
    for word in ("bound_nodes, affected_nodes, affected_instances, levels;", "uint32_t last_path;", "uint32_t last_reason;",
                 "unsigned long long device_refits, host_refits;"):
        assert word in body
    rust = open(os.path.join(ROOT, "rust", "hala-renderer-halart", "src", "lib.rs")).read()
    assert ("pub struct hala_node_refit_status { pub bound_nodes: u32, pub affected_nodes: u32, pub affected_instances: u32, pub levels: u32, "
            "pub last_path: u32, pub last_reason: u32, pub device_refits: u64, pub host_refits: u64 }") in rust
    assert "pub fn hala_rt_refit_nodes(r: *mut hala_rt_renderer, locals: *const f32, where_: c_int) -> c_int;" in rust


def test_wrapper_refuses_bad_arrays_before_the_call():
    torch = pytest.importorskip("torch")

    class Lib:
        calls = 0

        def hala_rt_refit_nodes(self, *a):
            Lib.calls += 1
            return 0

    r = object.__new__(H.HalaRenderer)
    r._lib, r._h, r._check = Lib(), None, lambda rc: None
    r.node_refit_status = lambda: A.NodeRefitStatus(bound_nodes=3)
    with pytest.raises(ValueError):
        r.refit_nodes(np.zeros((2, 4, 4), dtype=f32))
    with pytest.raises(ValueError):
        r.refit_nodes(np.zeros((3, 16), dtype=f32))
    with pytest.raises(TypeError):
        r.refit_nodes(np.zeros((3, 4, 4), dtype=np.float64))
    with pytest.raises(ValueError):
        r.refit_nodes(torch.zeros(3, 16, dtype=torch.float32))  # on the CPU: not device input
    with pytest.raises(TypeError):
        r.refit_nodes(torch.zeros(3, 16, dtype=torch.float64))

    class Elsewhere:  # what the wrapper looks at of a tensor, on another GPU than the renderer's (device 0)
        dtype, device = torch.float32, torch.device("cuda", 1)
        shape = (3, 16)
        numel = lambda self: 48  # noqa: E731
        is_contiguous = lambda self: True  # noqa: E731
        data_ptr = lambda self: 4096  # noqa: E731

    with pytest.raises(ValueError, match="device 1"):
        r.refit_nodes(Elsewhere())
    assert Lib.calls == 0
    r.refit_nodes(np.zeros((3, 4, 4), dtype=f32))
    assert Lib.calls == 1
    r._h = None


# ---- GPU tier: helpers ------------------------------------------------------------------------------------------------------------------
def state(r):
    st = levels_state(r)
    md, t = r.packed_primitives()
    return dict(refs=st["refs"], bounds=st["bounds"], nodes=st["nodes"].tobytes(), tris=st["tris"].tobytes(), ref_count=st["ref_count"],
                prims=b"".join(bytes(m)[:72] for m in md), t3x4=t.tobytes())  # (the two addresses behind byte 72 are each renderer's own)


def assert_same_state(a, b, what):
    sa, sb = state(a), state(b)
    for k in sa:
        assert sa[k] == sb[k], f"{what}: {k}"
    return sa


def move(a, b, s, moves):
    """a: refit_nodes for its bound set (moves in the bound order); b: the ordinary sequence; s follows"""
    a.refit_nodes(np.stack([np.asarray(m, dtype=f32) for _, m in moves]))
    for k, m in moves:
        b.update_node_transform(k, m)
        s.nodes[k].local_transform = np.asarray(m, dtype=f32)
    b.refit()


def assert_path(r, path, reason=0):
    st = r.node_refit_status()
    assert (st.last_path, st.last_reason) == (path, reason)
    return st


def check(a, b, oracle, s, what, two_level=True):
    sa = assert_same_state(a, b, what)
    ia, ib = images(a), images(b)
    assert ia == ib, what
    osc = oracle_scene(oracle, s) if two_level else oracle.OracleScene(s)
    assert validate_tree(oracle, osc, a)[0] == 0, what
    want, _ = osc.render(W, HGT, frames=2)
    assert ia == [w.tobytes() for w in want], what
    return sa


def twins(halart, s, levels="gpu", instancing=True):
    mk = lambda: make_renderer(halart, s, W, HGT, build=dict(instancing=instancing, instance_levels=levels))  # noqa: E731
    return mk(), mk()


def chain_scene():
    """five boxes, each below the one before it, and a sixth beside them"""
    s = H.HalaScene()
    s.materials = [H.HalaMaterial(type=0, base_color=(0.7, 0.6, 0.5))]
    s.meshes = [H.HalaMesh([_box()])]
    rs = np.random.RandomState(77)
    for k in range(5):
        m = np.eye(4)
        a = rs.uniform(-1.0, 1.0)
        m[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) @ np.diag(rs.uniform(0.7, 1.1, 3))
        m[:3, 3] = rs.uniform(-0.9, 0.9, 3)
        s.nodes.append(H.HalaNode(name=f"link_{k}", mesh_index=0, parent=k - 1 if k else None, local_transform=m.astype(f32)))
    m = np.eye(4, dtype=f32)
    m[:3, 3] = (2.0, 0.5, -1.0)
    s.nodes.append(H.HalaNode(name="beside", mesh_index=0, local_transform=m))
    s.nodes.append(H.HalaNode(name="camera", camera_index=0, local_transform=scenes.look_at_node_transform((3.0, 4.0, 10.0), (0.0, 0.0, 0.0))))
    s.cameras = [H.HalaPerspectiveCamera(aspect=W / HGT, yfov=0.7, znear=0.1)]
    return s


def run_sets(halart, oracle, s, sets, **kw):
    s = copy.deepcopy(s)
    a, b = twins(halart, s, **kw)
    try:
        for idx in sets:
            a.bind_nodes(idx)
            st = a.node_refit_status()
            assert st.bound_nodes == len(idx) and st.affected_nodes >= len(idx) and st.levels >= 1
            move(a, b, s, [(k, _moved(s.nodes[k].local_transform, k)) for k in idx])
            assert_path(a, DEVICE)
            check(a, b, oracle, s, f"bound {idx}", two_level=kw.get("instancing", True))
    finally:
        a.close(); b.close()


# ---- hierarchy --------------------------------------------------------------------------------------------------------------------------
@gpu
def test_hierarchy_nested_scene(halart, oracle):
    # instance_scene(17, True): nodes 3 and 10 hang below 2 and 9
    run_sets(halart, oracle, instance_scene(17, True), [[5], [2], [3, 2], list(range(17))])


@gpu
def test_hierarchy_chain_five_deep(halart, oracle):
    s = chain_scene()
    run_sets(halart, oracle, s, [[4], [1], [4, 3, 2, 1, 0], [0, 1, 2, 3, 4, 5]])
    r = make_renderer(halart, s, W, HGT, build=dict(instancing=True, instance_levels="gpu"))
    try:
        r.bind_nodes([1])
        st = r.node_refit_status()
        assert (st.bound_nodes, st.affected_nodes, st.affected_instances, st.levels) == (1, 4, 4, 4)
    finally:
        r.close()


@gpu
def test_hierarchy_past_one_block(halart, oracle):
    run_sets(halart, oracle, instance_scene(257, False), [list(range(257))])


# ---- tree forms -------------------------------------------------------------------------------------------------------------------------
@gpu
def test_host_built_levels_take_the_host_path(halart, oracle):
    s = copy.deepcopy(instance_scene(17, True))
    a, b = twins(halart, s, levels="host")
    try:
        a.bind_nodes([5, 2])
        move(a, b, s, [(k, _moved(s.nodes[k].local_transform, k)) for k in (5, 2)])
        assert_path(a, HOST, A.NODE_REFIT_HOST_LEVELS)
        check(a, b, oracle, s, "host levels")
    finally:
        a.close(); b.close()


@gpu
def test_one_level_tree_refits_on_the_device(halart, oracle):
    run_sets(halart, oracle, instance_scene(17, True), [[5], [3, 2], list(range(19))], instancing=False)


@gpu
def test_flattened_instance_moves_the_world_tree(halart, oracle):
    s = copy.deepcopy(instance_scene(17, True))
    ground = [k for k, n in enumerate(s.nodes) if n.name == "ground"][0]
    a, b = twins(halart, s)
    try:
        before = state(a)
        a.bind_nodes([ground, 4])
        m = np.eye(4, dtype=f32)
        m[:3, 3] = (0.25, -0.5, 0.125)
        move(a, b, s, [(ground, m), (4, _moved(s.nodes[4].local_transform, 4))])
        assert_path(a, DEVICE)
        after = check(a, b, oracle, s, "ground")
        assert after["nodes"][18 * 64:] != before["nodes"][18 * 64:] and after["tris"] != before["tris"]  # the world tree behind the 18 reserved level nodes
    finally:
        a.close(); b.close()


@gpu
def test_host_refit_that_changes_what_a_tree_is_published_with_then_the_device_path(halart, oracle):
    """The one material, which the flattened ground and box carry too, becomes invisible: the scene gains the any-hit copy of its
    triangles, which every tree learns of when the host path publishes it again (the pending edit).  The next call takes the device
    path, which publishes nothing, and moves the world tree; then the same with the material opaque again.  (The oracle's accumulated
    and final images of the invisible scene differ from the opaque one's in 199 of the 768 pixels: the images tell the two apart.)"""
    s = copy.deepcopy(instance_scene(17, True))
    ground = [k for k, n in enumerate(s.nodes) if n.name == "ground"][0]
    a, b = twins(halart, s)
    try:
        a.bind_nodes([ground, 4])
        step = 0
        for opacity in (0.0, 1.0):
            s.materials[0] = H.HalaMaterial(type=0, base_color=(0.7, 0.6, 0.5), opacity=opacity)
            for r in (a, b):
                r.update_material(0, s.materials[0])
            for path, reason in ((HOST, A.NODE_REFIT_PENDING_EDIT), (DEVICE, 0)):
                step += 1
                m = np.eye(4, dtype=f32)
                m[:3, 3] = (0.25 * step, -0.5, 0.125 * step)
                move(a, b, s, [(ground, m), (4, _moved(s.nodes[4].local_transform, 4 + step))])
                assert_path(a, path, reason)
                check(a, b, oracle, s, f"opacity {opacity}, path {path}")
    finally:
        a.close(); b.close()


@gpu
@pytest.mark.parametrize("policy", [A.REFIT_POLICY_OFF, A.REFIT_POLICY_MEASURE], ids=["policy_off", "measure_only"])
def test_unmoved_transforms_reproduce_the_tree(halart, policy):
    """with a policy on nothing moved means nothing is refitted and nothing measured; a moved tree is measured as on the twin"""
    for instancing in (True, False):
        s = copy.deepcopy(instance_scene(17, True))
        a, b = twins(halart, s, instancing=instancing)
        try:
            for r in (a, b):
                r.set_refit_policy(policy)
            before, measured = state(a), a.tree_quality()[1]
            idx = list(range(19))
            a.bind_nodes(idx)
            a.refit_nodes(np.stack([s.nodes[k].local_transform for k in idx]))
            assert_path(a, DEVICE)
            assert state(a) == before
            assert a.tree_quality()[1] == measured
            if policy != A.REFIT_POLICY_OFF:
                move(a, b, s, [(k, _moved(s.nodes[k].local_transform, k)) for k in idx])
                assert_path(a, DEVICE)
                assert_same_state(a, b, f"moved, instancing {instancing}")
                assert a.tree_quality()[1] == b.tree_quality()[1] == measured + 1  # one refit that moved a tree: one measurement
        finally:
            a.close(); b.close()


# ---- reclassification -------------------------------------------------------------------------------------------------------------------
@gpu
def test_squashed_node_is_reclassified_and_restored(halart, oracle):
    s = copy.deepcopy(instance_scene(17, True))
    a, b = twins(halart, s)
    try:
        a.bind_nodes([6])
        good = np.array(s.nodes[6].local_transform, dtype=f32)
        flat = good.copy()
        flat[:3, 1] = 0.0  # determinant 0
        move(a, b, s, [(6, flat)])
        assert_path(a, HOST, A.NODE_REFIT_CLASSIFICATION)
        assert a.bvh_info().instance_ref_count == 16
        check(a, b, oracle, s, "squashed")
        move(a, b, s, [(6, good)])
        assert_path(a, HOST, A.NODE_REFIT_CLASSIFICATION)
        assert a.bvh_info().instance_ref_count == 17
        check(a, b, oracle, s, "restored")
        move(a, b, s, [(6, _moved(good, 6))])  # the analysis follows the rebuilt trees
        assert_path(a, DEVICE)
        check(a, b, oracle, s, "after the rebuilds")
    finally:
        a.close(); b.close()


@gpu
def test_nan_translation_behaves_as_on_the_twin(halart):
    s = copy.deepcopy(instance_scene(17, True))
    a, b = twins(halart, s)
    try:
        a.bind_nodes([6])
        bad = np.array(s.nodes[6].local_transform, dtype=f32)
        bad[0, 3] = np.nan

        def outcome(fn):
            try:
                fn()
                return None
            except Exception as e:  # noqa: BLE001
                return str(e)

        def ordinary():
            b.update_node_transform(6, bad)
            b.refit()

        got, want = outcome(lambda: a.refit_nodes(bad[None])), outcome(ordinary)
        assert got == want
        if got is None:
            assert_path(a, HOST, A.NODE_REFIT_CLASSIFICATION)
        # (the trees are compared, not rendered: no image is defined for a scene with a NaN in it)
        assert_same_state(a, b, "NaN translation" if got is None else "NaN translation, both calls refused: " + got)
    finally:
        a.close(); b.close()


# ---- fallbacks --------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("what", ["material", "node", "key"])
def test_pending_edits_and_keys_take_the_host_path(halart, oracle, what):
    s = copy.deepcopy(instance_scene(17, True))
    a, b = twins(halart, s)
    try:
        a.bind_nodes([5, 12])
        reason = A.NODE_REFIT_PENDING_EDIT
        if what == "material":
            s.materials[0] = H.HalaMaterial(type=0, base_color=(0.2, 0.5, 0.9))
            for r in (a, b):
                r.update_material(0, s.materials[0])
        elif what == "node":
            s.nodes[9].local_transform = _moved(s.nodes[9].local_transform, 9)
            for r in (a, b):
                r.update_node_transform(9, s.nodes[9].local_transform)
        else:  # a key on an unbound node, the shutter off: the node stays at its open key
            for r in (a, b):
                r.set_node_keys(8, s.nodes[8].local_transform, _moved(s.nodes[8].local_transform, 8))
            reason = A.NODE_REFIT_SHUTTER_KEYS
        move(a, b, s, [(k, _moved(s.nodes[k].local_transform, k)) for k in (5, 12)])
        assert_path(a, HOST, reason)
        check(a, b, oracle, s, what)
        if what != "key":  # the edit is applied: the next call is the device's again
            move(a, b, s, [(k, _moved(s.nodes[k].local_transform, k + 1)) for k in (5, 12)])
            assert_path(a, DEVICE)
            check(a, b, oracle, s, what + ", then the device path")
    finally:
        a.close(); b.close()


@gpu
def test_build_options_set_since_the_build_take_the_host_path(halart, oracle):
    """instancing switched off on a committed two-level scene: the ordinary refit classifies by the new rule and builds one flattened
    tree; refit_nodes must leave that to it, and follow on the device afterwards"""
    s = copy.deepcopy(instance_scene(17, True))
    a, b = twins(halart, s)
    try:
        a.bind_nodes([5, 12])
        for r in (a, b):
            r.set_build_options(instancing=False, instance_levels="gpu")
        move(a, b, s, [(k, _moved(s.nodes[k].local_transform, k)) for k in (5, 12)])
        assert_path(a, HOST, A.NODE_REFIT_PENDING_EDIT)
        assert a.bvh_info().instance_ref_count == 0
        check(a, b, oracle, s, "flattened by the new options", two_level=False)
        move(a, b, s, [(k, _moved(s.nodes[k].local_transform, k + 1)) for k in (5, 12)])
        assert_path(a, DEVICE)
        check(a, b, oracle, s, "then the device path on the one tree", two_level=False)
    finally:
        a.close(); b.close()


@gpu
def test_bound_node_that_carries_the_camera(halart, oracle):
    s = copy.deepcopy(instance_scene(4, True))
    cam = s.nodes.pop()
    s.nodes.append(H.HalaNode(name="dolly"))
    cam.parent = len(s.nodes) - 1
    s.nodes.append(cam)
    a, b = twins(halart, s)
    try:
        dolly = len(s.nodes) - 2
        a.bind_nodes([dolly])
        m = np.eye(4, dtype=f32)
        m[:3, 3] = (0.5, -0.25, 0.75)
        move(a, b, s, [(dolly, m)])
        assert_path(a, HOST, A.NODE_REFIT_CAMERA_OR_LIGHT)
        check(a, b, oracle, s, "camera below the bound node")
    finally:
        a.close(); b.close()


# ---- the host mirror --------------------------------------------------------------------------------------------------------------------
@gpu
def test_ordinary_edits_after_a_device_path_call(halart, oracle):
    s = copy.deepcopy(instance_scene(17, True))
    a, b = twins(halart, s)
    try:
        original = state(a)
        first = {k: np.array(s.nodes[k].local_transform, dtype=f32) for k in (5, 2)}
        a.bind_nodes([5, 2])
        move(a, b, s, [(k, _moved(first[k], k)) for k in (5, 2)])
        assert_path(a, DEVICE)
        s.nodes[11].local_transform = _moved(s.nodes[11].local_transform, 11)  # another node, the ordinary way
        for r in (a, b):
            r.update_node_transform(11, s.nodes[11].local_transform)
            r.refit()
        check(a, b, oracle, s, "ordinary edit after the device path")
        move(a, b, s, [(k, _moved(first[k], k + 2)) for k in (5, 2)])
        assert_path(a, DEVICE)
        # everything back to the first transforms through the ordinary path: a stale `before` would find nothing moved
        back = dict(first)
        back[11] = instance_scene(17, True).nodes[11].local_transform
        for k, m in back.items():
            s.nodes[k].local_transform = m
            for r in (a, b):
                r.update_node_transform(k, m)
        a.refit(); b.refit()
        assert check(a, b, oracle, s, "moved back") == original
    finally:
        a.close(); b.close()


@gpu
def test_temporal_history_across_a_device_path_call(halart):
    s = copy.deepcopy(instance_scene(17, True))
    a, b = twins(halart, s)
    try:
        for r in (a, b):
            r.set_aovs(position=True, ids=True)
            r.set_temporal()
        a.bind_nodes([5, 2])
        move(a, b, s, [(k, _moved(s.nodes[k].local_transform, k)) for k in (5, 2)])  # the mirror is stale when the capture reads it
        assert_path(a, DEVICE)
        for r in (a, b):
            images(r)
            r.temporal_capture()
        move(a, b, s, [(k, _moved(s.nodes[k].local_transform, k + 1)) for k in (5, 2)])
        assert_path(a, DEVICE)
        out = []
        for r in (a, b):
            images(r)
            r.temporal_resolve()
            out.append((r.read_temporal(0).tobytes(), r.read_temporal(1).tobytes()))
        assert out[0] == out[1]
    finally:
        a.close(); b.close()


@gpu
def test_pose_rig_after_refit_nodes(halart, tmp_path):
    import rig_ref as R
    import test_scene_edits as SE
    from hala_renderer_amd.native_scene import NativeScene
    path = R.save(R.character_doc(), tmp_path / "character.gltf")
    base = SE.base_of("cornell")
    nat = NativeScene(path)
    py = H.HalaScene.new(path)
    carries = [n.camera_index != H.scene.INVALID or n.light_index != H.scene.INVALID for n in py.nodes]
    for k in reversed(range(len(py.nodes))):  # children come behind their parents: a camera or light below a node counts for the node
        if carries[k] and py.nodes[k].parent is not None:
            carries[py.nodes[k].parent] = True
    node = [k for k, n in enumerate(py.nodes) if n.mesh_index != H.scene.INVALID and not carries[k]][0]
    rs = [SE.make(halart, base, scene=nat), SE.make(halart, base, scene=nat)]
    try:
        for r in rs:
            r.set_rig(nat.rig)
            r.refit()  # the deformers the rig registered are posed: nothing is pending
        a, b = rs
        a.bind_nodes([node])
        m = _moved(py.nodes[node].local_transform, 1)
        a.refit_nodes(m[None])
        b.update_node_transform(node, m); b.refit()
        assert_path(a, DEVICE)  # the host mirror is stale when pose_rig writes the locals
        assert_same_state(a, b, "before the pose")
        for r in rs:
            r.pose_rig(0, 0.625)
            r.refit()
        assert_same_state(a, b, "posed")
        assert a.rig_pose()["locals"].tobytes() == b.rig_pose()["locals"].tobytes()
        for r in rs:
            r.update(); r.update(); r.render()
        assert [a.read_image(k).tobytes() for k in range(4)] == [b.read_image(k).tobytes() for k in range(4)]
    finally:
        for r in rs:
            r.close()
        nat.close()


# ---- device input -----------------------------------------------------------------------------------------------------------------------
@gpu
def test_device_tensor_equals_the_host_array(halart, oracle):
    import torch
    s = copy.deepcopy(instance_scene(17, True))
    a, b = twins(halart, s)
    try:
        idx = list(range(17))
        moved = np.stack([_moved(s.nodes[k].local_transform, k) for k in idx])
        a.bind_nodes(idx); b.bind_nodes(idx)
        stream = torch.cuda.ExternalStream(a.get_stream())
        half = torch.from_numpy(NB.column_major(moved) * f32(0.5)).cuda()
        with torch.cuda.stream(stream):
            d = half * 2.0  # produced on the renderer's stream (exact)
            a.refit_nodes(d)
        b.refit_nodes(moved)
        assert_path(a, DEVICE); assert_path(b, DEVICE)
        for k in idx:
            s.nodes[k].local_transform = moved[k]
        check(a, b, oracle, s, "device tensor")
        # the host's copy of the locals followed the device array: an ordinary refit finds nothing to move
        before = state(a)
        a.refit()
        assert state(a) == before
    finally:
        a.close(); b.close()


# ---- binding ----------------------------------------------------------------------------------------------------------------------------
@gpu
def test_binding_rules(halart):
    s = instance_scene(5, True)
    r = make_renderer(halart, s, W, HGT, build=dict(instancing=True, instance_levels="gpu"))
    try:
        want = images(r)
        with pytest.raises(Exception, match="no nodes are bound"):
            r.refit_nodes(np.zeros((0, 4, 4), dtype=f32))
        with pytest.raises(Exception, match="given twice"):
            r.bind_nodes([1, 2, 1])
        with pytest.raises(Exception, match="does not exist"):
            r.bind_nodes([1, len(s.nodes)])
        r.set_node_keys(3, s.nodes[3].local_transform, _moved(s.nodes[3].local_transform, 3))
        with pytest.raises(Exception, match="shutter keys"):
            r.bind_nodes([3])
        r.set_node_keys(3, None, None)
        assert r.node_refit_status().bound_nodes == 0
        r.reset_accumulation()
        assert images(r) == want  # every refusal left the renderer as it was
        r.bind_nodes([1, 2])
        assert r.node_refit_status().bound_nodes == 2
        r.bind_nodes([])
        assert r.node_refit_status().bound_nodes == 0
        with pytest.raises(Exception, match="no nodes are bound"):
            r.refit_nodes(np.zeros((0, 4, 4), dtype=f32))
        r.bind_nodes([1, 2])
        r.commit()
        assert r.node_refit_status().bound_nodes == 0
        with pytest.raises(Exception, match="no nodes are bound"):
            r.refit_nodes(np.zeros((0, 4, 4), dtype=f32))
        assert images(r) == want  # (the commit restarted the accumulation)
    finally:
        r.close()
    fresh = halart.HalaRenderer("unbound", W, HGT, 2, 1, False, False, False, 0)
    try:
        fresh.set_scene(s)
        with pytest.raises(Exception, match="acceleration structure is none"):
            fresh.bind_nodes([1])
    finally:
        fresh.close()


# ---- frames in flight -------------------------------------------------------------------------------------------------------------------
@gpu
def test_frames_in_flight_around_the_call(halart, oracle):
    s = copy.deepcopy(instance_scene(17, True))
    r = make_renderer(halart, s, W, HGT, build=dict(instancing=True, instance_levels="gpu"))
    try:
        r.set_frames_in_flight(2)
        idx = list(range(17))
        r.bind_nodes(idx)
        for _ in range(4):
            r.update()
        moved = np.stack([_moved(s.nodes[k].local_transform, k) for k in idx])
        r.refit_nodes(moved)
        assert_path(r, DEVICE)
        for k in idx:
            s.nodes[k].local_transform = moved[k]
        want, _ = oracle_scene(oracle, s).render(W, HGT, frames=4)
        assert images(r, frames=4) == [w.tobytes() for w in want]
    finally:
        r.close()
