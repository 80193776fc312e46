"""The instance levels of a two-level tree built on the GPU (hala_rt_build_options::instance_levels = 1; csrc/bvh_instances.hip,
RENDER_SPEC 4.5) against the host build (instance_levels = 0, csrc/bvh_tlas.cpp) and the oracle.  The spec fixes the format of the
levels, not their shape: the InstRef records, the scene bounds and every image must be the host path's and the oracle's byte for byte, the
tree must pass the oracle's structural check, and the oracle's walk of the downloaded tree must count the steps the GPU counts.

Item counts (instanced instances + one for the world-space tree over the flattened ones, where the scene has one): 2, 3 and 4 (one
node, partly filled), 5 (a second level), 17, 257 (past one 256-thread block in every kernel), 4100 with the automatic builder (past the
4096 items from which it is full-sweep SAH), 257 also with PLOC and with LBVH selected.  A scene with ONE item cannot be made through
the API: an instance is only instanced when a second one references its primitive, and that one is either instanced too (two items) or
flattened into the world tree (whose item is the second); the single-node path of the builder therefore only has the cases of two to
four items here."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

import hala_renderer_amd as H
from conftest import ROOT
from hala_renderer_amd import _abi as A
from hala_renderer_amd import scenes
from test_gpu_parity import make_renderer, validate_tree
from test_oracle_render import random_rays

gpu = pytest.mark.gpu
f32 = np.float32
W, HGT = 32, 24
MAX_LEVELS = 96  # csrc/bvh_build_impl.h: kMaxLevels


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_build_options_layout_and_mirrors():
    assert C.sizeof(A.BuildOptions) == 32
    assert A.BuildOptions.instance_levels.offset == 24 and A.BuildOptions.reserved.offset == 28 and A.BuildOptions.reserved.size == 4
    assert H.HalaRenderer.INSTANCE_LEVELS == {None: 0, "host": 0, "gpu": 1}
    header = open(os.path.join(ROOT, "include", "halart.h")).read()
    body = header[header.index("typedef struct hala_rt_build_options {"):header.index("} hala_rt_build_options;")]
    fields = [ln.split("/*")[0].strip() for ln in body.splitlines() if ln.strip().startswith("uint32_t")]
    assert fields == ["uint32_t builder;", "uint32_t ploc_tail;", "uint32_t ploc_look_every;", "uint32_t collapse_look_every;", "uint32_t instancing;",
                      "uint32_t texture_bundles;", "uint32_t instance_levels;", "uint32_t reserved[1];"]
    rust = open(os.path.join(ROOT, "rust", "hala-renderer-halart", "src", "lib.rs")).read()
    assert "pub texture_bundles: u32, pub instance_levels: u32, pub reserved: [u32; 1] }" in rust


@gpu
def test_the_option_is_taken_and_checked(halart):
    r = halart.HalaRenderer("levels", 16, 16, 2, 1, False, False, False, 0)
    try:
        set_options = lambda o: r._lib.hala_rt_set_build_options(r._h, C.byref(o))  # noqa: E731
        assert set_options(A.BuildOptions(instance_levels=1)) == 0  # (the parent commit refuses it: the word was reserved)
        assert set_options(A.BuildOptions(instance_levels=0)) == 0
        assert set_options(A.BuildOptions(instance_levels=2)) != 0
        assert halart.last_error().startswith("Invalid build options.")
        o = A.BuildOptions(instance_levels=1)
        o.reserved[0] = 1
        assert set_options(o) != 0 and "reserved" in halart.last_error()
        with pytest.raises(KeyError):
            r.set_build_options(instance_levels="device")
        r.set_build_options(instancing=True, instance_levels="gpu")
    finally:
        r.close()


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
def _prim(tri_pos):
    """a primitive of the given triangles ([T, 3, 3]), flat-shaded"""
    pos = np.asarray(tri_pos, dtype=f32)
    nrm = np.cross(pos[:, 1] - pos[:, 0], pos[:, 2] - pos[:, 0]).astype(np.float64)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    p = H.HalaPrimitive(indices=np.arange(3 * len(pos), dtype=np.uint32), vertices=scenes._vertices(pos.reshape(-1, 3), np.repeat(nrm, 3, axis=0)))
    p.material_index = 0
    return p


def _box():  # 12 triangles
    c = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)])
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return _prim([c[[q[i] for i in t]] for q in quads for t in ((0, 1, 2), (0, 2, 3))])


def _tetra():  # 4 triangles
    c = np.array([[0.5, 0.5, 0.5], [-0.5, -0.5, 0.5], [-0.5, 0.5, -0.5], [0.5, -0.5, -0.5]])
    return _prim([c[list(t)] for t in ((0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2))])


def _transform(rs, k, half):
    """the k-th instance's local transform: rotated and non-uniformly scaled; every third one mirrored, every fifth one sheared"""
    ry, rx = rs.uniform(-np.pi, np.pi), rs.uniform(-1.0, 1.0)
    cy, sy, cx, sx = np.cos(ry), np.sin(ry), np.cos(rx), np.sin(rx)
    R = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    scale = rs.uniform(0.4, 1.2, 3)
    if k % 3 == 1:
        scale[0] = -scale[0]
    m = np.eye(4)
    m[:3, :3] = R @ np.diag(scale)
    if k % 5 == 2:
        m[0, 1] += 0.35
    m[:3, 3] = rs.uniform(-half, half, 3)
    return m.astype(f32)


def instance_scene(n_inst, world, seed=0, same=False):
    """n_inst instanced instances of a 12-triangle box (the last two of a 4-triangle tetrahedron from four on); every seventh one hangs
    below the one before it (nested).  world: also a ground quad that is referenced once and one more box squashed flat (determinant 0):
    both are flattened into the world-space tree, which is one more item.  same: every instance gets the first one's transform"""
    rs = np.random.RandomState(9000 + 31 * n_inst + seed)
    half = 1.5 * max(n_inst, 2) ** (1.0 / 3.0)
    s = H.HalaScene()
    s.materials = [H.HalaMaterial(type=0, base_color=(0.7, 0.6, 0.5))]
    s.meshes = [H.HalaMesh([_box()]), H.HalaMesh([_tetra()])]
    first = None
    for k in range(n_inst):
        m = _transform(rs, k, half)
        first = m if first is None else first
        nested = k % 7 == 3 and not same
        if nested:
            m[:3, 3] *= f32(0.25)  # relative to its parent
        s.nodes.append(H.HalaNode(name=f"inst_{k}", mesh_index=1 if n_inst >= 4 and k >= n_inst - 2 else 0, parent=k - 1 if nested else None,
                                  local_transform=first.copy() if same else m))
    if world:
        e = f32(half * 1.5)
        s.meshes.append(H.HalaMesh([_prim([[[-e, -e, -e], [e, -e, e], [e, -e, -e]], [[-e, -e, -e], [-e, -e, e], [e, -e, e]]])]))
        s.nodes.append(H.HalaNode(name="ground", mesh_index=2))
        flat = np.eye(4, dtype=f32)
        flat[1, 1] = 0.0
        flat[:3, 3] = (0.25 * half, 0.5 * half, -0.25 * half)
        s.nodes.append(H.HalaNode(name="flat", mesh_index=0, local_transform=flat))
    d = 3.0 * half + 4.0
    s.nodes.append(H.HalaNode(name="camera", camera_index=0, local_transform=scenes.look_at_node_transform((0.3 * d, 0.4 * d, d), (0.0, 0.0, 0.0))))
    s.cameras = [H.HalaPerspectiveCamera(aspect=W / HGT, yfov=0.7, znear=0.1)]
    return s


def oracle_scene(oracle, s):
    oracle.set_instancing(True)
    try:
        return oracle.OracleScene(s)
    finally:
        oracle.set_instancing(False)


def renderer(halart, s, levels, builder=None):
    return make_renderer(halart, s, W, HGT, build=dict(instancing=True, instance_levels=levels, builder=builder))


def images(r, frames=2):
    for _ in range(frames):
        r.update()
    r.render()
    return [r.read_image(k).tobytes() for k in range(4)]


def levels_state(r):
    """what the two paths must agree on, and the instance levels themselves"""
    i = r.bvh_info()
    nodes, tris = r.download_bvh()
    return dict(refs=r.download_instance_refs().tobytes(), bounds=(np.array(i.scene_min, dtype=f32).tobytes(), np.array(i.scene_max, dtype=f32).tobytes()),
                top=nodes.reshape(-1, 16)[:i.instance_node_count].copy(), count=i.instance_node_count, ref_count=i.instance_ref_count, nodes=nodes.reshape(-1, 16), tris=tris,
                depth=i.max_depth)


_CASES = {}


def case(halart, oracle, n_inst, world):
    """scene, oracle scene, the oracle's images, a ray batch and what the host path gives: once per scene, shared by the builders"""
    key = (n_inst, world)
    if key not in _CASES:
        s = instance_scene(n_inst, world)
        osc = oracle_scene(oracle, s)
        want, _ = osc.render(W, HGT, frames=2)
        omn, omx = osc.bounds()
        pad = (omx - omn) * 0.2
        rays = np.concatenate([random_rays(1500, omn - pad, omx + pad, 11 + n_inst), osc.camera_rays(W, HGT, 0)])
        rh = renderer(halart, s, "host")
        host = levels_state(rh)
        host["images"] = images(rh)
        rh.close()
        _CASES[key] = (s, osc, [w.tobytes() for w in want], rays, host)
    return _CASES[key]


ITEM_CASES = [(k, None) for k in (2, 3, 4, 5, 17, 257, 4100)] + [(257, "ploc"), (257, "lbvh")]


@gpu
@pytest.mark.parametrize("world", [True, False], ids=["world", "noworld"])
@pytest.mark.parametrize("items,builder", ITEM_CASES, ids=[f"{k}-{b or 'auto'}" for k, b in ITEM_CASES])
def test_gpu_built_levels_equal_the_host_path_and_the_oracle(halart, oracle, items, builder, world):
    n_inst = items - 1 if world else items
    s, osc, want, rays, host = case(halart, oracle, n_inst, world)
    r = renderer(halart, s, "gpu", builder)
    try:
        got = levels_state(r)
        assert got["ref_count"] == host["ref_count"] == n_inst and 1 <= got["count"] < max(items, 2)
        rc, depth, two_level = validate_tree(oracle, osc, r)
        assert rc == 0 and two_level
        assert got["refs"] == host["refs"]
        assert got["bounds"] == host["bounds"]
        refs = r.download_instance_refs()
        for mode in (0, 1):  # closest hit, any hit: nodes visited and triangles tested, ray for ray the oracle's on this tree
            hits, cnt = r.trace_rays_host(rays, mode, count_steps=True)
            ohits, ocnt = oracle.trace_on_bvh(got["nodes"].reshape(-1), got["tris"], rays, mode, refs)
            assert cnt == ocnt, mode
            assert np.array_equal(hits["t"], ohits["t"])
        mine = images(r)
        assert mine == want
        assert mine == host["images"]
        if items <= 4:  # one node in both trees: the same box, the same children with the same plane bytes, in whatever slots
            a, b = got["top"], host["top"]
            assert len(a) == len(b) == 1
            assert a[0, :4].tobytes() == b[0, :4].tobytes()  # pmin and the three exponents

            def children(n):
                out = set()
                for c in range(4):
                    if n[12 + c] != 0xFFFFFFFF:
                        out.add((int(n[12 + c]),) + tuple(int((n[4 + w] >> (8 * c)) & 0xff) for w in range(6)))
                return out

            assert children(a[0]) == children(b[0]) and len(children(a[0])) == items
    finally:
        r.close()


@gpu
def test_instances_with_one_transform(halart, oracle):
    """64 instances in one place: equal Morton keys, which the hierarchy splits by index"""
    s = instance_scene(64, False, same=True)
    osc = oracle_scene(oracle, s)
    r = renderer(halart, s, "gpu")
    try:
        i = r.bvh_info()
        assert i.instance_ref_count == 64 and 1 <= i.max_depth <= MAX_LEVELS
        assert validate_tree(oracle, osc, r)[0] == 0
        want, _ = osc.render(W, HGT, frames=2)
        assert images(r) == [w.tobytes() for w in want]
    finally:
        r.close()


# ---- refit -----------------------------------------------------------------------------------------------------------------------------
def _moved(m, k):
    m = np.array(m, dtype=f32).copy()
    m[:3, 3] += np.array([0.5 + 0.125 * (k % 4), -0.25, 0.375 * ((k % 3) - 1)], dtype=f32)
    return m


@gpu
def test_refit_rebuilds_the_levels_on_the_gpu(halart, oracle):
    """17 instanced nodes and a world tree.  One node moves, then all: after each refit the tree is valid, InstRef records and bounds are
    the host path's, the images the oracle's, and no tree below the instance levels changed a byte.  A refit without an edit reproduces the
    levels; one that squashes an instance flat reclassifies it (a rebuild) and still renders the oracle's images."""
    n_inst, items = 17, 18
    s = copy.deepcopy(instance_scene(n_inst, True))
    rg, rh = renderer(halart, s, "gpu"), renderer(halart, s, "host")
    try:
        before = levels_state(rg)
        for which in ([5], list(range(n_inst))):
            for k in which:
                s.nodes[k].local_transform = _moved(s.nodes[k].local_transform, k)
                for r in (rg, rh):
                    r.update_node_transform(k, s.nodes[k].local_transform)
            rg.refit(); rh.refit()
            g, h = levels_state(rg), levels_state(rh)
            osc = oracle_scene(oracle, s)
            assert validate_tree(oracle, osc, rg)[0] == 0
            assert g["refs"] == h["refs"] and g["refs"] != before["refs"] and g["bounds"] == h["bounds"]
            assert g["tris"].tobytes() == before["tris"].tobytes()
            assert g["nodes"][items:].tobytes() == before["nodes"][items:].tobytes()  # the trees start behind the reserved instance levels
            want, _ = osc.render(W, HGT, frames=2)
            assert images(rg) == [w.tobytes() for w in want]
        rg.refit()
        again = levels_state(rg)
        assert again["count"] == g["count"] and again["top"].tobytes() == g["top"].tobytes() and again["refs"] == g["refs"]
        flat = np.array(s.nodes[3].local_transform, dtype=f32).copy()
        flat[:3, 1] = 0.0  # determinant 0
        s.nodes[3].local_transform = flat
        rg.update_node_transform(3, flat)
        rg.refit()
        assert rg.bvh_info().instance_ref_count == n_inst - 1
        osc = oracle_scene(oracle, s)
        assert validate_tree(oracle, osc, rg)[0] == 0
        want, _ = osc.render(W, HGT, frames=2)
        assert images(rg) == [w.tobytes() for w in want]
    finally:
        rg.close(); rh.close()


@gpu
def test_shutter_steps_rebuild_the_levels_on_the_gpu(halart):
    """node keys on three instanced nodes, a step per frame: every step refits, which rebuilds the instance levels; images do not
    depend on the tree"""
    s = instance_scene(17, True)
    out = []
    for levels in ("gpu", "host"):
        r = renderer(halart, s, levels)
        try:
            for k in (2, 8, 16):
                r.set_node_keys(k, s.nodes[k].local_transform, _moved(s.nodes[k].local_transform, k))
            r.set_shutter(0.0, 1.0, time_stride=1)
            r.refit()
            out.append(images(r, frames=4))
            assert r.shutter_status().steps >= 3  # the refit stands at step 0; each later frame takes a step, which refits
        finally:
            r.close()
    assert out[0] == out[1]


@gpu
def test_two_commits_build_the_same_levels(halart, oracle):
    s = case(halart, oracle, 4100, False)[0]
    r = renderer(halart, s, "gpu")
    try:
        a = levels_state(r)
        r.commit()
        b = levels_state(r)
        assert a["count"] == b["count"] and a["depth"] == b["depth"] and a["top"].tobytes() == b["top"].tobytes() and a["refs"] == b["refs"]
    finally:
        r.close()
