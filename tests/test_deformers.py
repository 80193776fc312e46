"""GPU-resident deformers (docs/RENDER_SPEC.md 17; include/halart.h "Deformers"): morph targets and a four-influence skin per primitive,
posed by k_deform (csrc/deform.hip) ahead of hala_rt_refit.

CPU tier: the numpy-float32 twin (tests/deform_ref.py) against a float64 evaluation of the same formulas and on its exact cases; the
layout of hala_deformer_desc; the header's contract; the oracle's render of the posed Cornell scene differs from the rest scene's.
GPU tier, every comparison by bytes: the kernel equals the twin (read_vertices) across wave, workgroup and arena edges; after the refit
the renderer equals the oracle's render of the scene holding the twin's vertices, on both tree forms; the same bytes as the
update_vertices path; nothing happens before the refit; pose after pose starts from the rest pose; refusals and the overflow to a
non-finite position change nothing; lifetime across set_scene / commit; temporal history."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import deform_ref as D
import scene_edits as E
import test_scene_edits as SE
from conftest import ROOT
from hala_renderer_amd import _abi as A
from hala_renderer_amd import scenes
from hala_renderer_amd.scene import HalaMesh, HalaNode, HalaPrimitive

gpu = pytest.mark.gpu
f32 = np.float32
U = 2.0 ** -24  # unit roundoff of float32
TALL, SHORT = 2, 1  # meshes of the Cornell base: the tall block (one node), the short block (three nodes: instanced on a two-level tree)


# ---- the Cornell rigs -------------------------------------------------------------------------------------------------------------------
def cornell():
    return SE.base_of("cornell")


_RIGS = {}


def cornell_rigs():
    """tall block: 2 targets with normal deltas + 3 joints (weights that sum to 1 exactly); short block: 3 targets with tangent deltas"""
    if not _RIGS:
        s = cornell().scene
        nv = len(s.meshes[TALL].primitives[0].vertices)
        _RIGS[TALL] = D.random_rig(nv, targets=2, joint_count=3, normals=True, seed=1, scale=60.0, dyadic=True)
        _RIGS[SHORT] = D.random_rig(len(s.meshes[SHORT].primitives[0].vertices), targets=3, tangents=True, seed=2, scale=50.0)
    return _RIGS


def cornell_pose(k):
    """pose k of both blocks -> {mesh: pose}"""
    s = cornell().scene
    out = {}
    for mesh, rig in cornell_rigs().items():
        pos = s.meshes[mesh].primitives[0].vertices["position"].astype(np.float64)
        out[mesh] = D.random_pose(rig, seed=10 * k + mesh, centre=0.5 * (pos.min(0) + pos.max(0)), scale=100.0)
    return out


def posed_ops(poses):
    """the ("vertices", ...) operations of tests/scene_edits.py that carry the twin's output of `poses`"""
    s = cornell().scene
    return [("vertices", mesh, 0, D.pose_vertices(s.meshes[mesh].primitives[0].vertices, cornell_rigs()[mesh], pose)) for mesh, pose in sorted(poses.items())]


def register(r, meshes=(TALL, SHORT)):
    for mesh in meshes:
        r.set_deformer(mesh, 0, **cornell_rigs()[mesh])


def pose(r, poses):
    for mesh, p in sorted(poses.items()):
        r.update_deformer(mesh, 0, **p)


_ORACLE = {}


def oracle_of(oracle, key, scene_fn, frames):
    """the oracle's images of a scene, rendered once per (key, frames) and shared"""
    if (key, frames) not in _ORACLE:
        _ORACLE[key, frames] = SE.oracle_images(oracle, cornell(), scene_fn(), frames)
    return _ORACLE[key, frames]


def rest_images(oracle, frames):
    return oracle_of(oracle, "rest", lambda: cornell().scene, frames)


def posed_images(oracle, k, frames):
    return oracle_of(oracle, f"pose{k}", lambda: E.apply_to_scene(cornell().scene, posed_ops(cornell_pose(k))), frames)


# ---- CPU tier ---------------------------------------------------------------------------------------------------------------------------
TWIN_CASES = [(257, 3, 5, True, True), (64, 0, 4, False, False), (65, 2, 0, True, False), (100, 1, 1, False, True), (33, 3, 256, True, True)]


@pytest.mark.parametrize("case", TWIN_CASES, ids=lambda c: "V{}-T{}-J{}".format(*c[:3]))
def test_twin_agrees_with_float64(case):
    """|twin - float64| <= 16 * 2^-24 * (sum of the absolute values of all terms) per component of position, normal and tangent.  The
    factor counts the roundings a term of RENDER_SPEC 17 passes through, not a measured error: with at most 3 targets a delta is rounded
    once in `w * delta` and at most 3 times by the sums of the morph, a matrix entry once in `w * J` and 4 times by the sums of M, and
    the transform rounds a product once and sums 3 times: 13, below 16."""
    nv, nt, nj, nrm, tan = case
    _, rest = D.strip(nv, seed=nv)
    rig = D.random_rig(nv, targets=nt, joint_count=nj, normals=nrm, tangents=tan, seed=nv + 1)
    assert nt <= 3
    worst = 0.0
    for k in range(3):
        p = D.random_pose(rig, seed=k, zero_some=k > 0, centre=(10.0, 0.5, 0.0))
        got = D.pose_vertices(rest, rig, p)
        kw = dict(targets=rig["targets"], normal_targets=rig["normal_targets"], tangent_targets=rig["tangent_targets"], morph_weights=p["morph_weights"],
                  joints=rig["joints"] if nj else None, weights=rig["weights"] if nj else None, joint_matrices=p["joint_matrices"])
        want = D.deform64(rest, **kw)
        mag = D.deform64(rest, magnitudes=True, **kw)
        for name, w, m in zip(("position", "normal", "tangent"), want, mag):
            err = np.abs(got[name].astype(np.float64) - w)
            bound = 16.0 * U * m
            print(f"{case} pose {k} {name}: max error / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all(), (case, k, name)
        assert got["tex_coord"].tobytes() == rest["tex_coord"].tobytes()
    assert worst > 0.0  # float32 does round somewhere


def test_twin_exact_cases():
    _, rest = D.strip(70, seed=5)
    rig = D.random_rig(70, targets=3, joint_count=4, normals=True, tangents=True, seed=6)
    # one target at weight 1: rest + delta
    got = D.deform(rest, rig["targets"][1:2], rig["normal_targets"][1:2], rig["tangent_targets"][1:2], [1.0])
    for name, key in (("position", "targets"), ("normal", "normal_targets"), ("tangent", "tangent_targets")):
        assert np.array_equal(got[name], rest[name] + rig[key][1])
    # position deltas only: normal and tangent are copied
    got = D.deform(rest, rig["targets"], None, None, [0.5, -1.0, 2.0])
    assert got["normal"].tobytes() == rest["normal"].tobytes() and got["tangent"].tobytes() == rest["tangent"].tobytes()
    # one joint at weight 1: the affine map in the stated association, 3 x 3 for normal and tangent
    m = D.random_pose(dict(targets=None, joint_count=1), seed=3)["joint_matrices"]
    j = np.zeros((70, 4), dtype=np.uint16)
    w = np.tile(np.array([1.0, 0.0, 0.0, 0.0], dtype=f32), (70, 1))
    got = D.deform(rest, joints=j, weights=w, joint_matrices=m)
    for name, translate in (("position", True), ("normal", False), ("tangent", False)):
        a = rest[name]
        for r in range(3):
            want = (m[0, r, 0] * a[:, 0] + m[0, r, 1] * a[:, 1]) + m[0, r, 2] * a[:, 2]
            if translate:
                want = want + m[0, r, 3]
            assert want.dtype == f32 and np.array_equal(got[name][:, r], want), (name, r)
    # all weights 0 and the identity palette with weights that sum to 1 exactly: the rest pose (by value: 0 * y may be -0)
    dy = D.random_rig(70, targets=3, joint_count=4, seed=7, dyadic=True)
    got = D.pose_vertices(rest, dy, {})
    for name in ("position", "normal", "tangent", "tex_coord"):
        assert np.array_equal(got[name], rest[name]), name
    # zero-weight targets are skipped: their deltas do not matter, not even as 0 * inf
    wild = rig["targets"].copy(); wild[0] = np.inf; wild[2] = np.nan
    a = D.deform(rest, wild, None, None, [0.0, 0.75, 0.0])
    b = D.deform(rest, rig["targets"][1:2], None, None, [0.75])
    assert a.tobytes() == b.tobytes()
    # targets apply in ascending index, from the rest value
    p = rest["position"]
    want = (p + f32(0.3) * rig["targets"][0]) + f32(-1.7) * rig["targets"][2]
    assert np.array_equal(D.deform(rest, rig["targets"], None, None, [0.3, 0.0, -1.7])["position"], want)


def test_deformer_desc_layout_matches_the_header(tmp_path):
    fields = [n for n, _ in A.DeformerDesc._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "halart.h"\nint main(void) {\n  printf("%zu", sizeof(hala_deformer_desc));\n' +
                   "".join(f'  printf(" %zu", offsetof(hala_deformer_desc, {n}));\n' for n in fields) +
                   '  printf(" %d %d", HALA_MAX_MORPH_TARGETS, HALA_MAX_JOINTS);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == C.sizeof(A.DeformerDesc) == 64
    assert out[1:-2] == [getattr(A.DeformerDesc, n).offset for n in fields]
    assert out[-2:] == [A.MAX_MORPH_TARGETS, A.MAX_JOINTS] == [64, 256]
    for fn in ("hala_rt_set_deformer", "hala_rt_update_deformer", "hala_rt_clear_deformer", "hala_rt_read_vertices"):
        assert fn in A.EXPORTS and fn in A.PROTOTYPES, fn


def test_header_states_the_refit_contract_and_every_refusal():
    text = open(os.path.join(ROOT, "include", "halart.h")).read()

    def comment_of(fn):
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int " + fn + r"\(", text, flags=re.S)
        assert m, fn
        return re.sub(r"\s*\n \*\s*", " ", m.group(1))

    for fn, words in (
            ("hala_rt_set_deformer", ("before hala_rt_commit the call is refused", "become the rest pose", "a refit right after the call changes nothing",
                                      "replaces the first", "mesh or primitive does not exist", "above HALA_MAX_MORPH_TARGETS", "above HALA_MAX_JOINTS",
                                      "neither targets nor a skin", ">= joint_count", "not finite", "hala_rt_set_scene drops every deformer")),
            ("hala_rt_update_deformer", ("no device work", "Takes effect at the next hala_rt_refit", "keep accumulating", "has no deformer",
                                         "differs from the registered target_count", "joint_count from the registered joint_count", "not finite")),
            ("hala_rt_clear_deformer", ("restores the rest pose", "clear it first", "without temporal history", "Vertex position is not finite.",
                                        "stay exactly as they were", "fall back to the last applied ones", "stays pending")),
            ("hala_rt_read_vertices", ("behind everything enqueued on the renderer's stream", "any other", "committed scene"))):
        c = comment_of(fn)
        for w in words:
            assert w in c, (fn, w)


def test_the_oracle_render_of_the_posed_scene_is_not_vacuous(oracle):
    s = cornell().scene
    before = rest_images(oracle, 3)
    for k in (1, 2, 3):
        ops = posed_ops(cornell_pose(k))
        for op in ops:
            assert op[3].tobytes() != s.meshes[op[1]].primitives[0].vertices.tobytes()
            assert np.isfinite(op[3]["position"]).all()
        after = posed_images(oracle, k, 3)
        assert int(np.any(after[0] != before[0], axis=-1).sum()) > 30, k
    assert posed_images(oracle, 1, 3)[0].tobytes() != posed_images(oracle, 2, 3)[0].tobytes()


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------------------
def strip_scene(vertex_count, neighbours=False, seed=0):
    """the Cornell box plus mesh 3: the strip (primitive 0, or primitive 1 between two neighbours of 37 and 5 vertices)"""
    s = scenes.cornell_box(aspect=E.W / E.H_)
    prims = [HalaPrimitive(*D.strip(vertex_count, seed=seed), material_index=4)]
    if neighbours:
        prims = [HalaPrimitive(*D.strip(37, seed=91, origin=(0.0, 3.0, 0.0)), material_index=0)] + prims + \
                [HalaPrimitive(*D.strip(5, seed=92, origin=(0.0, -3.0, 0.0)), material_index=1)]
    s.meshes = list(s.meshes) + [HalaMesh(prims)]
    s.nodes = list(s.nodes) + [HalaNode(name="strip", mesh_index=3, local_transform=E._translate((20.0, 200.0, 150.0)))]
    return s


# (vertices, targets, joints, normal deltas, tangent deltas, neighbours): V over the wave edge (63, 64, 65), the workgroup edge (257) and
# several workgroups (1031); 0 / 1 / 3 / the maximum of targets; 0 / 1 / 2 / 256 joints; targets only, skin only, both
KERNEL_CASES = [
    (1, 1, 1, False, False, False),
    (63, 3, 0, True, True, False),
    (64, 0, 2, False, False, False),
    (65, 64, 256, True, False, False),
    (257, 1, 256, False, True, False),
    (257, 0, 1, False, False, False),
    (1031, 3, 2, True, True, False),
    (1031, 64, 0, False, False, False),
    (1, 0, 256, False, False, False),
    (65, 3, 2, True, True, True),
    (64, 1, 0, True, False, False),
    (63, 64, 256, True, True, True),
]


@gpu
@pytest.mark.parametrize("case", KERNEL_CASES, ids=lambda c: "V{}-T{}-J{}{}{}{}".format(c[0], c[1], c[2], "-n" if c[3] else "", "-t" if c[4] else "", "-neighbours" if c[5] else ""))
def test_kernel_equals_the_twin(halart, case):
    """read_vertices after set_deformer / update_deformer / refit equals the twin byte for byte, for three poses in a row (some weights
    exactly 0); the neighbours in the arena come back untouched"""
    nv, nt, nj, nrm, tan, neighbours = case
    scene = strip_scene(nv, neighbours, seed=nv)
    prim = 1 if neighbours else 0
    rest = scene.meshes[3].primitives[prim].vertices
    rig = D.random_rig(nv, targets=nt, joint_count=nj, normals=nrm, tangents=tan, seed=nv + nt + nj)
    r = SE.make(halart, cornell(), scene=scene)
    try:
        others = [(m, p) for m, mesh in enumerate(scene.meshes) for p in range(len(mesh.primitives)) if (m, p) != (3, prim)]
        for m, p in [(3, prim)] + others:
            assert r.read_vertices(m, p).tobytes() == scene.meshes[m].primitives[p].vertices.tobytes(), ("as uploaded", m, p)
        r.set_deformer(3, prim, **rig)
        r.refit()
        assert r.read_vertices(3, prim).tobytes() == rest.tobytes(), "a refit right after set_deformer changes nothing"
        for k in range(3):
            p = D.random_pose(rig, seed=k, zero_some=k > 0, centre=(10.0, 0.5, 0.0))
            if nj > 1 and k == 1:
                p["morph_weights"] = None  # keeps the weights of pose 0
            r.update_deformer(3, prim, **p)
            if p["morph_weights"] is None and nt:
                p["morph_weights"] = D.random_pose(rig, seed=0, zero_some=False)["morph_weights"]
            r.refit()
            want = D.pose_vertices(rest, rig, p)
            assert np.isfinite(want["position"]).all()
            got = r.read_vertices(3, prim)
            if got.tobytes() != want.tobytes():
                bad = np.nonzero(got.view(np.uint32).reshape(nv, 11) != want.view(np.uint32).reshape(nv, 11))
                raise AssertionError(f"{case} pose {k}: {len(bad[0])} words differ, first (vertex, word) {bad[0][:4]}, {bad[1][:4]}")
            assert want.tobytes() != rest.tobytes()
        for m, p in others:
            assert r.read_vertices(m, p).tobytes() == scene.meshes[m].primitives[p].vertices.tobytes(), ("neighbour", m, p)
    finally:
        r.close()


@gpu
@pytest.mark.parametrize("two_level", [False, True], ids=["one_level", "two_level"])
def test_render_equals_the_oracle_of_the_posed_scene(halart, oracle, two_level):
    """an accumulation under way, deformers on the tall block and on the short block's shared mesh, a pose, the refit: images 0-3 of
    update_batch(2) + update() equal the oracle's render of the scene that holds the twin's vertices, the tree passes the structural check,
    closest-hit and any-hit ray batches equal the oracle's.  Two-level: the shared mesh's one object-space tree is refitted"""
    base = cornell()
    poses = cornell_pose(1)
    edited = E.apply_to_scene(base.scene, posed_ops(poses))
    with SE.tree_form(oracle, two_level) as build:
        r = SE.make(halart, base, build=build)
        try:
            assert (r.bvh_info().instance_ref_count > 0) == two_level
            r.update_batch(2); r.render()
            register(r)
            pose(r, poses)
            r.refit()
            r.update_batch(2); r.update(); r.render()
            SE.assert_images(r, SE.oracle_images(oracle, base, edited, 3), f"two_level={two_level} after the refit")
            assert r.statistics().total_frames == 3
            osc = oracle.OracleScene(edited, envmap=base.env)
            assert SE.validate_tree(oracle, osc, r) == 0
            rays = SE.rays_of(osc, base)
            for mode in (0, 1):
                assert r.trace_rays_host(rays, mode).tobytes() == osc.trace(rays, mode).tobytes(), (two_level, mode)
            osc.close()
        finally:
            r.close()


@gpu
def test_same_bytes_as_update_vertices(halart):
    """a second renderer that is handed the twin's arrays through update_vertices + refit holds the same tree and renders the same images"""
    base = cornell()
    poses = cornell_pose(2)
    a = SE.make(halart, base)
    b = SE.make(halart, base)
    try:
        register(a)
        pose(a, poses)
        a.refit()
        E.apply_to_renderer(b, posed_ops(poses))
        b.refit()
        for x, y, what in zip(a.download_bvh(), b.download_bvh(), ("nodes", "triangles")):
            assert x.tobytes() == y.tobytes(), what
        a.update_batch(3); b.update_batch(3)
        for k in range(4):
            SE.assert_same(a.read_image(k), b.read_image(k), f"image {k}")
        for mesh in (TALL, SHORT):
            assert a.read_vertices(mesh, 0).tobytes() == b.read_vertices(mesh, 0).tobytes()
    finally:
        a.close(); b.close()


@gpu
@pytest.mark.parametrize("fusion", [1, 2])
def test_takes_effect_at_the_refit(halart, oracle, fusion):
    """between update_deformer and refit the frames continue the unedited accumulation (fusion 2: behind an open tail); the refit applies"""
    base = cornell()
    poses = cornell_pose(1)
    r = SE.make(halart, base)
    try:
        r.set_pass_fusion(fusion)
        r.update_batch(2)
        register(r)
        pose(r, poses)
        r.update(); r.update_batch(2); r.render()
        SE.assert_images(r, rest_images(oracle, 5), "before the refit")
        assert r.statistics().total_frames == 5
        for mesh in (TALL, SHORT):
            assert r.read_vertices(mesh, 0).tobytes() == base.scene.meshes[mesh].primitives[0].vertices.tobytes()
        r.update()
        r.refit()
        r.update_batch(2); r.update(); r.render()
        SE.assert_images(r, posed_images(oracle, 1, 3), "after the refit")
    finally:
        r.close()


@gpu
def test_three_poses_in_a_row_and_back_to_the_rest_pose(halart, oracle):
    """each pose equals the oracle (a kernel that deformed the previous pose instead of the rest pose would not); weights 0 and the identity
    palette give the original tree and frame back, and so does clear_deformer"""
    base = cornell()
    for mesh in (TALL, SHORT):
        v = base.scene.meshes[mesh].primitives[0].vertices
        # (x + 0 * y is x bit for bit unless x is -0.0.  Some normals are -0.0 and come back as +0.0: equal by value, no position is)
        assert not (np.signbit(v["position"]) & (v["position"] == 0.0)).any(), f"mesh {mesh} has a -0.0 coordinate"
    r = SE.make(halart, base)
    try:
        n0, t0 = r.download_bvh()
        register(r)
        for k in (1, 2, 3):
            pose(r, cornell_pose(k))
            r.refit()
            r.update_batch(3)
            SE.assert_images(r, posed_images(oracle, k, 3), f"pose {k}")
        rigs = cornell_rigs()
        r.update_deformer(TALL, 0, morph_weights=np.zeros(2, f32), joint_matrices=D.identity_palette(3))
        r.update_deformer(SHORT, 0, morph_weights=np.zeros(3, f32))
        assert rigs[SHORT]["joint_count"] == 0
        r.refit()
        r.update_batch(3)
        n1, t1 = r.download_bvh()
        assert n1.tobytes() == n0.tobytes() and t1.tobytes() == t0.tobytes(), "the tree at weights 0 and the identity palette"
        SE.assert_images(r, rest_images(oracle, 3), "weights 0 and the identity palette")
        pose(r, cornell_pose(2))
        r.refit()
        r.clear_deformer(TALL, 0); r.clear_deformer(SHORT, 0)
        r.refit()
        r.update_batch(3)
        n2, t2 = r.download_bvh()
        assert n2.tobytes() == n0.tobytes() and t2.tobytes() == t0.tobytes(), "the tree after clear_deformer"
        SE.assert_images(r, rest_images(oracle, 3), "after clear_deformer")
        for mesh in (TALL, SHORT):
            assert r.read_vertices(mesh, 0).tobytes() == base.scene.meshes[mesh].primitives[0].vertices.tobytes()
        r.update_vertices(TALL, 0, base.scene.meshes[TALL].primitives[0].vertices)  # accepted again
    finally:
        r.close()


@gpu
def test_refusals_change_nothing(halart, oracle):
    base = cornell()
    s = base.scene
    rigs = cornell_rigs()
    tall = rigs[TALL]
    nv = len(s.meshes[TALL].primitives[0].vertices)
    err = halart.HalaRendererError
    fresh = halart.HalaRenderer("deformers", base.kw["width"], base.kw["height"], 5, 3, False, False, False, 0)
    try:
        for prepare in (lambda: None, lambda: fresh.set_scene(s)):  # nothing set; set, not committed
            prepare()
            for call in (lambda: fresh.set_deformer(TALL, 0, **tall), lambda: fresh.update_deformer(TALL, 0, morph_weights=np.zeros(2, f32)),
                         lambda: fresh.clear_deformer(TALL, 0), lambda: fresh.read_vertices(TALL, 0)):
                with pytest.raises(err, match="none"):
                    call()
    finally:
        fresh.close()
    r = SE.make(halart, base)
    try:
        register(r)
        pose(r, cornell_pose(1))
        r.refit()
        r.update_batch(2)
        before = [r.read_image(k).tobytes() for k in range(4)]
        verts = {m: r.read_vertices(m, 0).tobytes() for m in (TALL, SHORT, 0)}

        def rig(**changes):
            return {**tall, **changes}

        bad_joint = tall["joints"].copy(); bad_joint[7, 2] = 3
        nan_delta = tall["targets"].copy(); nan_delta[1, 4, 0] = np.nan
        inf_normal = tall["normal_targets"].copy(); inf_normal[0, 0, 2] = np.inf
        nan_weight = tall["weights"].copy(); nan_weight[3, 1] = np.nan
        nan_matrix = D.identity_palette(3); nan_matrix[2, 1, 3] = np.nan
        big = np.zeros((65, nv, 3), f32)
        refusals = [
            (lambda: r.set_deformer(len(s.meshes), 0, **tall), "mesh"),
            (lambda: r.set_deformer(TALL, 1, **tall), "primitive"),
            (lambda: r.set_deformer(TALL, 0, targets=big), "more than 64"),
            (lambda: r.set_deformer(TALL, 0, **rig(targets=None, normal_targets=None, joint_count=257)), "more than 256"),
            (lambda: r.set_deformer(0, 0), "neither"),
            (lambda: r.set_deformer(TALL, 0, **rig(joints=bad_joint)), "joint index"),
            (lambda: r.set_deformer(TALL, 0, **rig(targets=nan_delta)), "finite"),
            (lambda: r.set_deformer(TALL, 0, **rig(normal_targets=inf_normal)), "finite"),
            (lambda: r.set_deformer(TALL, 0, **rig(weights=nan_weight)), "finite"),
            (lambda: r.update_deformer(len(s.meshes), 0, morph_weights=np.zeros(2, f32)), "mesh"),
            (lambda: r.update_deformer(TALL, 3, morph_weights=np.zeros(2, f32)), "primitive"),
            (lambda: r.update_deformer(0, 0, morph_weights=np.zeros(2, f32)), "no deformer"),
            (lambda: r.update_deformer(TALL, 0, morph_weights=np.zeros(3, f32)), "weight count"),
            (lambda: r.update_deformer(TALL, 0, joint_matrices=D.identity_palette(2)), "joint count"),
            (lambda: r.update_deformer(TALL, 0, morph_weights=np.array([0.0, np.inf], f32)), "finite"),
            (lambda: r.update_deformer(TALL, 0, joint_matrices=nan_matrix), "finite"),
            (lambda: r.update_deformer(TALL, 0, morph_weights=np.array([0.5, np.nan], f32), joint_matrices=D.identity_palette(3)), "finite"),
            (lambda: r.clear_deformer(0, 0), "no deformer"),
            (lambda: r.clear_deformer(TALL, 1), "primitive"),
            (lambda: r.update_vertices(TALL, 0, s.meshes[TALL].primitives[0].vertices), "clear it first"),
        ]
        for k, (call, word) in enumerate(refusals):
            with pytest.raises(err, match=word):
                call()
            assert {m: r.read_vertices(m, 0).tobytes() for m in (TALL, SHORT, 0)} == verts, f"refusal {k} ({word}) changed the vertices"
        r.refit()  # nothing is pending: none of the refused calls left anything behind

        def unchanged(what):
            r.reset_accumulation()
            r.update_batch(2)
            assert [r.read_image(k).tobytes() for k in range(4)] == before, what
            assert {m: r.read_vertices(m, 0).tobytes() for m in (TALL, SHORT, 0)} == verts, what

        unchanged("after the refusals")
        # overflow: finite matrix entries near 3e38 give a position that is not finite (plain IEEE overflow, found by the kernel)
        huge = D.identity_palette(3); huge[:, 0, 0] = 3.0e38; huge[:, 0, 1] = 3.0e38
        r.update_deformer(TALL, 0, joint_matrices=huge)
        r.update_deformer(SHORT, 0, morph_weights=cornell_pose(2)[SHORT]["morph_weights"])  # a valid edit in the same refit: stays pending
        with pytest.raises(err, match="Vertex position is not finite."):
            r.refit()
        unchanged("after the overflow")
        r.refit()  # the offending parameters are gone; the short block's pose was kept and applies now
        want = {TALL: cornell_pose(1)[TALL], SHORT: cornell_pose(2)[SHORT]}
        r.update_batch(2)
        SE.assert_images(r, SE.oracle_images(oracle, base, E.apply_to_scene(s, posed_ops(want)), 2), "the pending pose after the failed refit")
        pose(r, cornell_pose(3))  # a following valid pose works
        r.refit()
        r.update_batch(3)
        SE.assert_images(r, posed_images(oracle, 3, 3), "a valid pose after the overflow")
    finally:
        r.close()


@gpu
def test_lifetime_across_set_scene_and_commit(halart, oracle):
    """a repeated commit keeps the pose (it builds from the arena); a second set_deformer replaces the first and starts from the rest pose;
    set_scene drops the deformers"""
    base = cornell()
    r = SE.make(halart, base)
    try:
        register(r)
        pose(r, cornell_pose(1))
        r.refit()
        posed = {m: r.read_vertices(m, 0).tobytes() for m in (TALL, SHORT)}
        r.commit()
        assert {m: r.read_vertices(m, 0).tobytes() for m in (TALL, SHORT)} == posed
        r.update_batch(3)
        SE.assert_images(r, posed_images(oracle, 1, 3), "after a repeated commit")
        pose(r, cornell_pose(2))  # still registered
        r.refit()
        r.update_batch(3)
        SE.assert_images(r, posed_images(oracle, 2, 3), "a pose after the repeated commit")
        register(r)  # replaces both: back to the rest pose at the next refit
        r.refit()
        r.update_batch(3)
        SE.assert_images(r, rest_images(oracle, 3), "after replacing the deformers")
        pose(r, cornell_pose(3))
        r.refit()
        r.update_batch(3)
        SE.assert_images(r, posed_images(oracle, 3, 3), "a pose of the replacements")
        r.set_scene(base.scene)
        r.commit()
        with pytest.raises(halart.HalaRendererError, match="no deformer"):
            r.update_deformer(TALL, 0, morph_weights=np.zeros(2, f32))
        r.update_batch(3)
        SE.assert_images(r, rest_images(oracle, 3), "after set_scene")
    finally:
        r.close()


@gpu
@pytest.mark.parametrize("two_level", [False, True], ids=["one_level", "two_level"])
def test_posed_instances_start_without_temporal_history(halart, two_level):
    """set_temporal on, a capture, a pose change: temporal_resolve equals tests/temporal_ref.py with every instance of the deformed
    primitives marked — what the vertex edit E4 expects"""
    import test_temporal as TT
    base = cornell()
    poses = cornell_pose(1)
    r = TT.make(halart, base, build=dict(instancing=True) if two_level else dict(instancing=False))
    try:
        r.set_temporal()
        twin = TT.Twin(r, base.scene)
        register(r)
        r.update_batch(5)
        r.temporal_capture()
        twin.capture()
        pose(r, poses)
        twin.mark(posed_ops(poses))
        assert twin.im.sum() == 4  # the tall block's node and the three of the short block
        r.refit()
        r.update_batch(4)
        t, _ = TT.check_resolve(r, twin, f"two_level={two_level} after the pose")
        assert (t[..., 3] > 4).any(), "some pixels carry history"
        r.update()
        TT.check_resolve(r, twin, "one update later")
    finally:
        r.close()
