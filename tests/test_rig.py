"""Rigs and clips (docs/RENDER_SPEC.md 19; include/halart.h "The rig of a glTF file", "Rigs and clips") and the deformer kernel over many segments
(k_deform, csrc/deform.hip).

CPU tier: the loader's rig equals what tests/rig_ref.py wrote, array for array, and leaves the scene description alone;
hala_rig_sample_clip against the float64 twin; every malformed file is refused with its message; the loader and the evaluation under
AddressSanitizer and UBSan in a host-only program; header layouts against the ctypes mirrors.
GPU tier, every comparison by bytes: the batched kernel equals tests/deform_ref.py across wave and workgroup edges and mixed kinds, with
the launch and segment counts of one launch per refit; an overflow inside a batch changes nothing; glTF -> set_rig -> pose_rig -> refit
equals the oracle's render of the reported pose on both tree forms; key_rig equals keys set by hand; refusals change nothing."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import deform_normals_ref as N
import deform_ref as D
import rig_ref as R
import scene_edits as E
import test_gltf_native as GN
import test_scene_edits as SE
import hala_renderer_amd as H
from conftest import ROOT
from hala_renderer_amd import _abi as A
from hala_renderer_amd import scenes
from hala_renderer_amd.native_scene import NativeScene
from hala_renderer_amd.scene import HalaMesh, HalaNode, HalaPrimitive

gpu = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the good file, the same without its rig, and the malformed ones — written once"""
    d = tmp_path_factory.mktemp("rig")
    out = dict(good=R.save(R.character_doc(), d / "character.gltf"), plain=R.save(R.strip_rig(R.character_doc()), d / "plain.gltf"),
               singular=R.save(R.singular_doc(), d / "singular.gltf"), bad=[])
    for name, doc, words in R.malformed():
        out["bad"].append((name, R.save(doc, d / f"{name}.gltf"), words))
    return out


def clip_times(twin, clip):
    """before the first key, every key, three points inside every interval between keys, after the last key"""
    an = twin.doc["animations"][clip]
    keys = sorted({float(t) for s in an["samplers"] for t in twin.accessor(s["input"])[:, 0]})
    inside = [a + f * (b - a) for a, b in zip(keys[:-1], keys[1:]) for f in (0.25, 0.5, 0.8125)]
    return [keys[0] - 0.5] + keys + inside + [keys[-1] + 0.5]


# ---- CPU tier ---------------------------------------------------------------------------------------------------------------------------
def test_loader_returns_what_the_writer_put_in(files):
    truth = R.character()["truth"]
    doc = R.character_doc()
    twin = R.Twin(doc)
    nat = NativeScene(files["good"])
    rig = nat.rig
    scene_of = {name: twin.scene_of_gltf[g] for name, g in truth["gltf_index"].items()}
    # nodes: the breadth-first renumbering, and the TRS or the matrix flag
    assert rig.node_of_gltf == [twin.scene_of_gltf[g] for g in range(len(doc["nodes"]))]
    assert rig.node_of_gltf != list(range(len(doc["nodes"]))), "the walk renumbers this file"
    assert rig.node_count == nat.desc.node_count == twin.n
    for k, n in enumerate(rig.nodes):
        assert n["parent"] == twin.parent[k] == nat.desc.nodes[k].parent
        assert n["local_transform"].tobytes() == bytes(memoryview(nat.desc.nodes[k].local_transform))
        assert n["is_matrix"] == (twin.trs[k] is None)
        if twin.trs[k] is not None:
            for got, want in zip((n["translation"], n["rotation"], n["scale"]), twin.trs[k]):
                assert got.tobytes() == want.tobytes(), k
    for name, parent, t, q, s, mesh in R.RIG_NODES:
        n = rig.nodes[scene_of[name]]
        assert (list(n["translation"]), list(n["rotation"]), list(n["scale"])) == (list(t), list(q), list(s)), name
    # skins
    assert len(rig.skins) == 3
    for got, want in zip(rig.skins, truth["skins"]):
        assert got["joints"] == [scene_of[j] for j in want["joints"]]
        assert got["inverse_bind_matrices"].tobytes() == want["ibm"].tobytes()
    assert np.array_equal(rig.skins[2]["inverse_bind_matrices"], np.eye(4, dtype=f32).reshape(1, 16)), "absent: the identity"
    # bindings: two primitives under one skin (u8 and u16 joints; float and normalised u8 weights), skin + targets (normalised u16
    # weights, a sparse POSITION target, normal deltas), targets only (tangent deltas, one target without them, default weights)
    assert len(rig.bindings) == len(truth["bindings"]) == 4
    wf = pf = 0
    for got, want in zip(rig.bindings, truth["bindings"]):
        tables = want["rig"]
        assert (got["mesh_index"], got["primitive_index"], got["node"], got["node_count"], got["skin"]) == (want["mesh"], want["prim"], scene_of[want["node"]], 1, want["skin"])
        assert got["influence_sets"] == want["sets"]
        assert got["vertex_count"] == nat.desc.meshes[want["mesh"]].primitives[want["prim"]].vertex_count
        if want["skin"] is None:
            assert got["joints"] is None and got["weights"] is None and got["joint_count"] == 0
        else:
            assert got["joints"].dtype == np.uint16 and np.array_equal(got["joints"], tables["joints"])
            assert got["weights"].tobytes() == tables["weights"].tobytes()
            assert got["palette_first"] == pf
            pf += 12 * got["joint_count"]
        for key in ("targets", "normal_targets", "tangent_targets"):
            if tables[key] is None:
                assert got[key] is None, key
            else:
                assert got[key].tobytes() == np.ascontiguousarray(tables[key], dtype=f32).tobytes(), (want["mesh"], key)
        assert got["target_count"] == (0 if tables["targets"] is None else len(tables["targets"]))
        if got["target_count"]:
            assert got["default_weights"].tobytes() == want["default"].tobytes() and got["weight_first"] == wf
            wf += got["target_count"]
    assert (rig.weight_floats, rig.palette_floats) == (wf, pf) == (5, 12 * (3 + 3 + 2))
    sparse = truth["bindings"][2]["rig"]["targets"][1]
    assert 0 < np.count_nonzero(sparse.any(axis=1)) <= 7, "the sparse target is mostly zeros"
    # clips
    assert [c["name"] for c in rig.clips] == ["bend", "spline", ""]
    modes = {"STEP": A.RIG_STEP, "LINEAR": A.RIG_LINEAR, "CUBICSPLINE": A.RIG_CUBICSPLINE}
    seen = set()
    for got, want in zip(rig.clips, truth["clips"]):
        assert len(got["channels"]) == len(got["samplers"]) == len(want["channels"])
        for ch, sm, w in zip(got["channels"], got["samplers"], want["channels"]):
            assert (ch["node"], ch["path"], sm["interpolation"]) == (scene_of[w["node"]], R.PATHS[w["path"]], modes[w["interpolation"]])
            assert sm["times"].tobytes() == np.asarray(w["times"], dtype=f32).tobytes()
            assert sm["values"].tobytes() == np.ascontiguousarray(w["values"], dtype=f32).tobytes()
            width = {"translation": 3, "rotation": 4, "scale": 3}.get(w["path"]) or len([b for b in truth["bindings"] if b["node"] == w["node"]][0]["default"])
            assert sm["width"] == width
            seen.add((w["path"], w["interpolation"]))
        times = [t for w in want["channels"] for t in w["times"]]
        assert (got["time_first"], got["time_last"]) == (f32(min(times)), f32(max(times)))
    assert {p for p, _ in seen} == set(R.PATHS) and {m for _, m in seen} == set(modes)
    # the scene description: as without the rig, and as the Python mirror reads it
    plain = NativeScene(files["plain"])
    GN.assert_same_desc(nat.desc, plain.desc)
    assert plain.rig.node_count == 0 and not plain.rig.bindings and not plain.rig.clips and not plain.rig.skins and not plain.rig.node_of_gltf
    mirror = H.HalaScene.new(files["good"]).to_desc()
    GN.assert_same_desc(nat.desc, mirror.desc)
    plain.close(); nat.close()


def test_sample_clip_agrees_with_the_float64_twin(files):
    """Both sides compute in float64, where the accumulated error is about 1e-14 of the largest term, and round once: a matrix or a
    vector differs by at most one float32 ulp at the magnitude of its largest entry.  Nodes the clip does not touch compare by bytes."""
    twin = R.Twin(R.character_doc())
    nat = NativeScene(files["good"])
    rig = nat.rig
    worst = 0
    for clip in (None, 0, 1, 2):
        for t in ([0.0] if clip is None else clip_times(twin, clip)):
            got, want = H.sample_clip(rig, clip, t), twin.sample(clip, t)
            for k in range(twin.n):
                if want["touched"][k] and clip is not None:
                    assert R.within_one_ulp(got["locals"][k], want["locals"][k]), (clip, t, "node", k)
                else:
                    assert got["locals"][k].tobytes() == want["locals"][k].tobytes(), (clip, t, "untouched node", k)
            for b in range(len(rig.bindings)):
                for key in ("weights", "palettes"):
                    if want[key][b] is None:
                        assert got[key][b] is None
                    else:
                        assert R.within_one_ulp(got[key][b], want[key][b]), (clip, t, key, b)
                        worst = max(worst, int((got[key][b] != want[key][b]).sum()))
            if clip is not None:
                assert want["touched"].any() and any(not np.array_equal(p, D.identity_palette(len(p))) for p in want["palettes"] if p is not None)
    print("entries that differ by one ulp, at most, in one array:", worst)
    # the file's own pose: identity palettes bit for bit (the bind pose is exact), default weights
    own = H.sample_clip(rig, None, 0.0)
    for b, p in zip(rig.bindings, own["palettes"]):
        if p is not None:
            assert np.array_equal(p, D.identity_palette(b["joint_count"]))
    assert [None if w is None else w.tolist() for w in own["weights"]] == [None, None, [0.0, 0.0], [0.25, 0.0, -0.5]]
    for call, word in ((lambda: H.sample_clip(rig, 3, 0.0), "clip does not exist"), (lambda: H.sample_clip(rig, 0, float("nan")), "not finite")):
        with pytest.raises(H.HalaRendererError, match=word):
            call()
    nat.close()
    # a clip that squashes a bound mesh node flat: posed while the scale stands, refused from the key that zeroes it
    flat = NativeScene(files["singular"])
    stw = R.Twin(R.singular_doc())
    got, want = H.sample_clip(flat.rig, 3, 0.5), stw.sample(3, 0.5)
    for key in ("weights", "palettes"):
        assert all((g is None and w is None) or R.within_one_ulp(g, w) for g, w in zip(got[key], want[key])), key
    for t in (1.0, 1.5):
        with pytest.raises(H.HalaRendererError, match="world transform of the node of mesh 3 is singular"):
            H.sample_clip(flat.rig, 3, t)
    again = H.sample_clip(flat.rig, 3, 0.5)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got["palettes"][:3], again["palettes"][:3])), "a refused sample leaves nothing behind"
    flat.close()


def test_malformed_rigs_are_refused_with_their_message(files):
    assert len(files["bad"]) == 13
    for name, path, words in files["bad"]:
        with pytest.raises(H.HalaRendererError) as e:
            NativeScene(path)
        assert "glTF rig" in str(e.value) and words in str(e.value), (name, str(e.value))


def test_loader_and_sampling_under_host_sanitizers(files, tmp_path):
    """tests/rig_host_check.c with the library's host sources, built with -fsanitize=address,undefined, run as its own process on the good
    file and on every malformed one"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    cc = shutil.which("gcc") or shutil.which("clang")
    assert cxx and cc, "no host compiler"
    csrc = os.path.join(ROOT, "hala-renderer_amd", "csrc")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    flags = ["-g1", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    inc = ["-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", os.path.join(ROOT, "include"), "-I", csrc]
    sources = [os.path.join(csrc, f) for f in ("gltf_loader.cpp", "rig.cpp", "host_util.cpp", "jpeg_decode.cpp")] + [os.path.join(ROOT, "tests", "rig_host_shim.cpp")]
    objs = [str(tmp_path / (os.path.basename(src) + ".o")) for src in sources] + [str(tmp_path / "main.o")]
    jobs = [subprocess.Popen([cxx, "-std=c++17", *flags, *inc, "-c", src, "-o", obj], stderr=subprocess.PIPE, text=True) for src, obj in zip(sources, objs)]
    jobs.append(subprocess.Popen([cc, "-std=c99", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "tests", "rig_host_check.c"),
                                  "-o", objs[-1]], stderr=subprocess.PIPE, text=True))
    for job in jobs:  # (the units compile side by side)
        _, err = job.communicate()
        assert job.returncode == 0, err[-3000:]
    exe = str(tmp_path / "rig_host_check")
    # (the runtimes linked into the program itself: clang's default; for gcc it has to be asked for)
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx).startswith("g++") else []
    subprocess.run([cxx, *flags, *static, *objs, "-lz", "-ldl", "-o", exe], check=True, capture_output=True, text=True)
    paths = [files["good"], files["plain"], files["singular"]] + [p for _, p, _ in files["bad"]]
    run = subprocess.run([exe, *paths], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-3000:]
    lines = run.stdout.splitlines()
    assert len(lines) == len(paths)
    assert lines[0].startswith("loaded") and " 4 bindings 3 clips 63 samples 0 failed" in lines[0], lines[0]
    assert lines[1].startswith("loaded") and " 0 nodes 0 skins 0 bindings 0 clips 0 samples 0 failed" in lines[1], lines[1]
    assert lines[2].startswith("loaded") and " 4 bindings 4 clips 84 samples 3 failed" in lines[2], lines[2]  # the squashed mesh node from time 1 on
    for line, (name, _, words) in zip(lines[3:], files["bad"]):
        assert line.startswith("refused") and words in line, (name, line)


RIG_STRUCTS = [("hala_rig_node", A.RigNode, 112), ("hala_rig_skin", A.RigSkin, 24), ("hala_rig_binding", A.RigBinding, 88), ("hala_rig_sampler", A.RigSampler, 32),
               ("hala_rig_channel", A.RigChannel, 16), ("hala_rig_clip", A.RigClip, 40), ("hala_rig_desc", A.RigDesc, 72), ("hala_rig_status", A.RigStatus, 32)]


def test_rig_layouts_match_the_header(tmp_path):
    src = tmp_path / "layout.c"
    body = ""
    for name, mirror, _ in RIG_STRUCTS:
        body += f'  printf("%zu", sizeof({name}));\n' + "".join(f'  printf(" %zu", offsetof({name}, {n}));\n' for n, _ in mirror._fields_) + '  printf("\\n");\n'
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "halart.h"\nint main(void) {\n' + body +
                   '  printf("%u %u %u %u %u %u %u\\n", HALA_RIG_STEP, HALA_RIG_LINEAR, HALA_RIG_CUBICSPLINE, HALA_RIG_TRANSLATION, HALA_RIG_ROTATION, HALA_RIG_SCALE, HALA_RIG_WEIGHTS);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    for line, (name, mirror, size) in zip(lines, RIG_STRUCTS):
        out = [int(x) for x in line.split()]
        assert out[0] == C.sizeof(mirror) == size, name
        assert out[1:] == [getattr(mirror, n).offset for n, _ in mirror._fields_], name
    assert [int(x) for x in lines[-1].split()] == [A.RIG_STEP, A.RIG_LINEAR, A.RIG_CUBICSPLINE, A.RIG_TRANSLATION, A.RIG_ROTATION, A.RIG_SCALE, A.RIG_WEIGHTS]
    for fn in ("hala_scene_get_rig", "hala_rig_sample_clip", "hala_rt_set_rig", "hala_rt_pose_rig", "hala_rt_key_rig", "hala_rt_get_rig_pose", "hala_rt_get_rig_status"):
        assert fn in A.EXPORTS and fn in A.PROTOTYPES, fn


# ---- GPU tier: the batched kernel -----------------------------------------------------------------------------------------------------------
# (vertices, targets, joints, normal deltas, tangent deltas, all weights 0): the wave edge (63, 64, 65), the workgroup edge (255, 256,
# 257), more than one workgroup (257, 513); no active target, 1 and 64 targets with and without normal / tangent deltas, no skin, 1 and
# 256 joints, targets and a skin
BATCH = [(1, 2, 1, False, False, True), (63, 1, 0, True, False, False), (64, 64, 0, False, True, False), (65, 0, 1, False, False, False),
         (255, 0, 256, False, False, False), (256, 1, 256, True, True, False), (257, 64, 4, True, False, False), (513, 3, 2, False, False, False)]
BATCH_MESH = 3


def batch_scene():
    s = scenes.cornell_box(aspect=E.W / E.H_)
    prims = [HalaPrimitive(*D.strip(c[0], seed=c[0], origin=(0.0, 3.0 * k, 0.0)), material_index=k % 5) for k, c in enumerate(BATCH)]
    s.meshes = list(s.meshes) + [HalaMesh(prims)]
    s.nodes = list(s.nodes) + [HalaNode(name="strips", mesh_index=BATCH_MESH, local_transform=E._translate((20.0, 200.0, 150.0)))]
    return s


_BATCH_RIGS = []


def batch_rigs():
    if not _BATCH_RIGS:
        _BATCH_RIGS.extend(D.random_rig(c[0], targets=c[1], joint_count=c[2], normals=c[3], tangents=c[4], seed=sum(c[:3])) for c in BATCH)
    return _BATCH_RIGS


def batch_pose(k, seed):
    p = D.random_pose(batch_rigs()[k], seed=seed, zero_some=seed > 0, centre=(10.0, 0.5, 0.0))
    if BATCH[k][5]:
        p["morph_weights"] = np.zeros(BATCH[k][1], dtype=f32)
    return p


def counts(r):
    s = r.rig_status()
    return s.pose_launches, s.segments_posed, s.batch_launches


def assert_posed(r, scene, poses, what):
    """every primitive of the strip mesh holds the twin's vertices for its pose (None: the rest pose), byte for byte"""
    for k, p in enumerate(poses):
        rest = scene.meshes[BATCH_MESH].primitives[k].vertices
        want = rest if p is None else D.pose_vertices(rest, batch_rigs()[k], p)
        got = r.read_vertices(BATCH_MESH, k)
        if got.tobytes() != want.tobytes():
            bad = np.nonzero(got.view(np.uint32).reshape(-1, 11) != want.view(np.uint32).reshape(-1, 11))
            raise AssertionError(f"{what}: primitive {k} {BATCH[k]}: {len(bad[0])} words differ, first (vertex, word) {bad[0][:4]}, {bad[1][:4]}")


@gpu
def test_batched_kernel_equals_the_twin(halart):
    """eight deformers of mixed kinds registered, all posed, one refit: one launch, eight segments, the twin's bytes — three poses in a
    row; then exactly two dirty deformers (the smallest batch: a launch counted in batch_launches) and exactly one (a launch that is not)"""
    scene = batch_scene()
    r = SE.make(halart, SE.base_of("cornell"), scene=scene)
    try:
        for k, rig in enumerate(batch_rigs()):
            r.set_deformer(BATCH_MESH, k, **rig)
        assert r.rig_status().deformers == 8 and r.rig_status().bindings == 0
        before = counts(r)
        r.refit()
        assert counts(r) == before, "nothing is dirty"
        poses = [None] * 8
        for seed in range(3):
            poses = [batch_pose(k, seed) for k in range(8)]
            for k, p in enumerate(poses):
                r.update_deformer(BATCH_MESH, k, **p)
            r.refit()
            after = counts(r)
            assert tuple(a - b for a, b in zip(after, before)) == (1, 8, 1), f"pose {seed}: launches, segments, batch launches {before} -> {after}"
            before = after
            assert_posed(r, scene, poses, f"pose {seed}")
        assert any(D.pose_vertices(scene.meshes[BATCH_MESH].primitives[k].vertices, batch_rigs()[k], poses[k]).tobytes() !=
                   scene.meshes[BATCH_MESH].primitives[k].vertices.tobytes() for k in range(8))
        for m in range(3):  # the primitives without deformers
            assert r.read_vertices(m, 0).tobytes() == scene.meshes[m].primitives[0].vertices.tobytes(), m
        for dirty in ((2, 6), (5,)):
            for k in dirty:
                poses[k] = batch_pose(k, 7 + len(dirty))
                r.update_deformer(BATCH_MESH, k, **poses[k])
            r.refit()
            after = counts(r)
            assert tuple(a - b for a, b in zip(after, before)) == (1, len(dirty), 1 if len(dirty) > 1 else 0), (dirty, before, after)
            before = after
            assert_posed(r, scene, poses, f"dirty {dirty}")
    finally:
        r.close()


# (vertices, targets, joints, normal deltas, normals mode): the staged sections of one launch as unequal as they can be — the largest
# active list and palette beside a deformer that has neither, the middle one no segment of the normals passes, the last with two of
# its three weights exactly 0 and more than one workgroup
UNEQUAL = [(65, 64, 256, True, 1), (1, 0, 1, False, 0), (257, 3, 0, False, 1)]


@gpu
def test_unequal_staged_sections_equal_the_twins(halart):
    """three deformers whose tables, active targets and palettes differ as far as the limits allow, posed by one refit: every primitive
    the twins' bytes (tests/deform_ref.py, then tests/deform_normals_ref.py where the mode is 1), one pose launch of three segments, two
    normals launches; then the middle one alone: one launch of one segment, no normals launch, the same bytes everywhere"""
    prims = [D.strip(c[0], seed=c[0], origin=(0.0, 3.0 * k, 0.0)) for k, c in enumerate(UNEQUAL)]
    s = scenes.cornell_box(aspect=E.W / E.H_)
    s.meshes = list(s.meshes) + [HalaMesh([HalaPrimitive(idx, v, material_index=k % 5) for k, (idx, v) in enumerate(prims)])]
    s.nodes = list(s.nodes) + [HalaNode(name="strips", mesh_index=BATCH_MESH, local_transform=E._translate((20.0, 200.0, 150.0)))]
    rigs = [D.random_rig(c[0], targets=c[1], joint_count=c[2], normals=c[3], seed=40 + k) for k, c in enumerate(UNEQUAL)]
    poses = [D.random_pose(rig, seed=50 + k, zero_some=False, centre=(10.0, 0.5, 0.0)) for k, rig in enumerate(rigs)]
    poses[2]["morph_weights"][[0, 2]] = 0.0
    assert np.count_nonzero(poses[0]["morph_weights"]) == 64 and np.count_nonzero(poses[2]["morph_weights"]) == 1
    want = []
    for (idx, rest), rig, p, c in zip(prims, rigs, poses, UNEQUAL):
        v = D.pose_vertices(rest, rig, p)
        assert np.isfinite(v["position"]).all() and v.tobytes() != rest.tobytes()
        want.append(N.recompute(v, idx, N.classes(rest, idx)) if c[4] else v)
    assert want[2]["normal"].tobytes() != D.pose_vertices(prims[2][1], rigs[2], poses[2])["normal"].tobytes(), "the case exercises the passes"
    r = SE.make(halart, SE.base_of("cornell"), scene=s)

    def assert_all(what):
        for k in range(3):
            got = r.read_vertices(BATCH_MESH, k)
            if got.tobytes() != want[k].tobytes():
                bad = np.nonzero(got.view(np.uint32).reshape(-1, 11) != want[k].view(np.uint32).reshape(-1, 11))
                raise AssertionError(f"{what}: primitive {k} {UNEQUAL[k]}: {len(bad[0])} words differ, first (vertex, word) {bad[0][:4]}, {bad[1][:4]}")
        for m in range(3):  # the primitives without deformers
            assert r.read_vertices(m, 0).tobytes() == s.meshes[m].primitives[0].vertices.tobytes(), (what, m)

    try:
        for k, rig in enumerate(rigs):
            r.set_deformer(BATCH_MESH, k, **rig)
            r.set_deformer_normals(BATCH_MESH, k, UNEQUAL[k][4])
        r.refit()  # (the mode switches made 0 and 2 dirty: posed at the identity pose)
        before, normals_before = counts(r), r.get_deformer_normals(BATCH_MESH, 0).launches
        for k, p in enumerate(poses):
            r.update_deformer(BATCH_MESH, k, **p)
        r.refit()
        after, normals_after = counts(r), r.get_deformer_normals(BATCH_MESH, 0).launches
        assert tuple(a - b for a, b in zip(after, before)) == (1, 3, 1) and normals_after - normals_before == 2, (before, after, normals_before, normals_after)
        assert_all("three at once")
        r.update_deformer(BATCH_MESH, 1, **poses[1])
        r.refit()
        assert tuple(a - b for a, b in zip(counts(r), after)) == (1, 1, 0) and r.get_deformer_normals(BATCH_MESH, 0).launches == normals_after
        assert_all("the second alone")
    finally:
        r.close()


@gpu
def test_overflow_inside_a_batch_changes_nothing(halart):
    """one segment of eight is driven to a non-finite position by a large finite weight: the refit fails, every primitive and the tree
    are what they were, the offender falls back and the others stay pending for the next refit"""
    scene = batch_scene()
    r = SE.make(halart, SE.base_of("cornell"), scene=scene)
    try:
        for k, rig in enumerate(batch_rigs()):
            r.set_deformer(BATCH_MESH, k, **rig)
        first = [batch_pose(k, 1) for k in range(8)]
        for k, p in enumerate(first):
            r.update_deformer(BATCH_MESH, k, **p)
        r.refit()
        assert_posed(r, scene, first, "the first pose")
        nodes, tris = r.download_bvh()
        second = [batch_pose(k, 2) for k in range(8)]
        offender = 6
        huge = second[offender]["morph_weights"].copy(); huge[:] = 3.0e38
        for k, p in enumerate(second):
            r.update_deformer(BATCH_MESH, k, **({**p, "morph_weights": huge} if k == offender else p))
        with pytest.raises(halart.HalaRendererError, match="Vertex position is not finite."):
            r.refit()
        assert_posed(r, scene, first, "after the failed refit")
        n2, t2 = r.download_bvh()
        assert n2.tobytes() == nodes.tobytes() and t2.tobytes() == tris.tobytes(), "the tree after the failed refit"
        for m in range(3):
            assert r.read_vertices(m, 0).tobytes() == scene.meshes[m].primitives[0].vertices.tobytes(), m
        before = counts(r)
        r.refit()  # the others were kept and apply now; the offender stands at its last applied pose
        after = counts(r)
        assert (after[0] - before[0], after[1] - before[1]) == (1, 7)
        assert_posed(r, scene, [first[k] if k == offender else second[k] for k in range(8)], "the refit after the failed one")
    finally:
        r.close()


# ---- GPU tier: the rig ------------------------------------------------------------------------------------------------------------------------
def tables_of(binding):
    return {k: binding[k] for k in ("targets", "normal_targets", "tangent_targets", "joints", "weights", "joint_count")}


def posed_ops(py_scene, rig, pose):
    """the operations of tests/scene_edits.py that carry a reported pose: every node's local transform, and the twin of RENDER_SPEC 17
    applied to every binding with the pose's weights and palettes"""
    ops = [("node", k, pose["locals"][k]) for k in range(len(py_scene.nodes))]
    for b, w, p in zip(rig.bindings, pose["weights"], pose["palettes"]):
        rest = py_scene.meshes[b["mesh_index"]].primitives[b["primitive_index"]].vertices
        ops.append(("vertices", b["mesh_index"], b["primitive_index"], D.pose_vertices(rest, tables_of(b), dict(morph_weights=w, joint_matrices=p))))
    return ops


def touched_nodes(rig, clip):
    return sorted({ch["node"] for ch in rig.clips[clip]["channels"] if ch["path"] != A.RIG_WEIGHTS})


@gpu
@pytest.mark.parametrize("two_level", [False, True], ids=["one_level", "two_level"])
def test_file_to_frame_equals_the_oracle_of_the_reported_pose(halart, oracle, files, two_level):
    """NativeScene -> set_scene -> commit -> set_rig -> pose_rig at two times -> refit: images 0-3 of three frames, the tree and two ray
    batches equal the oracle's of the scene that holds the reported locals and tests/deform_ref.py's vertices; the file's own pose brings
    the loaded vertices back.  (Byte for byte where the file's weights sum to 1 exactly and the mesh has no default weights — the float
    and the one-hot u16 primitives; 64 / 255 weights and default morph weights pose away from the loaded bytes by definition, and
    those primitives equal the twin's pose.)"""
    base = SE.base_of("cornell")
    nat = NativeScene(files["good"])
    py = H.HalaScene.new(files["good"])
    rig = nat.rig
    with SE.tree_form(oracle, two_level) as build:
        r = SE.make(halart, base, scene=nat, build=build)
        try:
            r.set_rig(rig)
            st = r.rig_status()
            assert (st.bindings, st.deformers) == (4, 4)
            before = counts(r)
            for clip, t in ((0, 0.625), (1, 1.75)):
                r.pose_rig(clip, t)
                r.refit()
                pose = r.rig_pose()
                assert (pose["clip"], pose["time"]) == (clip, t)
                want = H.sample_clip(rig, clip, t)
                assert pose["locals"].tobytes() == want["locals"].tobytes()
                ops = posed_ops(py, rig, pose)
                for op in ops[len(py.nodes):]:
                    assert r.read_vertices(op[1], op[2]).tobytes() == op[3].tobytes(), (clip, op[1], op[2])
                    assert op[3].tobytes() != py.meshes[op[1]].primitives[op[2]].vertices.tobytes()
                edited = E.apply_to_scene(py, ops)
                r.update_batch(2); r.update(); r.render()
                SE.assert_images(r, SE.oracle_images(oracle, base, edited, 3), f"two_level={two_level} clip {clip} at {t}")
            after = counts(r)
            assert (after[0] - before[0], after[1] - before[1]) == (2, 8), "one launch per refit for the four bindings"
            osc = oracle.OracleScene(edited, envmap=base.env)
            assert SE.validate_tree(oracle, osc, r) == 0
            rays = SE.rays_of(osc, base)
            for mode in (0, 1):
                assert r.trace_rays_host(rays, mode).tobytes() == osc.trace(rays, mode).tobytes(), (two_level, mode)
            osc.close()
            r.pose_rig(None, 0.0)
            r.refit()
            own = r.rig_pose()
            assert own["clip"] is None
            for k, op in enumerate(posed_ops(py, rig, own)[len(py.nodes):]):
                assert r.read_vertices(op[1], op[2]).tobytes() == op[3].tobytes(), ("the file's own pose", op[1], op[2])
                if k in (0, 2):
                    assert op[3].tobytes() == py.meshes[op[1]].primitives[op[2]].vertices.tobytes(), ("the loaded vertices", op[1], op[2])
            r.update_batch(2); r.update(); r.render()
            SE.assert_images(r, SE.oracle_images(oracle, base, E.apply_to_scene(py, posed_ops(py, rig, own)), 3), "the file's own pose")
        finally:
            r.close()
    nat.close()


@gpu
def test_key_rig_equals_keys_set_by_hand(halart, files):
    """key_rig + set_shutter + refit + 4 updates against a second renderer whose node and deformer keys the test sets from rig_pose"""
    base = SE.base_of("cornell")
    nat = NativeScene(files["good"])
    rig = nat.rig
    a = SE.make(halart, base, scene=nat)
    b = SE.make(halart, base, scene=nat)
    try:
        a.set_rig(rig)
        a.key_rig(0, 0.375, 1.125)
        a.set_shutter(0.0, 1.0, 1)
        a.refit()
        opened, closed = a.rig_pose(0), a.rig_pose(1)
        assert (opened["time"], closed["time"]) == (0.375, 1.125) and opened["locals"].tobytes() != closed["locals"].tobytes()
        for bd in rig.bindings:
            b.set_deformer(bd["mesh_index"], bd["primitive_index"], **tables_of(bd))
        for n in touched_nodes(rig, 0):
            b.set_node_keys(n, opened["locals"][n], closed["locals"][n])
        for k, bd in enumerate(rig.bindings):
            b.set_deformer_keys(bd["mesh_index"], bd["primitive_index"], dict(morph_weights=opened["weights"][k], joint_matrices=opened["palettes"][k]),
                                dict(morph_weights=closed["weights"][k], joint_matrices=closed["palettes"][k]))
        b.set_shutter(0.0, 1.0, 1)
        b.refit()
        for r in (a, b):
            for _ in range(4):
                r.update()
            r.render()
        assert a.shutter_status().steps == b.shutter_status().steps > 0
        for k in range(4):
            SE.assert_same(a.read_image(k), b.read_image(k), f"image {k}")
        for x, y, what in zip(a.download_bvh(), b.download_bvh(), ("nodes", "triangles")):
            assert x.tobytes() == y.tobytes(), what
        for bd in rig.bindings:
            assert a.read_vertices(bd["mesh_index"], bd["primitive_index"]).tobytes() == b.read_vertices(bd["mesh_index"], bd["primitive_index"]).tobytes()
        with pytest.raises(halart.HalaRendererError, match="shutter keys"):
            a.pose_rig(0, 0.5)  # a keyed holder refuses the plain edit
        a.key_rig(None)
        a.pose_rig(0, 0.5)
        a.refit()
    finally:
        a.close(); b.close()
    nat.close()


def _copy_desc(rig):
    """a shallow ctypes copy of a rig's description and of its binding and skin tables, free to be changed"""
    d = A.RigDesc.from_buffer_copy(rig.desc)
    bindings = (A.RigBinding * d.binding_count)(*[A.RigBinding.from_buffer_copy(rig.desc.bindings[k]) for k in range(d.binding_count)])
    skins = (A.RigSkin * d.skin_count)(*[A.RigSkin.from_buffer_copy(rig.desc.skins[k]) for k in range(d.skin_count)])
    d.bindings, d.skins = C.cast(bindings, C.POINTER(A.RigBinding)), C.cast(skins, C.POINTER(A.RigSkin))
    keep = [bindings, skins, rig]

    class Changed:
        desc = d

        def desc_ptr(self):
            return C.pointer(d)
    c = Changed()
    c.keep, c.bindings, c.skins = keep, bindings, skins
    return c


@gpu
def test_rig_refusals_change_nothing(halart, files, tmp_path):
    base = SE.base_of("cornell")
    err = halart.HalaRendererError
    nat = NativeScene(files["singular"])  # the character, and clip 3 that squashes a mesh node
    rig = nat.rig
    r = SE.make(halart, base, scene=nat)
    ref = SE.make(halart, base, scene=nat)
    plain = SE.make(halart, base)
    try:
        ref.update_batch(2)
        want = [ref.read_image(k).tobytes() for k in range(4)]
        verts = {(b["mesh_index"], b["primitive_index"]): r.read_vertices(b["mesh_index"], b["primitive_index"]).tobytes() for b in rig.bindings}
        for call in (lambda: r.pose_rig(0, 0.0), lambda: r.key_rig(0, 0.0, 1.0), lambda: r.rig_pose()):
            with pytest.raises(err, match="No rig is set"):
                call()
        # (descriptions that are sound but for the limit: the packed pose has room, and no clip reads the widened tables)
        many_targets = _copy_desc(rig); many_targets.bindings[2].target_count = 65
        many_targets.desc.weight_floats, many_targets.desc.clip_count = 80, 0
        many_joints = _copy_desc(rig)
        joints = (C.c_uint32 * 257)(*([rig.skins[0]["joints"][0]] * 257))
        ibm = (C.c_float * (257 * 16))(*(np.tile(np.eye(4, dtype=f32).reshape(16), 257).tolist()))
        many_joints.skins[1].joint_count, many_joints.skins[1].joints, many_joints.skins[1].inverse_bind_matrices = 257, joints, ibm
        many_joints.desc.palette_floats, many_joints.desc.clip_count = rig.palette_floats + 12 * 255, 0
        two_nodes = R.character_doc()
        two_nodes["nodes"].append({"name": "again", "mesh": R.BODY, "translation": [5.0, 5.0, 5.0]})
        two_nodes["scenes"][0]["nodes"].append(len(two_nodes["nodes"]) - 1)
        twice = NativeScene(R.save(two_nodes, tmp_path / "twice.gltf"))
        r2 = SE.make(halart, base, scene=twice)
        try:
            with pytest.raises(err, match="Mesh 3 is instantiated by 2 nodes.*mesh 3 primitive 0"):
                r2.set_rig(twice.rig)
            assert r2.rig_status().deformers == 0
        finally:
            r2.close(); twice.close()
        with pytest.raises(err, match="nodes and the committed scene"):
            plain.set_rig(rig)  # indices outside the committed scene
        tables = tables_of(rig.bindings[2])
        rest = r.read_vertices(R.MORPH, 0)
        refusals = [(lambda: r.set_rig(many_targets), "mesh 4 primitive 0 has more than 64 morph targets"),
                    (lambda: r.set_rig(many_joints), "mesh 4 primitive 0 has more than 256 joints")]
        for call, words in refusals:
            with pytest.raises(err, match=words):
                call()
            assert r.rig_status().deformers == 0
        r.set_deformer(R.BOTH, 0, **tables)
        with pytest.raises(err, match=r"already has a deformer \(mesh 4 primitive 0\)"):
            r.set_rig(rig)
        assert r.rig_status().deformers == 1
        r.clear_deformer(R.BOTH, 0)
        r.set_vertex_keys(R.MORPH, 0, rest, rest)
        with pytest.raises(err, match=r"shutter vertex keys \(mesh 5 primitive 0\)"):
            r.set_rig(rig)
        r.set_vertex_keys(R.MORPH, 0, None, None)
        r.refit()
        assert r.rig_status().deformers == 0 and r.rig_status().bindings == 0
        r.set_rig(rig)
        with pytest.raises(err, match="A rig is set"):
            r.set_rig(rig)
        for call, words in ((lambda: r.pose_rig(4, 0.0), "clip does not exist"), (lambda: r.pose_rig(0, float("inf")), "not finite"),
                            (lambda: r.key_rig(7, 0.0, 1.0), "clip does not exist"), (lambda: r.key_rig(1, 0.0, float("nan")), "not finite"),
                            (lambda: r.pose_rig(3, 1.5), "world transform of the node of mesh 3 is singular"),
                            (lambda: r.key_rig(3, 0.0, 1.0), "world transform of the node of mesh 3 is singular"),
                            (lambda: r.rig_pose(), "No pose has been recorded")):
            with pytest.raises(err, match=words):
                call()
        # keyed holders refuse the plain edit of a pose: a node the clip touches, a binding's deformer (keys that move nothing)
        node = touched_nodes(rig, 0)[0]
        loaded = rig.nodes[node]["local_transform"].reshape(4, 4).T
        r.set_node_keys(node, loaded, loaded)
        with pytest.raises(err, match="The node has shutter keys"):
            r.pose_rig(0, 0.5)
        r.set_node_keys(node)
        still = dict(morph_weights=np.zeros(3, f32))
        r.set_deformer_keys(R.MORPH, 0, still, still)
        with pytest.raises(err, match="The deformer has shutter keys"):
            r.pose_rig(0, 0.5)
        r.set_deformer_keys(R.MORPH, 0)
        # a deformer the host put in the rig's place is the host's: no pose goes to it, and clearing the rig leaves it
        r.clear_deformer(R.BOTH, 0)
        r.set_deformer(R.BOTH, 0, **tables)
        with pytest.raises(err, match=r"no longer has the deformer the rig registered \(mesh 4 primitive 0\)"):
            r.pose_rig(0, 0.5)
        r.refit()  # nothing but the cleared keys is pending: the refused calls left nothing behind
        assert {k: r.read_vertices(*k).tobytes() for k in verts} == verts
        r.reset_accumulation()
        r.update_batch(2)
        assert [r.read_image(k).tobytes() for k in range(4)] == want, "after the refused poses"
        r.set_rig(None)
        assert r.rig_status().deformers == 1 and r.rig_status().bindings == 0
        r.clear_deformer(R.BOTH, 0)
        # a pose that is accepted, then the rig cleared: vertices and nodes are the file's again
        r.set_rig(rig)
        r.pose_rig(0, 0.5)
        r.refit()
        assert {k: r.read_vertices(*k).tobytes() for k in verts} != verts
        r.set_rig(None)
        assert r.rig_status().deformers == 0
        r.refit()
        r.reset_accumulation()
        r.update_batch(2)
        assert [r.read_image(k).tobytes() for k in range(4)] == want, "after the refusals"
        assert {k: r.read_vertices(*k).tobytes() for k in verts} == verts
    finally:
        r.close(); ref.close(); plain.close()
    nat.close()
