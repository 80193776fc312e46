"""Rigs and clips (docs/RENDER_SPEC.md 19), the test side.  Two jobs:

1. character_doc() writes a rigged glTF document: the Cornell box plus strip primitives (tests/deform_ref.strip) under skins, with morph
   targets and three animation clips, its nodes listed in an order the loader's breadth-first walk has to renumber.  malformed() lists
   the documents the loader must refuse; strip_rig() takes skins, targets and animations out again.
2. Twin is a numpy-float64 evaluation of RENDER_SPEC 19 that reads the glTF JSON itself (its own accessor reader, its own renumbering)
   and shares nothing with the library's arrays.

The bind pose uses transforms that are exact in binary arithmetic — rotations by 120 degrees about (1, 1, 1) (the quaternion of four
halves) or by 180 degrees about an axis, scales of 1/2, 1 or 2, whole translations — so that the file's own pose gives palettes that
are the identity bit for bit; the clips rotate by arbitrary angles."""
import base64
import copy
import json

import numpy as np

import deform_ref as D
import gltf_writer
import scene_edits as E
from hala_renderer_amd import scenes
from hala_renderer_amd.scene import HalaMesh, HalaNode, HalaPrimitive

f32 = np.float32
BODY, BOTH, MORPH = 3, 4, 5  # meshes: two skinned primitives under one skin; skin + targets; targets only
PATHS = {"translation": 0, "rotation": 1, "scale": 2, "weights": 3}


# ---- matrices -----------------------------------------------------------------------------------------------------------------------------
def trs_matrix(t, q, s):
    """T * R * S in float64 -> [4, 4]"""
    x, y, z, w = (float(v) for v in q)
    r = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=np.float64)
    m = np.eye(4, dtype=np.float64)
    m[:3, :3] = r * np.asarray(s, dtype=np.float64)[None, :]
    m[:3, 3] = np.asarray(t, dtype=np.float64)
    return m


def big_strip(vertex_count, seed, origin=(16.0, 24.0, 8.0)):
    """deform_ref.strip scaled to the size of the Cornell box, without a zero coordinate"""
    idx, v = D.strip(vertex_count, seed=seed, origin=(1.0, 1.0, 1.0))
    v["position"] = (v["position"] * np.array([8.0, 60.0, 8.0], dtype=f32) + np.asarray(origin, dtype=f32)).astype(f32)
    assert (v["position"] != 0).all() and (v["normal"] != 0).all() and (v["tangent"] != 0).all()
    return idx, v


# ---- the document -------------------------------------------------------------------------------------------------------------------------
HALF = (0.5, 0.5, 0.5, 0.5)  # 120 degrees about (1, 1, 1): a cyclic permutation of the axes, exact
# the rig's nodes, by name: (parent name, translation, rotation, scale, mesh)
RIG_NODES = [
    ("armature", None, (120.0, 40.0, 200.0), (0.0, 0.0, 0.0, 1.0), (1.0, 1.0, 1.0), None),
    ("joint0", "armature", (8.0, 0.0, 0.0), HALF, (2.0, 1.0, 1.0), None),
    ("joint1", "joint0", (0.0, 32.0, 0.0), (0.0, 1.0, 0.0, 0.0), (1.0, 0.5, 1.0), None),
    ("joint2", "joint1", (0.0, 0.0, 16.0), (-0.5, -0.5, -0.5, 0.5), (0.5, 2.0, 1.0), None),
    ("body", None, (100.0, 100.0, 250.0), (0.0, 0.0, 1.0, 0.0), (1.0, 2.0, 0.5), BODY),
    ("both", "armature", (64.0, 16.0, -32.0), HALF, (0.5, 0.5, 2.0), BOTH),
    ("morph", None, (300.0, 260.0, 300.0), (1.0, 0.0, 0.0, 0.0), (2.0, 1.0, 1.0), MORPH),
]
SKINS = [dict(joints=["joint0", "joint1", "joint2"], mesh_node="body", ibm=True), dict(joints=["joint2", "joint0"], mesh_node="both", ibm=True),
         dict(joints=["joint1"], mesh_node=None, ibm=False)]  # the last: no inverse bind matrices, no node uses it


def _unit(q):
    q = np.asarray(q, dtype=np.float64)
    return (q / np.linalg.norm(q)).astype(f32)


def _clips(rs):
    """three clips over all four paths and all three interpolations"""
    def quats(n):
        return np.stack([_unit(rs.normal(size=4)) for _ in range(n)])

    q = quats(5)
    if np.dot(q[0].astype(np.float64), q[1].astype(np.float64)) >= 0:  # keys 0 -> 1 have a negative dot ...
        q[1] = -q[1]
    q[3] = _unit(q[2].astype(np.float64) + 0.01 * rs.normal(size=4))  # ... and keys 2 -> 3 are closer than a dot of 0.9995
    assert np.dot(q[0].astype(np.float64), q[1].astype(np.float64)) < 0 and np.dot(q[2].astype(np.float64), q[3].astype(np.float64)) > 0.9995
    assert abs(np.dot(q[1].astype(np.float64), q[2].astype(np.float64))) < 0.9995
    spline_q = np.stack([np.stack([0.2 * rs.normal(size=4), _unit(rs.normal(size=4)), 0.2 * rs.normal(size=4)]) for _ in range(3)]).astype(f32)
    return [
        dict(name="bend", channels=[
            dict(node="joint1", path="rotation", interpolation="LINEAR", times=[0.0, 0.5, 1.25, 1.5, 2.0], values=q),
            dict(node="armature", path="translation", interpolation="LINEAR", times=[0.25, 1.0, 1.75],
                 values=(np.array([120.0, 40.0, 200.0]) + rs.uniform(-30, 30, (3, 3))).astype(f32)),
            dict(node="joint2", path="scale", interpolation="STEP", times=[0.0, 0.75, 1.5], values=rs.uniform(0.5, 2.0, (3, 3)).astype(f32)),
        ]),
        dict(name="spline", channels=[
            dict(node="joint0", path="rotation", interpolation="CUBICSPLINE", times=[0.0, 1.0, 2.5], values=spline_q.reshape(3, 12)),
            dict(node="joint1", path="translation", interpolation="CUBICSPLINE", times=[0.5, 1.5],
                 values=(rs.uniform(-20, 20, (2, 3, 3)) + np.array([0.0, 32.0, 0.0])[None, None, :] * np.array([0, 1, 0])[None, :, None]).astype(f32).reshape(2, 9)),
            dict(node="morph", path="weights", interpolation="CUBICSPLINE", times=[0.0, 2.0], values=rs.uniform(-0.5, 1.0, (2, 9)).astype(f32)),
            dict(node="both", path="rotation", interpolation="STEP", times=[0.0, 1.25], values=quats(2)),
        ]),
        dict(name="", channels=[
            dict(node="both", path="weights", interpolation="LINEAR", times=[0.0, 1.0, 2.0], values=rs.uniform(-1.0, 1.5, (3, 2)).astype(f32)),
            dict(node="morph", path="weights", interpolation="STEP", times=[0.5, 1.5], values=rs.uniform(-0.5, 1.0, (2, 3)).astype(f32)),
            dict(node="joint0", path="scale", interpolation="LINEAR", times=[1.0], values=np.array([[1.5, 0.75, 1.25]], dtype=f32)),  # one key
            dict(node="body", path="translation", interpolation="LINEAR", times=[0.0, 2.0], values=np.array([[100, 100, 250], [160, 130, 220]], dtype=f32)),
            dict(node="body", path="rotation", interpolation="LINEAR", times=[0.0, 2.0], values=np.stack([np.array([0, 0, 1, 0], dtype=f32), _unit([0.2, 0.1, 0.9, 0.3])])),
        ]),
    ]


class _Buffer:
    def __init__(self, doc):
        self.doc = doc
        uri = doc["buffers"][0]["uri"]
        self.buf = bytearray(base64.b64decode(uri[uri.index(",") + 1:]))

    def view(self, arr):
        arr = np.ascontiguousarray(arr)
        while len(self.buf) % 4:
            self.buf.append(0)
        self.doc["bufferViews"].append({"buffer": 0, "byteOffset": len(self.buf), "byteLength": arr.nbytes})
        self.buf.extend(arr.tobytes())
        return len(self.doc["bufferViews"]) - 1

    def add(self, arr, ctype, atype, normalized=False):
        arr = np.ascontiguousarray(arr)
        acc = {"bufferView": self.view(arr), "componentType": ctype, "count": int(arr.shape[0]), "type": atype}
        if normalized:
            acc["normalized"] = True
        self.doc["accessors"].append(acc)
        return len(self.doc["accessors"]) - 1

    def add_sparse(self, arr, rows):
        """a float VEC3 accessor of zeros whose `rows` are replaced (no buffer view of its own)"""
        arr = np.ascontiguousarray(arr, dtype=f32)
        self.doc["accessors"].append({"componentType": 5126, "count": int(arr.shape[0]), "type": "VEC3",
                                      "sparse": {"count": len(rows), "indices": {"bufferView": self.view(np.asarray(rows, dtype=np.uint16)), "componentType": 5123},
                                                 "values": {"bufferView": self.view(arr[rows])}}})
        return len(self.doc["accessors"]) - 1

    def close(self):
        self.doc["buffers"][0] = {"byteLength": len(self.buf), "uri": "data:application/octet-stream;base64," + base64.b64encode(bytes(self.buf)).decode()}


_CACHE = {}


def character():
    """-> dict(doc: the glTF document, truth: what the writer put in, by name) — built once, never changed (callers copy)"""
    if "c" in _CACHE:
        return _CACHE["c"]
    rs = np.random.RandomState(77)
    scene = scenes.cornell_box(aspect=E.W / E.H_)
    assert len(scene.meshes) == 3
    prims = {BODY: [big_strip(70, 1), big_strip(33, 2, origin=(16.0, 150.0, 8.0))], BOTH: [big_strip(65, 3)], MORPH: [big_strip(40, 4)]}
    scene.meshes = list(scene.meshes) + [HalaMesh([HalaPrimitive(i, v, material_index=k % 3) for i, v in prims[m]]) for k, m in enumerate((BODY, BOTH, MORPH))]
    first_rig_node = len(scene.nodes)
    names = [n[0] for n in RIG_NODES]
    for name, parent, t, q, s, mesh in RIG_NODES:
        scene.nodes = list(scene.nodes) + [HalaNode(name=name, parent=None if parent is None else first_rig_node + names.index(parent),
                                                    local_transform=trs_matrix(t, q, s).astype(f32), **({} if mesh is None else {"mesh_index": mesh}))]
    import os
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        gltf_writer.write_gltf(scene, os.path.join(tmp, "c.gltf"))
        doc = json.load(open(os.path.join(tmp, "c.gltf")))
    b = _Buffer(doc)
    index = {name: first_rig_node + k for k, name in enumerate(names)}
    world = {}
    for name, parent, t, q, s, mesh in RIG_NODES:
        n = doc["nodes"][index[name]]
        del n["matrix"]
        n["translation"], n["rotation"], n["scale"] = [float(x) for x in t], [float(x) for x in q], [float(x) for x in s]
        world[name] = (world[parent] if parent else np.eye(4)) @ trs_matrix(t, q, s)
    truth = dict(skins=[], bindings=[], clips=[], index=index, scene=scene)
    doc["skins"] = []
    for k, sk in enumerate(SKINS):
        js = {"joints": [index[j] for j in sk["joints"]]}
        ibm = np.tile(np.eye(4, dtype=f32).reshape(1, 16), (len(sk["joints"]), 1))
        if sk["ibm"]:
            ibm = np.stack([(np.linalg.inv(world[j]) @ world[sk["mesh_node"]]).T.reshape(16) for j in sk["joints"]]).astype(f32)  # column-major
            js["inverseBindMatrices"] = b.add(ibm, 5126, "MAT4")
        doc["skins"].append(js)
        if sk["mesh_node"]:
            doc["nodes"][index[sk["mesh_node"]]]["skin"] = k
        truth["skins"].append(dict(joints=sk["joints"], ibm=ibm))
    # bindings: (mesh, primitive, skin, joints as, weights as, targets, normal deltas, tangent deltas, sparse, default weights)
    plan = [(BODY, 0, 0, np.uint8, "float", 0, False, False, False, None), (BODY, 1, 0, np.uint16, "u8", 0, False, False, False, None),
            (BOTH, 0, 1, np.uint8, "u16", 2, True, False, True, None), (MORPH, 0, None, None, None, 3, False, True, False, [0.25, 0.0, -0.5])]
    for mesh, p, skin, jt, wt, nt, nrm, tan, sparse, dflt in plan:
        jp = doc["meshes"][mesh]["primitives"][p]
        nv = len(prims[mesh][p][1])
        rig = D.random_rig(nv, targets=nt, joint_count=len(SKINS[skin]["joints"]) if skin is not None else 0, normals=nrm, tangents=tan, seed=10 * mesh + p,
                           scale=40.0, dyadic=True)
        if skin is not None:
            jp["attributes"]["JOINTS_0"] = b.add(rig["joints"].astype(jt), 5121 if jt == np.uint8 else 5123, "VEC4")
            w = rig["weights"]  # multiples of 1/4
            if wt == "u16":  # one influence of 1: 65535 / 65535 is 1 exactly, so this primitive's bind pose is its loaded vertices bit for bit
                w = np.eye(4, dtype=f32)[np.argmax(w, axis=1)]
            if wt == "float":
                jp["attributes"]["WEIGHTS_0"] = b.add(w, 5126, "VEC4")
            else:
                top = 255 if wt == "u8" else 65535
                q = np.round(w.astype(np.float64) * top).astype(np.uint8 if wt == "u8" else np.uint16)
                jp["attributes"]["WEIGHTS_0"] = b.add(q, 5121 if wt == "u8" else 5123, "VEC4", normalized=True)
                rig["weights"] = (q.astype(f32) / f32(top)).astype(f32)
            if mesh == BODY and p == 1:  # a second influence set: counted, not read
                jp["attributes"]["JOINTS_1"] = jp["attributes"]["JOINTS_0"]; jp["attributes"]["WEIGHTS_1"] = jp["attributes"]["WEIGHTS_0"]
        if nt:
            jp["targets"] = []
            if sparse:
                rows = sorted(rs.choice(nv, 7, replace=False).tolist())
                keep = np.zeros_like(rig["targets"][1]); keep[rows] = rig["targets"][1][rows]
                rig["targets"][1] = keep
            for t in range(nt):
                jt_ = {"POSITION": b.add_sparse(rig["targets"][t], rows) if sparse and t == 1 else b.add(rig["targets"][t], 5126, "VEC3")}
                if nrm:
                    jt_["NORMAL"] = b.add(rig["normal_targets"][t], 5126, "VEC3")
                if tan and t != 1:  # a target without the attribute: zeros
                    jt_["TANGENT"] = b.add(rig["tangent_targets"][t], 5126, "VEC3")
                elif tan:
                    rig["tangent_targets"][t] = 0.0
                jp["targets"].append(jt_)
            if dflt is not None:
                doc["meshes"][mesh]["weights"] = dflt
        node = [n[0] for n in RIG_NODES if n[5] == mesh][0]
        truth["bindings"].append(dict(mesh=mesh, prim=p, node=node, skin=skin, rig=rig, sets=2 if (mesh, p) == (BODY, 1) else (1 if skin is not None else 0),
                                      default=np.asarray(dflt if dflt is not None else [0.0] * nt, dtype=f32)))
    doc["animations"] = []
    for clip in _clips(rs):
        ja = {"samplers": [], "channels": []}
        if clip["name"]:
            ja["name"] = clip["name"]
        for ch in clip["channels"]:
            v = np.asarray(ch["values"], dtype=f32)
            per = {"translation": 3, "rotation": 4, "scale": 3}.get(ch["path"])
            out = b.add(v.reshape(-1, 1), 5126, "SCALAR") if per is None else b.add(v.reshape(-1, per), 5126, "VEC3" if per == 3 else "VEC4")
            ja["samplers"].append({"input": b.add(np.asarray(ch["times"], dtype=f32).reshape(-1, 1), 5126, "SCALAR"), "output": out, "interpolation": ch["interpolation"]})
            ja["channels"].append({"sampler": len(ja["samplers"]) - 1, "target": {"node": index[ch["node"]], "path": ch["path"]}})
        doc["animations"].append(ja)
        truth["clips"].append(clip)
    b.close()
    # list the nodes in another order: the breadth-first walk has to renumber them
    n = len(doc["nodes"])
    new_of_old = list(rs.permutation(n))
    assert new_of_old != list(range(n))
    nodes = [None] * n
    for old, nd in enumerate(doc["nodes"]):
        nd = copy.deepcopy(nd)
        if "children" in nd:
            nd["children"] = [int(new_of_old[c]) for c in nd["children"]]
        nodes[new_of_old[old]] = nd
    doc["nodes"] = nodes
    doc["scenes"][0]["nodes"] = [int(new_of_old[r]) for r in doc["scenes"][0]["nodes"]]
    for sk in doc["skins"]:
        sk["joints"] = [int(new_of_old[j]) for j in sk["joints"]]
    for an in doc["animations"]:
        for ch in an["channels"]:
            ch["target"]["node"] = int(new_of_old[ch["target"]["node"]])
    truth["gltf_index"] = {name: int(new_of_old[i]) for name, i in index.items()}
    _CACHE["c"] = dict(doc=doc, truth=truth)
    return _CACHE["c"]


def character_doc():
    return copy.deepcopy(character()["doc"])


def singular_doc():
    """the character plus clip 3, whose STEP scale channel squashes the `body` mesh node flat from time 1 on: no inverse, no palette"""
    doc = character_doc()
    b = _Buffer(doc)
    sampler = {"input": b.add(np.array([[0.0], [1.0]], dtype=f32), 5126, "SCALAR"), "output": b.add(np.array([[1.0, 2.0, 0.5], [0.0, 2.0, 0.5]], dtype=f32), 5126, "VEC3"),
               "interpolation": "STEP"}
    b.close()
    doc["animations"].append({"name": "squash", "samplers": [sampler], "channels": [{"sampler": 0, "target": {"node": character()["truth"]["gltf_index"]["body"], "path": "scale"}}]})
    return doc


def save(doc, path):
    with open(path, "w") as f:
        json.dump(doc, f)
    return str(path)


def strip_rig(doc):
    """the same document without skins, targets and animations"""
    doc = copy.deepcopy(doc)
    doc.pop("skins", None); doc.pop("animations", None)
    for n in doc["nodes"]:
        n.pop("skin", None)
    for m in doc["meshes"]:
        m.pop("weights", None)
        for p in m["primitives"]:
            p.pop("targets", None)
            for k in [k for k in p["attributes"] if k.startswith("JOINTS_") or k.startswith("WEIGHTS_")]:
                del p["attributes"][k]
    return doc


def malformed():
    """-> [(name, document, words the loader's message holds)]: one per case the loader must refuse"""
    c = character()
    gi = c["truth"]["gltf_index"]
    out = []

    def case(name, words, change):
        doc = character_doc()
        change(doc)
        out.append((name, doc, words))

    def channel(doc, clip, k):
        return doc["animations"][clip]["channels"][k]

    def sampler_acc(doc, clip, k, which):
        return doc["accessors"][doc["animations"][clip]["samplers"][k][which]]

    def rewrite_times(doc, clip, k, times):
        b = _Buffer(doc)
        doc["animations"][clip]["samplers"][k]["input"] = b.add(np.asarray(times, dtype=f32).reshape(-1, 1), 5126, "SCALAR")
        b.close()

    case("joint-out-of-range", "joint of skin 0 is out of range", lambda d: d["skins"][0]["joints"].__setitem__(1, len(d["nodes"])))
    case("channel-node-out-of-range", "node of a channel of animation 0 is out of range", lambda d: channel(d, 0, 0)["target"].__setitem__("node", len(d["nodes"]) + 3))
    case("inverse-bind-count", "inverse bind matrices for 2 joints", lambda d: d["skins"][0]["joints"].pop())
    case("times-not-increasing", "not finite and strictly increasing", lambda d: rewrite_times(d, 0, 0, [0.0, 0.5, 0.5, 1.5, 2.0]))
    case("times-not-finite", "not finite and strictly increasing", lambda d: rewrite_times(d, 0, 1, [0.25, np.inf, np.nan]))
    case("output-count", "values for 5 keys", lambda d: sampler_acc(d, 0, 0, "output").__setitem__("count", 4))
    case("cubicspline-output-count", "values for 3 keys", lambda d: d["animations"][1]["samplers"][0].__setitem__("interpolation", "LINEAR"))
    case("weights-on-node-without-mesh", "node without a morphed mesh", lambda d: channel(d, 2, 0)["target"].__setitem__("node", gi["joint1"]))
    case("weights-width", "values for 3 keys", lambda d: channel(d, 2, 0)["target"].__setitem__("node", gi["morph"]))
    case("target-counts-differ", "primitives of mesh 3 have different target counts",
         lambda d: d["meshes"][BODY]["primitives"][1].__setitem__("targets", copy.deepcopy(d["meshes"][MORPH]["primitives"][0]["targets"][:1])))
    case("target-vertex-count", "does not have one VEC3 per vertex",
         lambda d: d["meshes"][MORPH]["primitives"][0]["targets"][0].__setitem__("POSITION", d["meshes"][BOTH]["primitives"][0]["targets"][0]["POSITION"]))
    case("joints-vertex-count", "JOINTS_0 of mesh 3 primitive 1 does not have one VEC4 per vertex",
         lambda d: d["meshes"][BODY]["primitives"][1]["attributes"].__setitem__("JOINTS_0", d["meshes"][BODY]["primitives"][0]["attributes"]["JOINTS_0"]))

    def to_matrix(d):
        n = d["nodes"][gi["joint1"]]
        n["matrix"] = trs_matrix(n.pop("translation"), n.pop("rotation"), n.pop("scale")).T.reshape(-1).tolist()
    case("channel-on-matrix-node", "which is given as a matrix", to_matrix)
    return out


# ---- the twin -----------------------------------------------------------------------------------------------------------------------------
class Twin:
    """RENDER_SPEC 19 from the glTF JSON, in numpy float64"""

    def __init__(self, doc):
        self.doc = doc
        uri = doc["buffers"][0]["uri"]
        self.buf = base64.b64decode(uri[uri.index(",") + 1:])
        # the loader's numbering: breadth-first from the scene roots, parents before children
        self.scene_of_gltf, self.gltf_of_scene, self.parent = {}, [], []
        queue = [(-1, r) for sc in doc["scenes"] for r in sc["nodes"]]
        while queue:
            parent, g = queue.pop(0)
            self.scene_of_gltf[g] = len(self.gltf_of_scene)
            self.gltf_of_scene.append(g); self.parent.append(parent)
            queue += [(self.scene_of_gltf[g], c) for c in doc["nodes"][g].get("children", [])]
        self.n = len(self.gltf_of_scene)
        self.trs, self.loaded = [], []
        for g in self.gltf_of_scene:
            nd = doc["nodes"][g]
            if "matrix" in nd:
                self.trs.append(None)
                self.loaded.append(np.asarray(nd["matrix"], dtype=f32).reshape(4, 4).T.copy())
            else:
                t, q, s = nd.get("translation", [0, 0, 0]), nd.get("rotation", [0, 0, 0, 1]), nd.get("scale", [1, 1, 1])
                self.trs.append((np.asarray(t, dtype=f32), np.asarray(q, dtype=f32), np.asarray(s, dtype=f32)))
                self.loaded.append(trs_matrix(t, q, s).astype(f32))
        # bindings, mesh-major: a primitive with targets, or with JOINTS_0 / WEIGHTS_0 under a node that has a skin
        self.bindings = []
        for m, mesh in enumerate(doc["meshes"]):
            nodes = [k for k, g in enumerate(self.gltf_of_scene) if doc["nodes"][g].get("mesh") == m]
            if not nodes:
                continue
            skin = doc["nodes"][self.gltf_of_scene[nodes[0]]].get("skin")
            for p, prim in enumerate(mesh["primitives"]):
                nt = len(prim.get("targets", []))
                skinned = skin is not None and "JOINTS_0" in prim["attributes"] and "WEIGHTS_0" in prim["attributes"]
                if not nt and not skinned:
                    continue
                self.bindings.append(dict(mesh=m, prim=p, node=nodes[0], node_count=len(nodes), skin=skin if skinned else None, target_count=nt,
                                          default=np.asarray(mesh.get("weights", [0.0] * nt), dtype=f32)))

    def accessor(self, k):
        a = self.doc["accessors"][k]
        dt = {5120: np.int8, 5121: np.uint8, 5122: np.int16, 5123: np.uint16, 5125: np.uint32, 5126: np.float32}[a["componentType"]]
        nc = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4, "MAT4": 16}[a["type"]]

        def read(view, offset, count, dtype, ncomp):
            v = self.doc["bufferViews"][view]
            start = v.get("byteOffset", 0) + offset
            return np.frombuffer(self.buf, dtype=dtype, count=count * ncomp, offset=start).reshape(count, ncomp)

        out = read(a["bufferView"], a.get("byteOffset", 0), a["count"], dt, nc).copy() if "bufferView" in a else np.zeros((a["count"], nc), dtype=dt)
        if "sparse" in a:
            sp = a["sparse"]
            it = {5121: np.uint8, 5123: np.uint16, 5125: np.uint32}[sp["indices"]["componentType"]]
            rows = read(sp["indices"]["bufferView"], sp["indices"].get("byteOffset", 0), sp["count"], it, 1)[:, 0]
            out[rows.astype(np.int64)] = read(sp["values"]["bufferView"], sp["values"].get("byteOffset", 0), sp["count"], dt, nc)
        if a.get("normalized") and dt != np.float32:
            out = out.astype(f32) / f32(np.iinfo(dt).max)
        return out

    def binding_tables(self, b):
        """-> the dict tests/deform_ref.py poses with (targets, normal_targets, tangent_targets, joints, weights, joint_count)"""
        prim = self.doc["meshes"][b["mesh"]]["primitives"][b["prim"]]
        nv = self.doc["accessors"][prim["attributes"]["POSITION"]]["count"]
        out = dict(targets=None, normal_targets=None, tangent_targets=None, joints=None, weights=None, joint_count=0)
        if b["target_count"]:
            for key, attr in (("targets", "POSITION"), ("normal_targets", "NORMAL"), ("tangent_targets", "TANGENT")):
                if attr == "POSITION" or any(attr in t for t in prim["targets"]):
                    out[key] = np.stack([self.accessor(t[attr]).astype(f32) if attr in t else np.zeros((nv, 3), f32) for t in prim["targets"]])
        if b["skin"] is not None:
            out["joints"] = self.accessor(prim["attributes"]["JOINTS_0"]).astype(np.uint16)
            out["weights"] = self.accessor(prim["attributes"]["WEIGHTS_0"]).astype(f32)
            out["joint_count"] = len(self.doc["skins"][b["skin"]]["joints"])
        return out

    @staticmethod
    def _sample(times, values, mode, width, t, rotation):
        times = times.astype(np.float64); n = len(times)
        cubic = mode == "CUBICSPLINE"
        v = values.astype(np.float64).reshape(n, 3 if cubic else 1, width)
        val = v[:, 1 if cubic else 0]
        if n == 1 or t <= times[0]:
            return val[0]
        if t >= times[-1]:
            return val[-1]
        k = int(np.searchsorted(times, t, side="right")) - 1
        dt = times[k + 1] - times[k]
        u = (t - times[k]) / dt
        if mode == "STEP":
            return val[k]
        if cubic:
            out = (2 * u ** 3 - 3 * u ** 2 + 1) * val[k] + (u ** 3 - 2 * u ** 2 + u) * (dt * v[k, 2]) + (-2 * u ** 3 + 3 * u ** 2) * val[k + 1] + (u ** 3 - u ** 2) * (dt * v[k + 1, 0])
            return out / np.linalg.norm(out) if rotation else out
        if rotation:
            a, b = val[k], val[k + 1]
            d = float(a @ b)
            if d < 0:
                b, d = -b, -d
            if d > 0.9995:
                out = a + u * (b - a)
                return out / np.linalg.norm(out)
            th = np.arccos(d)
            return (np.sin((1 - u) * th) / np.sin(th)) * a + (np.sin(u * th) / np.sin(th)) * b
        return val[k] + u * (val[k + 1] - val[k])

    def sample(self, clip, t):
        """-> dict(locals [N, 4, 4] float32, touched [N] bool, weights / palettes: one entry per binding or None)"""
        doc = self.doc
        local = [m.copy() for m in self.loaded]
        touched = np.zeros(self.n, dtype=bool)
        weights = [b["default"].copy() if b["target_count"] else None for b in self.bindings]
        if clip is None:
            for an in doc.get("animations", []):
                for ch in an["channels"]:
                    if ch["target"]["path"] != "weights":
                        touched[self.scene_of_gltf[ch["target"]["node"]]] = True
        else:
            an = doc["animations"][clip]
            trs = [None if x is None else [c.astype(np.float64) for c in x] for x in self.trs]
            for ch in an["channels"]:
                node = self.scene_of_gltf[ch["target"]["node"]]
                path = ch["target"]["path"]
                s = an["samplers"][ch["sampler"]]
                times = self.accessor(s["input"])[:, 0]
                width = {"translation": 3, "rotation": 4, "scale": 3}.get(path) or [b["target_count"] for b in self.bindings if b["node"] == node][0]
                v = self._sample(times, self.accessor(s["output"]), s.get("interpolation", "LINEAR"), width, float(f32(t)), path == "rotation")
                if path == "weights":
                    for k, b in enumerate(self.bindings):
                        if b["node"] == node:
                            weights[k] = v.astype(f32)
                else:
                    trs[node][PATHS[path]] = v
                    touched[node] = True
            for k in np.nonzero(touched)[0]:
                local[k] = trs_matrix(*trs[k]).astype(f32)
        world = []
        for k in range(self.n):
            l = local[k].astype(np.float64)
            world.append(l if self.parent[k] < 0 else world[self.parent[k]] @ l)
        palettes = []
        for b in self.bindings:
            if b["skin"] is None:
                palettes.append(None)
                continue
            sk = doc["skins"][b["skin"]]
            ibm = self.accessor(sk["inverseBindMatrices"]).astype(np.float64).reshape(-1, 4, 4).transpose(0, 2, 1) if "inverseBindMatrices" in sk else \
                np.tile(np.eye(4), (len(sk["joints"]), 1, 1))
            inv = np.linalg.inv(world[b["node"]])
            palettes.append(np.stack([(inv @ world[self.scene_of_gltf[j]] @ ibm[i])[:3] for i, j in enumerate(sk["joints"])]).astype(f32))
        return dict(locals=np.stack(local), touched=touched, weights=weights, palettes=palettes)


def within_one_ulp(got, want):
    """each matrix or vector (the last two axes, or the last one) differs by at most one float32 ulp at the magnitude of its largest entry"""
    got, want = np.asarray(got, dtype=f32), np.asarray(want, dtype=f32)
    if got.shape != want.shape:
        return False
    axes = tuple(range(max(got.ndim - 2, 0), got.ndim)) if got.ndim >= 2 else None
    top = np.maximum(np.abs(got).max(axis=axes, keepdims=True), np.abs(want).max(axis=axes, keepdims=True))
    ulp = np.spacing(top.astype(f32))
    return bool((np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp.astype(np.float64)).all())
