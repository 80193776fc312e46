#!/usr/bin/env python3
"""Prints a sha256 of the built tree (download_bvh() and download_instance_refs()) for a fixed list of scenes and build options, three
times per entry: after commit(), after a refit with one node moved, after a refit with one mesh's vertices rippled.  Run it against two
builds of the library (HALART_LIB selects one) to show that a change of the builder leaves every tree as it was:
  python scripts/tree_digest.py --out a.json;  HALART_LIB=/path/to/other/libhalart.so python scripts/tree_digest.py --out b.json
  python scripts/tree_digest.py --compare a.json b.json"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402


def entries(big):
    from hala_renderer_amd import scenes
    from test_gpu_parity import SMALL_TREES, small_scene
    yield "cornell", scenes.cornell_box, {}
    yield "bunny_class(5)", lambda: scenes.bunny_class(subdivisions=5), {}
    for builder in ("sah", "ploc", "lbvh"):
        for instancing in (False, True):
            yield f"sponza_class(60000) {builder} instancing={instancing}", lambda: scenes.sponza_class(target_triangles=60_000), dict(builder=builder, instancing=instancing)
    if big:
        yield "sponza_class(1000000)", lambda: scenes.sponza_class(target_triangles=1_000_000), {}
    for n, builder, drive in SMALL_TREES:
        yield f"small n={n} {builder} {drive}", lambda n=n: small_scene(n), dict(builder=builder, instancing=False, **drive)


def digest(r):
    h = hashlib.sha256()
    nodes, tris = r.download_bvh()
    i = r.bvh_info()
    h.update(nodes.tobytes()); h.update(tris.tobytes()); h.update(r.download_instance_refs().tobytes())
    h.update(np.array([i.node_count, i.max_depth, i.triangle_count], dtype=np.uint32).tobytes())
    h.update(np.array(list(i.scene_min) + list(i.scene_max), dtype=np.float32).tobytes())
    return h.hexdigest()


def three_digests(H, scene, build):
    r = H.HalaRenderer("digest", 16, 16, 5, 3, False, False, False, 0)
    r.set_build_options(**build)
    r.set_scene(scene)
    r.commit()
    out = [digest(r)]
    node = next(k for k, n in enumerate(scene.nodes) if getattr(n, "mesh_index", 0xffffffff) != 0xffffffff)
    m = np.array(scene.nodes[node].local_transform, dtype=np.float32).reshape(4, 4).copy()
    m[0, 3] += np.float32(0.03125)
    r.update_node_transform(node, m)
    r.refit()
    out.append(digest(r))
    mesh = scene.nodes[node].mesh_index
    v = scene.meshes[mesh].primitives[0].vertices.copy()
    pos = v["position"]
    amp = np.float32(0.02) * (pos.max() - pos.min())
    pos[:, 2] += (amp * np.sin(3.0 * pos[:, 0] + 1.7 * pos[:, 1])).astype(np.float32)
    r.update_vertices(mesh, 0, v)
    r.refit()
    out.append(digest(r))
    r.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--no-big", action="store_true", help="leave the 1 M-triangle atrium out")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.compare:
        x, y = (json.load(open(p))["digests"] for p in a.compare)
        bad = [k for k in sorted(set(x) | set(y)) if x.get(k) != y.get(k)]
        print(f"{len(x)} / {len(y)} entries, {len(bad)} differ", *bad, sep="\n")
        sys.exit(1 if bad or not x else 0)
    import hala_renderer_amd as H
    res = {}
    for name, make, build in entries(not a.no_big):
        res[name] = three_digests(H, make(), build)
        print(name, *[d[:16] for d in res[name]], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"library": os.path.basename(H.LIB_PATH), "digests": res}, f, indent=1)


if __name__ == "__main__":
    main()
