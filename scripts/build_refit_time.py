#!/usr/bin/env python3
"""Times commit() (upload + BVH build) and refit() (node transforms -> instance records -> leaf boxes -> level pack) on the
1M-triangle atrium (or: triangle count, --builder, --instancing); run by hand on the GPU box.  The numbers quoted in DESIGN.md section 5 come from here."""
import argparse
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import hala_renderer_amd as H
from hala_renderer_amd import scenes

ap = argparse.ArgumentParser()
ap.add_argument("tris", nargs="?", type=int, default=1_000_000)
ap.add_argument("--builder", choices=("sah", "ploc", "lbvh"), default=None, help="default: automatic")
ap.add_argument("--instancing", action="store_true", help="two-level tree: one small tree per instanced primitive")
a = ap.parse_args()
s = scenes.sponza_class(target_triangles=a.tris)
r = H.HalaRenderer("time", 1920, 1080, 5, 3, True, True, False, 0)
if a.builder or a.instancing:
    r.set_build_options(builder=a.builder, instancing=True if a.instancing else None)
r.set_scene(s)
t0 = time.perf_counter(); r.commit(); t1 = time.perf_counter()
print("triangles", r.bvh_info().triangle_count, "first commit ms %.2f" % ((t1 - t0) * 1e3), flush=True)
t0 = time.perf_counter(); r.commit(); t1 = time.perf_counter()
print("second commit ms %.2f" % ((t1 - t0) * 1e3), flush=True)
node = next(k for k, n in enumerate(s.nodes) if getattr(n, "mesh_index", 0xffffffff) != 0xffffffff)
m = np.array(s.nodes[node].local_transform, dtype=np.float32).reshape(4, 4).copy()
best = 1e9
for k in range(6):
    m[0, 3] += 0.01
    r.update_node_transform(node, m)
    t0 = time.perf_counter(); r.refit(); t1 = time.perf_counter()
    best = min(best, t1 - t0)
print("refit ms (best of 6) %.3f" % (best * 1e3))
r.update(); r.render()
r.close()
