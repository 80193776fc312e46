"""Time GPU-resident deformers (hala_rt_set_deformer, docs/RENDER_SPEC.md 17) and write profiles/deform_timing.json.

configs[3] (atrium); a deformer with 2 morph targets (position and normal deltas) and 32 joints on its largest primitive.  Per pose
change, over `--poses` poses, host wall time until the renderer's stream is idle:
  (a) update_deformer + refit: a few hundred bytes handed over, k_deform, the refit;
  (b) update_vertices with the same posed array (tests/deform_ref.py makes it) + refit: the path without a deformer.
  (c) k_deform alone, from the kernel trace of `--child` (the (a) loop in a process of its own under
      `rocprofv3 --kernel-trace --output-format csv`), with the achieved GB/s against the byte model of DESIGN.md 17.

With --parent-root, bench.py of this tree and of the parent commit's tree (built there) also alternate, `--bench-rounds` times, each as
its own process: bench.py --gpus 1 --steps K --warmup W --no-cpu-baseline --no-secondary."""
import argparse
import csv
import glob
import json
import os
import platform
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))  # deform_ref (needs the test tree): the twin makes the rig, the poses and the posed arrays of (b)

import deform_ref as D  # noqa: E402
import hala_renderer_amd as H  # noqa: E402
from hala_renderer_amd import workloads  # noqa: E402

TARGETS, JOINTS = 2, 32


def summary(xs):
    return {"median": statistics.median(xs), "mean": statistics.fmean(xs), "min": min(xs), "max": max(xs), "stdev": statistics.pstdev(xs), "poses": len(xs)}


def setup():
    cfg = workloads.baseline_config(3)
    scene = cfg["scene"]
    mesh, prim = max(((m, p) for m in range(len(scene.meshes)) for p in range(len(scene.meshes[m].primitives))),
                     key=lambda mp: len(scene.meshes[mp[0]].primitives[mp[1]].vertices))
    rest = scene.meshes[mesh].primitives[prim].vertices
    r = H.HalaRenderer("deform-timing", cfg["width"], cfg["height"], cfg["max_depth"], cfg["rr_depth"], False, False, False, 0)
    r.set_envmap(cfg["env"], 0.0)
    r.set_scene(scene)
    r.commit()
    pos = rest["position"].astype(np.float64)
    extent = float(np.ptp(pos, axis=0).max())
    rig = D.random_rig(len(rest), targets=TARGETS, joint_count=JOINTS, normals=True, seed=17, scale=0.02 * extent)
    return r, scene, mesh, prim, rest, rig, 0.5 * (pos.min(0) + pos.max(0)), extent


def pose_of(rig, k, centre, extent):
    return D.random_pose(rig, seed=k, zero_some=False, centre=centre, scale=0.05 * extent)


def model_bytes(vertices):
    """rest read + posed written + 12 B per active target and attribute with deltas + 24 B of skin bindings"""
    return vertices * (44 + 44 + TARGETS * 2 * 12 + 24)


def timed(r, fn):
    r.wait_idle()
    t0 = time.perf_counter()
    fn()
    r.wait_idle()
    return (time.perf_counter() - t0) * 1e3


def child(poses):
    r, _, mesh, prim, _, rig, centre, extent = setup()
    r.set_deformer(mesh, prim, **rig)
    for k in range(poses):
        r.update_deformer(mesh, prim, **pose_of(rig, k, centre, extent))
        r.refit()
    r.wait_idle()
    r.close()


def kernel_trace(poses):
    """-> the durations (ms) of every k_deform launch of a --child run under rocprofv3"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "t", "--", sys.executable, os.path.abspath(__file__), "--child", str(poses)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            raise RuntimeError(f"the traced run failed ({p.returncode}): {p.stderr[-2000:]}")
        out = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    if re.search(r"\bk_deform\(", row["Kernel_Name"]):  # (the name itself: not k_deform_faces, k_deform_vertex_normals)
                        out.append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6)
    if not out:
        raise RuntimeError("the kernel trace holds no k_deform launch")
    return out


def bench(root, steps, warmup):
    env = dict(os.environ)
    env.pop("HALART_LIB", None)
    root = os.path.abspath(root)
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--no-cpu-baseline", "--no-secondary"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise RuntimeError(f"bench.py in {root} failed ({p.returncode}): {p.stderr[-2000:]}")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    return json.loads(line)["ms_per_step"]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--poses", type=int, default=24)
    ap.add_argument("--child", type=int, default=0, help="only run the (a) loop with this many poses (what the kernel trace wraps)")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--bench-rounds", type=int, default=4)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deform_timing.json"))
    args = ap.parse_args()
    H.load_library()
    if args.child:
        child(args.child)
        return
    if args.poses < 20:
        ap.error("--poses must be at least 20")
    import torch
    res = {"what": "GPU-resident deformers (scripts/deform_timing.py): one pose change of the largest primitive of configs[3], "
                   f"{TARGETS} morph targets (position + normal deltas) + {JOINTS} joints; host wall ms until the stream is idle",
           "box": {"gpu": torch.cuda.get_device_name(0), "host": platform.processor() or platform.machine(), "hip": torch.version.hip}}

    def save():  # after every stage: a later one that fails keeps the earlier figures
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)

    r, scene, mesh, prim, rest, rig, centre, extent = setup()
    nv = len(rest)
    res["primitive"] = {"mesh": mesh, "primitive": prim, "vertices": nv, "triangles": len(scene.meshes[mesh].primitives[prim].indices) // 3,
                        "scene_triangles": int(r.bvh_info().triangle_count), "model_bytes_per_pose": model_bytes(nv),
                        "host_bytes_per_pose_deformer": 4 * (TARGETS + 12 * JOINTS), "host_bytes_per_pose_update_vertices": 44 * nv}
    poses = [pose_of(rig, k, centre, extent) for k in range(args.poses + 2)]
    r.set_deformer(mesh, prim, **rig)
    for p in poses[:2]:  # warm-up: first launches, allocations
        r.update_deformer(mesh, prim, **p); r.refit()
    a = []
    for p in poses[2:]:
        a.append(timed(r, lambda: (r.update_deformer(mesh, prim, **p), r.refit())))
    last = r.read_vertices(mesh, prim)
    res["a_update_deformer_refit_ms"] = summary(a)
    save()
    arrays = [D.pose_vertices(rest, rig, p) for p in poses]
    res["kernel_equals_twin_on_the_last_pose"] = bool(last.tobytes() == arrays[-1].tobytes())
    r.clear_deformer(mesh, prim)
    for v in arrays[:2]:
        r.update_vertices(mesh, prim, v); r.refit()
    b = []
    for v in arrays[2:]:
        b.append(timed(r, lambda: (r.update_vertices(mesh, prim, v), r.refit())))
    res["b_update_vertices_refit_ms"] = summary(b)
    r.update_vertices(mesh, prim, rest)
    r.refit()  # untimed: applies the vertex edit above, so that the refits below find nothing to do
    refit_only = [timed(r, r.refit) for _ in range(args.poses)]  # nothing moved: the host side of a refit, the tree untouched
    res["refit_without_an_edit_ms"] = summary(refit_only)
    r.close()
    save()
    if not args.no_trace:
        ms = kernel_trace(args.poses)
        res["c_k_deform_ms"] = summary(ms)
        res["c_k_deform_gb_per_s"] = {"at_median": model_bytes(nv) / (statistics.median(ms) * 1e-3) / 1e9, "at_min": model_bytes(nv) / (min(ms) * 1e-3) / 1e9}
        save()
    if args.parent_root:
        rounds = []
        for k in range(args.bench_rounds):  # the order within a round alternates too: whichever runs second finds the GPU warmer
            order = (("parent", args.parent_root), ("this", ROOT))[::1 if k % 2 == 0 else -1]
            ms = {name: bench(root, args.bench_steps, args.bench_warmup) for name, root in order}
            rounds.append({"order": [name for name, _ in order], "parent_ms_per_step": ms["parent"], "this_ms_per_step": ms["this"]})
            res["bench_alternating"] = {"command": f"bench.py --gpus 1 --steps {args.bench_steps} --warmup {args.bench_warmup} --no-cpu-baseline --no-secondary", "rounds": rounds}
            save()
    print(json.dumps({k: v for k, v in res.items() if k != "bench_alternating"}, indent=1))
    if "bench_alternating" in res:
        print(json.dumps(res["bench_alternating"]))


if __name__ == "__main__":
    main()
