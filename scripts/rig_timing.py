"""Time the posing of a character of P primitives (docs/RENDER_SPEC.md 17, 19) and write profiles/rig_timing.json.

configs[1] plus one mesh of P strip primitives of 2 000 vertices each, every one with a deformer of 2 morph targets (position and normal
deltas) and 32 joints.  Per pose, over `--poses` poses, host wall time until the renderer's stream is idle of update_deformer on all P +
refit, for P = 1, 2, 4, 8, 32, 128.  A refit poses its dirty deformers, one or many, with one launch of k_deform behind one copy.  With
`--parent-root` (the parent commit's tree, built there) the two libraries alternate as separate processes, and the order alternates
from round to round.  Also: k_deform alone from one `rocprofv3 --kernel-trace` child run at P = 32, and one shutter run at P = 32 with
time_stride = 1 (every frame poses all 32 and refits) against the parent.

`--morph-only`: the deformers have no skin (joint_count = 0), P = 1 and 2 only, no shutter run and no trace; the rows are added to the
output file under "morph_only_by_count"."""
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

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VERTICES, TARGETS, JOINTS = 2000, 2, 32
COUNTS = (1, 2, 4, 8, 32, 128)


def summary(xs):
    return {"median": statistics.median(xs), "mean": statistics.fmean(xs), "min": min(xs), "max": max(xs), "stdev": statistics.pstdev(xs), "n": len(xs)}


def character(root, count, joints=JOINTS):
    """-> (renderer, mesh index, rigs, poses(k)) of the tree at `root`"""
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import numpy as np

    import deform_ref as D
    import hala_renderer_amd as H
    from hala_renderer_amd import workloads
    from hala_renderer_amd.scene import HalaMesh, HalaNode, HalaPrimitive
    cfg = workloads.baseline_config(1)
    scene = cfg["scene"]
    mesh = len(scene.meshes)
    scene.meshes = list(scene.meshes) + [HalaMesh([HalaPrimitive(*D.strip(VERTICES, seed=k, origin=(0.0, 2.5 * k, 0.0)), material_index=0) for k in range(count)])]
    scene.nodes = list(scene.nodes) + [HalaNode(name="character", mesh_index=mesh)]
    r = H.HalaRenderer("rig-timing", cfg["width"], cfg["height"], cfg["max_depth"], cfg["rr_depth"], False, False, False, 0)
    if cfg.get("env") is not None:
        r.set_envmap(cfg["env"], 0.0)
    r.set_scene(scene)
    r.commit()
    rigs = [D.random_rig(VERTICES, targets=TARGETS, joint_count=joints, normals=True, seed=k) for k in range(count)]
    for k, rig in enumerate(rigs):
        r.set_deformer(mesh, k, **rig)
    return r, mesh, rigs, lambda k, seed: D.random_pose(rigs[k], seed=seed * 1000 + k, zero_some=False, centre=(500.0, 0.5, 0.0)), np


def measure(root, count, poses, joints=JOINTS):
    """update_deformer on all + refit, `poses` times after two warm-up poses -> ms each"""
    r, mesh, rigs, pose, _ = character(root, count, joints)
    out = []
    for n in range(poses + 2):
        ps = [pose(k, n) for k in range(count)]
        r.wait_idle()
        t0 = time.perf_counter()
        for k, p in enumerate(ps):
            r.update_deformer(mesh, k, **p)
        r.refit()
        r.wait_idle()
        out.append((time.perf_counter() - t0) * 1e3)
    status = None
    if hasattr(r, "rig_status"):
        s = r.rig_status()
        status = {"pose_launches": s.pose_launches, "segments_posed": s.segments_posed}
    r.close()
    return {"ms": out[2:], "status": status}


def measure_shutter(root, count, frames):
    """every deformer keyed, time_stride 1: each update poses all `count` and refits before its frame -> ms per update"""
    r, mesh, rigs, pose, _ = character(root, count)
    for k in range(count):
        r.set_deformer_keys(mesh, k, pose(k, 1), pose(k, 2))
    r.set_shutter(0.0, 1.0, 1)
    r.refit()
    out = []
    for n in range(frames + 2):
        r.wait_idle()
        t0 = time.perf_counter()
        r.update()
        r.wait_idle()
        out.append((time.perf_counter() - t0) * 1e3)
    steps = r.shutter_status().steps
    r.close()
    return {"ms": out[2:], "steps": steps}


def run_child(root, *args):
    env = dict(os.environ)
    env.pop("HALART_LIB", None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", os.path.abspath(root), *[str(a) for a in args]], capture_output=True, text=True, timeout=900, env=env)
    if p.returncode != 0:
        raise RuntimeError(f"the child run in {root} failed ({p.returncode}): {p.stderr[-2000:]}")
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def kernel_trace(count, poses):
    """-> the durations (ms) of every k_deform launch of a child run of this build under rocprofv3"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "t", "--", sys.executable, os.path.abspath(__file__), "--root", HERE, "--measure", str(count),
               "--poses", str(poses)]
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--poses", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--morph-only", action="store_true", help="deformers without a skin, P = 1 and 2, added to the output file")
    ap.add_argument("--root", default=None, help="child mode: the tree whose package and library to load")
    ap.add_argument("--measure", type=int, default=0, help="child mode: time this many primitives")
    ap.add_argument("--shutter", type=int, default=0, help="child mode: the shutter run with this many primitives")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "rig_timing.json"))
    args = ap.parse_args()
    if args.root:
        joints = 0 if args.morph_only else JOINTS
        print(json.dumps(measure(args.root, args.measure, args.poses, joints) if args.measure else measure_shutter(args.root, args.shutter, args.poses)))
        return
    sys.path.insert(0, HERE)
    import torch
    res = {"what": f"scripts/rig_timing.py: update_deformer on P primitives of {VERTICES} vertices ({TARGETS} targets with normal deltas + {JOINTS} joints) + refit on "
                   "configs[1]; host wall ms per pose until the stream is idle",
           "box": {"gpu": torch.cuda.get_device_name(0), "host": platform.processor() or platform.machine(), "hip": torch.version.hip}, "by_count": {}}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)

    trees = [("this", HERE)] + ([("parent", args.parent_root)] if args.parent_root else [])
    if args.morph_only:
        if os.path.exists(args.out):
            with open(args.out) as f:
                res = json.load(f)
        res["morph_only_by_count"] = {}
    for count in (1, 2) if args.morph_only else COUNTS:
        runs = {name: [] for name, _ in trees}
        for k in range(args.rounds):
            for name, root in trees[::1 if k % 2 == 0 else -1]:
                got = run_child(root, "--measure", count, "--poses", args.poses, *(["--morph-only"] if args.morph_only else []))
                runs[name].append({"round": k, **summary(got["ms"]), "status": got["status"]})
        res["morph_only_by_count" if args.morph_only else "by_count"][str(count)] = runs
        save()
    if args.morph_only:
        print(json.dumps(res["morph_only_by_count"], indent=1))
        return
    if args.parent_root:
        sh = {name: [] for name, _ in trees}
        for k in range(args.rounds):
            for name, root in trees[::1 if k % 2 == 0 else -1]:
                got = run_child(root, "--shutter", 32, "--poses", args.poses)
                sh[name].append({"round": k, **summary(got["ms"]), "steps": got["steps"]})
        res["shutter_stride_1_at_32_ms_per_update"] = sh
        save()
    if not args.no_trace:
        ms = kernel_trace(32, args.poses)
        bytes_per_pose = 32 * VERTICES * (44 + 44 + TARGETS * 2 * 12 + 24)
        res["k_deform_at_32_ms"] = {**summary(ms), "model_bytes": bytes_per_pose, "gb_per_s_at_median": bytes_per_pose / (statistics.median(ms) * 1e-3) / 1e9}
        save()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
