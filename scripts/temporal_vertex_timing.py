"""Time temporal reprojection with vertex motion (hala_rt_set_temporal_vertex_motion, docs/RENDER_SPEC.md 16 "Vertex motion") and write
profiles/temporal_vertex_timing.json.

configs[3] (atrium) at 1920x1080, one-level tree, its largest primitive under the rig of scripts/deform_timing.py (2 morph targets + 32
joints).  One block: set the feature off or on, 16 samples, `--calls / 4` captures (each between two HIP events on the renderer's stream:
the resolve, three image copies and, with the feature on, the copy of the triangles), the next pose, refit, 4 samples, then `--calls`
resolves back to back, each timed by the library's own HIP events around k_temporal_resolve.  A session is one process that runs `--blocks`
blocks, off and on alternating; with the feature off the posed primitive's pixels start without history (the kernel instantiation without
the vertex branch), with it on they take the vertex branch.

With --parent-root (the parent commit's tree, built there) a session of the parent's library, which has no such entry point and runs every
block "off", alternates with this build's, `--rounds` times; the parent's spread over its own blocks and sessions is the margin for "off
costs nothing".  bench.py of both trees then alternates as well, `--bench-rounds` times, each as its own process:
bench.py --gpus 1 --steps K --warmup W --no-cpu-baseline --no-secondary."""
import argparse
import json
import os
import platform
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# a --session of the parent's library imports the parent's package and twin
PKG_ROOT = os.path.abspath(sys.argv[sys.argv.index("--package-root") + 1]) if "--package-root" in sys.argv[:-1] else ROOT
sys.path.insert(0, PKG_ROOT)
sys.path.insert(0, os.path.join(PKG_ROOT, "tests"))  # deform_ref: the rig and the poses

import numpy as np  # noqa: E402

import deform_ref as D  # noqa: E402
import hala_renderer_amd as H  # noqa: E402
from hala_renderer_amd import workloads  # noqa: E402

W, HGT, SPP = 1920, 1080, 4
TARGETS, JOINTS = 2, 32


def summary(xs):
    return {"median": statistics.median(xs), "mean": statistics.fmean(xs), "min": min(xs), "max": max(xs), "stdev": statistics.pstdev(xs), "calls": len(xs)}


def events(r, fn, calls):
    """GPU ms of each of `calls` calls of fn(), between two HIP events on the renderer's stream (stream_handle() joins the second frame slot)"""
    import torch
    out = []
    for _ in range(calls):
        stream = torch.cuda.ExternalStream(r.stream_handle())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        stream = torch.cuda.ExternalStream(r.stream_handle())
        e1.record(stream)
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def session(blocks, calls):
    """one process, one renderer -> the blocks' figures"""
    cfg = workloads.baseline_config(3)
    scene = cfg["scene"]
    mesh, prim = max(((m, p) for m in range(len(scene.meshes)) for p in range(len(scene.meshes[m].primitives))),
                     key=lambda mp: len(scene.meshes[mp[0]].primitives[mp[1]].vertices))
    rest = scene.meshes[mesh].primitives[prim].vertices
    r = H.HalaRenderer("temporal-vertex-timing", W, HGT, cfg["max_depth"], cfg["rr_depth"], False, False, False, 0)
    r.set_build_options(instancing=False)
    if cfg["env"] is not None:
        r.set_envmap(cfg["env"], 0.0)
    r.set_scene(scene)
    r.commit()
    r.set_launch_timing_period(0)
    r.set_aovs(position=True, ids=True)
    r.set_temporal()
    has_feature = hasattr(r, "set_temporal_vertex_motion")
    pos = rest["position"].astype(np.float64)
    extent = float(np.ptp(pos, axis=0).max())
    centre = 0.5 * (pos.min(0) + pos.max(0))
    rig = D.random_rig(len(rest), targets=TARGETS, joint_count=JOINTS, normals=True, seed=17, scale=0.02 * extent)
    r.set_deformer(mesh, prim, **rig)
    out = {"vertex_motion_available": has_feature, "triangles": int(r.bvh_info().triangle_count), "deformed_vertices": len(rest), "blocks": []}
    r.update_deformer(mesh, prim, **D.random_pose(rig, seed=0, zero_some=False, centre=centre, scale=0.05 * extent))
    r.refit()
    for k in range(blocks):
        on = has_feature and k % 2 == 1
        if has_feature:
            r.set_temporal_vertex_motion(on)
        for _ in range(4):
            r.update_batch(SPP); r.render()
        capture = events(r, r.temporal_capture, max(calls // 4, 4))
        r.update_deformer(mesh, prim, **D.random_pose(rig, seed=k + 1, zero_some=False, centre=centre, scale=0.05 * extent))
        r.refit()
        r.update_batch(SPP)
        r.temporal_resolve()  # uploads the table
        resolve = [r.temporal_resolve(timed=True) for _ in range(calls)]
        t, m = r.read_temporal(0), r.read_temporal(1)
        out["blocks"].append({"vertex_motion": on, "resolve_gpu_ms": summary(resolve), "capture_gpu_ms": summary(capture[1:]),
                              "pixels_with_history": int((t[..., 3] > SPP).sum()), "pixels_with_motion": int((np.abs(m[..., :2]).max(axis=-1) > 0.05).sum())})
    r.close()
    return out


def run_session(root, blocks, calls):
    env = dict(os.environ)
    env.pop("HALART_LIB", None)
    root = os.path.abspath(root)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--session", "--blocks", str(blocks), "--calls", str(calls), "--package-root", root],
                       cwd=root, env=env, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise RuntimeError(f"the session in {root} failed ({p.returncode}): {p.stderr[-2000:]}")
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


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
    ap.add_argument("--calls", type=int, default=80)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--session", action="store_true", help="run one session in this process and print its figures")
    ap.add_argument("--package-root", default=ROOT, help="the tree whose package a --session imports")
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_vertex_timing.json"))
    args = ap.parse_args()
    H.load_library()
    if args.session:
        print(json.dumps(session(args.blocks, args.calls)))
        return
    import torch
    res = {"what": "temporal reprojection with vertex motion (scripts/temporal_vertex_timing.py): configs[3] 1920x1080, the largest primitive "
                   f"posed by {TARGETS} morph targets + {JOINTS} joints; blocks alternate the feature off / on within a session",
           "box": {"gpu": torch.cuda.get_device_name(0), "host": platform.processor() or platform.machine(), "hip": torch.version.hip},
           "sessions": []}

    def save():  # after every stage: a later one that fails keeps the earlier figures
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)

    for k in range(args.rounds):
        order = [("parent", args.parent_root), ("this", ROOT)] if args.parent_root else [("this", ROOT)]
        if k % 2:
            order.reverse()
        for name, root in order:
            s = run_session(root, args.blocks, args.calls)
            s["build"] = name
            res["sessions"].append(s)
            print(name, [(b["vertex_motion"], round(b["resolve_gpu_ms"]["median"], 4), round(b["capture_gpu_ms"]["median"], 4)) for b in s["blocks"]], flush=True)
            save()

    def medians(build, on, key):
        return [b[key]["median"] for s in res["sessions"] if s["build"] == build for b in s["blocks"] if b["vertex_motion"] == on]

    res["resolve_gpu_ms_block_medians"] = {"this_off": medians("this", False, "resolve_gpu_ms"), "this_on": medians("this", True, "resolve_gpu_ms"),
                                           "parent": medians("parent", False, "resolve_gpu_ms")}
    res["capture_gpu_ms_block_medians"] = {"this_off": medians("this", False, "capture_gpu_ms"), "this_on": medians("this", True, "capture_gpu_ms"),
                                           "parent": medians("parent", False, "capture_gpu_ms")}
    save()
    if args.parent_root:
        rounds = []
        for k in range(args.bench_rounds):  # the order within a round alternates too: whichever runs second finds the GPU warmer
            order = (("parent", args.parent_root), ("this", ROOT))[::1 if k % 2 == 0 else -1]
            ms = {name: bench(root, args.bench_steps, args.bench_warmup) for name, root in order}
            rounds.append({"order": [name for name, _ in order], "parent_ms_per_step": ms["parent"], "this_ms_per_step": ms["this"]})
            res["bench_alternating"] = {"command": f"bench.py --gpus 1 --steps {args.bench_steps} --warmup {args.bench_warmup} --no-cpu-baseline --no-secondary", "rounds": rounds}
            print("bench.py round", k, rounds[-1], flush=True)
            save()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
