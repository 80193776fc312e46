"""Time the tree cost and the refit policy (docs/RENDER_SPEC.md 4.6) and write profiles/tree_quality_timing.json.

The scene is configs[3]'s atrium (1 000 210 triangles, one tree; --textures attaches its 18 textures, off by default: they add the same
shading time to every frame figure and nothing to a refit).  Its largest primitive (the 120 050-triangle floor) carries one morph
target of tests/deform_ref.py's random rig, scaled to the primitive's extent; a pose is one morph weight.
  cost     k_tree_cost alone on the committed tree: the time between two events on the renderer's stream around the call that measures
           (a 24-B clear, the kernel, a 24-B copy back) and the host wall time of that call; bytes/s = 64 B x nodes / event time.  The
           kernel's sums are checked against the numpy twin on the downloaded nodes.
  refit    hala_rt_refit after a small pose change with the policy off (mode 0) and measuring (mode 3): host wall ms until the stream is
           idle, median of --reps calls after a warm-up call.  With --parent-root (the parent commit's tree, built there) the mode-0
           figure also runs on the parent's library, --parent-rounds sessions each; the spread of the parent's sessions is the margin.
  curve    per pose of growing weight, from a tree built at the rest pose: the inflation the refit measures, ms per 1920 x 1080 frame on
           the refitted tree, the same after a rebuild (mode 2), and what the rebuild added to the refit."""
import argparse
import json
import os
import platform
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, HGT = 1920, 1080
WEIGHTS = [0.0, 0.01, 0.03, 0.1, 0.3, 1.0]


def session(what, reps, frames, textures):
    """one library in this process; a JSON line per result"""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.getcwd())
    import deform_ref as D
    import hala_renderer_amd as H
    from hala_renderer_amd import workloads
    med = statistics.median

    def say(name, **kw):
        print(json.dumps(dict(result=name, **kw)), flush=True)

    s, env = workloads.atrium(aspect=W / HGT, textures=textures)
    _, mesh, prim = max((len(p.vertices), mi, pi) for mi, m in enumerate(s.meshes) for pi, p in enumerate(m.primitives))
    rest = s.meshes[mesh].primitives[prim].vertices
    extent = float((rest["position"].max(axis=0) - rest["position"].min(axis=0)).max())
    rig = D.random_rig(len(rest), targets=1, seed=11, scale=extent)  # deltas of about 0.3 extents at weight 1
    r = H.HalaRenderer("quality", W, HGT, workloads.MAX_DEPTH, workloads.RR_DEPTH, False, False, False, 0)
    r.set_envmap(env, 0.0)
    r.set_scene(s)
    r.commit()
    r.set_deformer(mesh, prim, **rig)
    r.refit()
    has_policy = hasattr(r, "set_refit_policy")

    def timed(fn):
        r.wait_idle()
        t0 = time.perf_counter()
        fn()
        r.wait_idle()
        return (time.perf_counter() - t0) * 1e3

    def pose(w):
        r.update_deformer(mesh, prim, morph_weights=np.array([w], dtype=np.float32))

    def frame_ms():
        r.update()  # warm-up: the first frame after a refit also restarts what the refit invalidated
        return timed(lambda: [r.update() for _ in range(frames)]) / frames

    def refit_ms(small):
        """refits after small pose changes around weight `small`"""
        t = []
        for k in range(reps + 1):
            pose(small * (1.0 + 0.125 * (k % 3)))
            t.append(timed(r.refit))
        return t[1:]

    if "refit0" in what:
        t = refit_ms(0.01)
        say("refit mode 0", ms=med(t), all=t)
    if not has_policy:
        r.close()
        return
    if "cost" in what:
        import torch
        from tree_quality_ref import tree_cost
        ext = torch.cuda.ExternalStream(r.get_stream())
        ev, wall = [], []
        for _ in range(reps + 1):
            r.set_refit_policy(0)
            r.wait_idle()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record(ext)
            r.set_refit_policy(3)  # measures the committed tree at once
            b.record(ext)
            b.synchronize()
            wall.append((time.perf_counter() - t0) * 1e6)
            ev.append(a.elapsed_time(b) * 1e3)
        (t,), _, _ = r.tree_quality()
        nodes = r.download_bvh()[0].reshape(-1, 16)
        want = tree_cost(nodes, (t.first_node, t.node_count))
        us = med(ev[1:])
        say("cost", nodes=t.node_count, bytes=64 * t.node_count, event_us=us, event_us_all=ev[1:], wall_us=med(wall[1:]), bytes_per_s=64 * t.node_count / (us * 1e-6),
            equals_twin=(t.valid, t.node_q_now, t.tri_q_now) == want, node_q=t.node_q_now, tri_q=t.tri_q_now)
    if "refit3" in what:
        r.set_refit_policy(0)
        t0 = refit_ms(0.01)
        r.set_refit_policy(3)
        t3 = refit_ms(0.01)
        say("refit mode 0 and 3, one session", mode0_ms=med(t0), mode3_ms=med(t3), mode0_all=t0, mode3_all=t3)
    if "curve" in what:
        rows = []
        for w in WEIGHTS:
            r.set_refit_policy(2)
            pose(0.0)
            r.refit()  # built at the rest pose
            r.set_refit_policy(3)
            pose(w)
            t_refit = timed(r.refit)
            (t,), _, _ = r.tree_quality()
            inflation = (t.node_q_now + t.tri_q_now) / (t.node_q_built + t.tri_q_built)
            f_refit = frame_ms()
            r.set_refit_policy(2)
            pose(w)
            t_rebuild = timed(r.refit)
            (t,), _, rebuilt = r.tree_quality()
            assert t.rebuilt_last_refit == 1
            f_rebuilt = frame_ms()
            gain = f_refit - f_rebuilt
            rows.append(dict(weight=w, inflation=inflation, refit_ms=t_refit, frame_ms_refitted=f_refit, frame_ms_rebuilt=f_rebuilt,
                             refit_and_rebuild_ms=t_rebuild, rebuild_ms=t_rebuild - t_refit,
                             frames_to_repay=(t_rebuild - t_refit) / gain if gain > 0 else None, cost_built=t.node_q_built + t.tri_q_built))
            say("curve row", **rows[-1])
    r.close()


def run_session(root, what, reps, frames, textures, cap):
    env = dict(os.environ)
    env.pop("HALART_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--session", "--what", what, "--reps", str(reps), "--frames", str(frames)] + (["--textures"] if textures else [])
    p = subprocess.run(cmd, cwd=os.path.abspath(root), env=env, capture_output=True, text=True, timeout=cap)  # (a session that is capped ends the script)
    if p.returncode != 0:
        raise RuntimeError(f"the session {what} in {root} failed ({p.returncode}): {p.stderr[-2000:]}")
    return [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--textures", action="store_true")
    ap.add_argument("--cap", type=float, default=300.0, help="wall seconds one session may take")
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--parent-rounds", type=int, default=3)
    ap.add_argument("--session", action="store_true", help="one library in this process")
    ap.add_argument("--what", default="cost,refit0,refit3,curve")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_quality_timing.json"))
    args = ap.parse_args()
    if args.session:
        session(args.what.split(","), args.reps, args.frames, args.textures)
        return
    import torch
    res = {"what": "tree cost and refit policy on configs[3]'s atrium (scripts/tree_quality_timing.py): k_tree_cost alone, hala_rt_refit with the policy off "
                   "and measuring, and the degradation curve of the 120 050-triangle floor posed by one morph target; textures " + ("on" if args.textures else "off"),
           "box": {"gpu": torch.cuda.get_device_name(0), "host": platform.processor() or platform.machine(), "hip": torch.version.hip}}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)

    rows = run_session(ROOT, args.what, args.reps, args.frames, args.textures, args.cap)
    res["session"] = [x for x in rows if x.get("result") != "curve row"]
    res["curve"] = [{k: v for k, v in x.items() if k != "result"} for x in rows if x.get("result") == "curve row"]
    save()
    mode0 = [x["ms"] for x in rows if x.get("result") == "refit mode 0"]
    for k in range(1, args.parent_rounds if args.parent_root else 1):
        mode0 += [x["ms"] for x in run_session(ROOT, "refit0", args.reps, args.frames, args.textures, args.cap) if "ms" in x]
    parent = []
    for k in range(args.parent_rounds if args.parent_root else 0):
        parent += [x["ms"] for x in run_session(args.parent_root, "refit0", args.reps, args.frames, args.textures, args.cap) if "ms" in x]
    summary = {"refit mode 0 ms, per session": mode0, "parent refit ms, per session": parent}
    if len(parent) > 1 and mode0:
        spread = max(parent) - min(parent)
        summary["margin (spread of the parent's sessions)"] = spread
        summary["mode 0 equals the parent within the margin"] = min(parent) - spread <= statistics.median(mode0) <= max(parent) + spread
    both = [x for x in rows if x.get("result") == "refit mode 0 and 3, one session"]
    if both:
        summary["measuring costs, ms per refit (mode 3 - mode 0, one session)"] = both[0]["mode3_ms"] - both[0]["mode0_ms"]
    res["summary"] = summary
    save()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
