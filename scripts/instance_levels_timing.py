"""Time the instance levels of a two-level tree (hala_rt_build_options::instance_levels, docs/RENDER_SPEC.md 4.5) built on the host and on
the GPU, and write profiles/instance_levels_timing.json.

The scene: N instances of one 1 280-triangle blob, rotated, scaled and scattered in a box whose volume grows with N, seen by one camera
from outside; N = 1 024, 16 384 and 131 072 (1.7e8 global triangles, below 2^28).  Every figure is host wall time until the renderer's
stream is idle.  Per N and per variant, each in a process of its own:
  commit        hala_rt_commit (the second of two: the first one also loads the code objects)
  refit_one     hala_rt_refit after hala_rt_update_node_transform on one node
  refit_all     the same after moving every node
  frame         ms per 1920 x 1080 update()
The variants: the host build (instance_levels = 0) of this tree and, with --parent-root (the parent commit's tree, built there), of the
parent's library; the GPU build (instance_levels = 1) with the automatic builder and with SAH, PLOC and LBVH selected.  (`builder` also
selects the builder of the blob's own tree, so a frame time is compared with the host variant of the same builder.)  A host variant gets
a wall-time cap per N (--cap): past it the process is ended and the stages it did not reach are reported as "not finished".

The summary gives, per stage, the smallest N from which the GPU build is the faster one, and the frame time on the GPU-built tree
against the host-built one; the margin for "equal" is the spread of the parent library's repeated host-tree frames."""
import argparse
import json
import os
import platform
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1024, 16384, 131072)
CAPS = {1024: 60.0, 16384: 90.0, 131072: 180.0}
W, HGT = 1920, 1080
STAGES = ("commit", "refit_one", "refit_all", "frame")


def transforms(n):
    """n object -> world matrices: rotation about two axes, a uniform scale of 0.5 ... 1.5, a position in a box of side 3 n^(1/3)"""
    import numpy as np
    rs = np.random.RandomState(77)
    ry, rx = rs.uniform(-np.pi, np.pi, n), rs.uniform(-np.pi, np.pi, n)
    m = np.zeros((n, 4, 4))
    cy, sy, cx, sx = np.cos(ry), np.sin(ry), np.cos(rx), np.sin(rx)
    rot_y = np.zeros((n, 3, 3)); rot_x = np.zeros((n, 3, 3))
    rot_y[:, 0, 0], rot_y[:, 0, 2], rot_y[:, 1, 1], rot_y[:, 2, 0], rot_y[:, 2, 2] = cy, sy, 1.0, -sy, cy
    rot_x[:, 0, 0], rot_x[:, 1, 1], rot_x[:, 1, 2], rot_x[:, 2, 1], rot_x[:, 2, 2] = 1.0, cx, -sx, sx, cx
    m[:, :3, :3] = (rot_y @ rot_x) * rs.uniform(0.5, 1.5, (n, 1, 1))
    m[:, :3, 3] = rs.uniform(-0.5, 0.5, (n, 3)) * (3.0 * n ** (1.0 / 3.0))
    m[:, 3, 3] = 1.0
    return m.astype(np.float32)


def scene_of(H, n):
    from hala_renderer_amd import scenes
    s = H.HalaScene()
    s.materials = [H.HalaMaterial(type=0, base_color=(0.8, 0.6, 0.4))]
    blob = scenes.blob_mesh(3, 1234)
    blob.material_index = 0
    s.meshes = [H.HalaMesh([blob])]
    s.nodes = [H.HalaNode(name=f"i{k}", mesh_index=0, local_transform=m) for k, m in enumerate(transforms(n))]
    d = 3.0 * n ** (1.0 / 3.0)
    s.nodes.append(H.HalaNode(name="camera", camera_index=0, local_transform=scenes.look_at_node_transform((0.4 * d, 0.5 * d, 1.4 * d), (0.0, 0.0, 0.0))))
    s.cameras = [H.HalaPerspectiveCamera(aspect=W / HGT, yfov=0.7, znear=0.1)]
    return s


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "calls": len(v)}


def session(n, levels, builder, frames):
    """one variant in this process; a JSON line per finished stage"""
    import numpy as np
    sys.path.insert(0, os.getcwd())
    import hala_renderer_amd as H
    H.load_library()

    def say(stage, value):
        print(json.dumps({"stage": stage, "ms": value}), flush=True)

    def timed(r, fn):
        r.wait_idle()
        t0 = time.perf_counter()
        fn()
        r.wait_idle()
        return (time.perf_counter() - t0) * 1e3

    s = scene_of(H, n)
    r = H.HalaRenderer("levels", W, HGT, 5, 3, False, False, False, 0)
    options = dict(instancing=True, builder=builder)
    if levels == "gpu":
        options["instance_levels"] = "gpu"  # (the parent's set_build_options has no such argument: its sessions are host ones)
    r.set_build_options(**options)
    r.set_scene(s)
    first = timed(r, r.commit)
    say("first_commit", first)
    say("commit", timed(r, r.commit))
    i = r.bvh_info()
    print(json.dumps({"stage": "tree", "instance_nodes": i.instance_node_count, "instance_refs": i.instance_ref_count, "max_depth": i.max_depth}), flush=True)
    step = np.float32(0.25)

    def move(k):
        m = np.array(s.nodes[k].local_transform, dtype=np.float32)
        m[0, 3] += step
        s.nodes[k].local_transform = m
        r.update_node_transform(k, m)

    one = []
    for k in range(5):
        move((k * 7919) % n)
        one.append(timed(r, r.refit))
    say("refit_one", summary(one))
    every = []
    for _ in range(3):
        for k in range(n):
            move(k)
        every.append(timed(r, r.refit))
    say("refit_all", summary(every))
    for _ in range(2):
        r.update()
    per_frame = []
    for _ in range(3):
        per_frame.append(timed(r, lambda: [r.update() for _ in range(frames)]) / frames)
    say("frame", summary(per_frame))
    r.close()


def run_session(root, n, levels, builder, frames, cap):
    """-> {stage: figure | "not finished"}, wall seconds"""
    env = dict(os.environ)
    env.pop("HALART_LIB", None)
    root = os.path.abspath(root)
    cmd = [sys.executable, os.path.abspath(__file__), "--session", "--n", str(n), "--levels", levels, "--builder", builder or "auto", "--frames", str(frames)]
    t0 = time.perf_counter()
    p = subprocess.Popen(cmd, cwd=root, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    try:
        out, err = p.communicate(timeout=cap)
        capped = False
    except subprocess.TimeoutExpired:
        p.kill()
        out, err = p.communicate()
        capped = True
    wall = time.perf_counter() - t0
    if not capped and p.returncode != 0:
        raise RuntimeError(f"the session {cmd[3:]} in {root} failed ({p.returncode}): {err[-2000:]}")
    res = {}
    for ln in out.splitlines():
        if ln.startswith("{"):
            d = json.loads(ln)
            res[d.pop("stage")] = d.get("ms", d)
    for st in STAGES:
        res.setdefault(st, "not finished")
    res["capped_after_s"] = cap if capped else None
    return res, wall


def med(x):
    return x if isinstance(x, (int, float)) else (x["median"] if isinstance(x, dict) else None)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--cap", type=float, default=None, help="wall seconds a host variant may take per N (default: 60 / 90 / 180 by size)")
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--parent-rounds", type=int, default=3, help="sessions of the parent's library per N (their frame times give the margin)")
    ap.add_argument("--session", action="store_true", help="one variant in this process")
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--levels", default="host")
    ap.add_argument("--builder", default="auto")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "instance_levels_timing.json"))
    args = ap.parse_args()
    if args.session:
        session(args.n, args.levels, None if args.builder == "auto" else args.builder, args.frames)
        return
    import torch
    res = {"what": "instance levels built on the host and on the GPU (scripts/instance_levels_timing.py): N instances of a 1 280-triangle blob; host wall ms "
                   f"until the stream is idle; frames at {W} x {HGT}",
           "box": {"gpu": torch.cuda.get_device_name(0), "host": platform.processor() or platform.machine(), "hip": torch.version.hip}, "sizes": {}}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)

    for n in args.sizes:
        cap = args.cap or CAPS.get(n, 240.0)
        rows = res["sizes"].setdefault(str(n), {})
        variants = [("gpu", None), ("gpu", "sah"), ("gpu", "ploc"), ("gpu", "lbvh"), ("host", None), ("host", "sah"), ("host", "ploc"), ("host", "lbvh")]
        for levels, builder in variants:
            name = f"{levels}/{builder or 'auto'}"
            if levels == "host" and builder and rows.get("host/auto", {}).get("capped_after_s"):
                continue  # the host build does not depend on the builder: it would run into the cap again
            rows[name], wall = run_session(ROOT, n, levels, builder, args.frames, cap if levels == "host" else 900.0)
            print(f"N={n} {name}: {wall:.1f} s " + " ".join(f"{st}={med(rows[name][st]) if med(rows[name][st]) is not None else 'not finished'}" for st in STAGES), flush=True)
            save()
        if args.parent_root:
            rows["parent host/auto"] = []
            for k in range(args.parent_rounds):
                one, wall = run_session(args.parent_root, n, "host", None, args.frames, cap)
                rows["parent host/auto"].append(one)
                print(f"N={n} parent host/auto #{k}: {wall:.1f} s " + " ".join(f"{st}={med(one[st]) if med(one[st]) is not None else 'not finished'}" for st in STAGES), flush=True)
                save()
                if one["capped_after_s"]:
                    break
    # from which N the GPU build wins each stage (automatic builder), and the frame on its tree against the host-built one
    out = {"gpu_wins_from_n": {}, "frame_ms": {}}
    for st in ("commit", "refit_one", "refit_all"):
        wins = []
        for n in args.sizes:
            g, h = med(res["sizes"][str(n)]["gpu/auto"][st]), med(res["sizes"][str(n)]["host/auto"][st])
            wins.append(g is not None and (h is None or g < h))
        from_n = next((n for k, n in enumerate(args.sizes) if all(wins[k:])), None)
        out["gpu_wins_from_n"][st] = from_n
    for n in args.sizes:
        rows = res["sizes"][str(n)]
        parent = [med(x["frame"]) for x in rows.get("parent host/auto", []) if med(x["frame"]) is not None]
        out["frame_ms"][str(n)] = {name: med(v["frame"]) for name, v in rows.items() if isinstance(v, dict)}
        out["frame_ms"][str(n)]["parent host/auto runs"] = parent
        out["frame_ms"][str(n)]["margin (spread of the parent's runs)"] = max(parent) - min(parent) if len(parent) > 1 else None
    res["summary"] = out
    save()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
