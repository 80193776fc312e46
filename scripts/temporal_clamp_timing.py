"""Time temporal reprojection with the history clamp (hala_rt_set_temporal_clamp, docs/RENDER_SPEC.md 16 "History clamp") and write
profiles/temporal_clamp_timing.json.

The scenario of scripts/temporal_timing.py: configs[3] (atrium) at 1920x1080, 64 samples, capture, one instance moved, refit, 4 samples.
One block: set the clamp off or to radius 1, 2 or 3 (gamma = 2), then `--calls` resolves back to back, each timed by the library's own
HIP events around k_temporal_resolve.  A session is one process that runs `--blocks` rounds of the four settings in turn; behind them, the
same rounds again for the capture (`--calls / 4` captures per block, each between two HIP events on the renderer's stream: the resolve and
three image copies).

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
# a --session of the parent's library imports the parent's package
PKG_ROOT = os.path.abspath(sys.argv[sys.argv.index("--package-root") + 1]) if "--package-root" in sys.argv[:-1] else ROOT
sys.path.insert(0, PKG_ROOT)

import numpy as np  # noqa: E402

import hala_renderer_amd as H  # noqa: E402
from hala_renderer_amd import workloads  # noqa: E402

W, HGT, SPP, HISTORY = 1920, 1080, 4, 64
SETTINGS = (None, (1, 2.0), (2, 2.0), (3, 2.0))


def summary(xs):
    return {"median": statistics.median(xs), "mean": statistics.fmean(xs), "min": min(xs), "max": max(xs), "stdev": statistics.pstdev(xs), "calls": len(xs)}


def translate(t):
    m = np.eye(4, dtype=np.float32)
    m[:3, 3] = t
    return m


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


def moved_instance(r):
    """(node, instance) of the instance that covers the most pixels among those covering less than 15 % of the frame: an object, not a wall"""
    ids = r.read_ids()
    inst = ids[..., 1][ids[..., 1] != 0xFFFFFFFF]
    counts = np.bincount(inst)
    counts[counts > 0.15 * ids.shape[0] * ids.shape[1]] = 0
    k = int(np.argmax(counts))
    return int(ids[..., 0][ids[..., 1] == k][0]), k


def session(blocks, calls):
    """one process, one renderer -> the blocks' figures"""
    cfg = workloads.baseline_config(3)
    r = H.HalaRenderer("temporal-clamp-timing", W, HGT, cfg["max_depth"], cfg["rr_depth"], False, False, False, 0)
    if cfg["env"] is not None:
        r.set_envmap(cfg["env"], 0.0)
    r.set_scene(cfg["scene"])
    r.commit()
    r.set_launch_timing_period(0)
    r.set_aovs(position=True, ids=True)
    r.set_temporal()
    has_feature = hasattr(r, "set_temporal_clamp")
    left = HISTORY
    while left > 0:
        r.update_batch(min(left, 16)); r.render()
        left -= min(left, 16)
    node, _ = moved_instance(r)
    r.temporal_capture()
    info = r.bvh_info()
    extent = float(max(b - a for a, b in zip(info.scene_min, info.scene_max)))
    r.update_node_transform(node, np.asarray(cfg["scene"].nodes[node].local_transform, np.float32) @ translate((0.01 * extent, 0.0, 0.005 * extent)))
    r.refit()
    r.update_batch(SPP)
    r.temporal_resolve()  # uploads the table
    out = {"clamp_available": has_feature, "blocks": []}

    def setting(k):
        s = SETTINGS[k % len(SETTINGS)] if has_feature else None
        if has_feature:
            r.set_temporal_clamp(*s) if s else r.set_temporal_clamp(enable=False)
        return s

    plain = None
    for k in range(blocks * len(SETTINGS)):
        s = setting(k)
        r.temporal_resolve()
        resolve = [r.temporal_resolve(timed=True) for _ in range(calls)]  # back to back: what they read stays in the Infinity Cache
        t = r.read_temporal(0)
        plain = t if s is None and plain is None else plain
        out["blocks"].append({"clamp": s, "resolve_gpu_ms": summary(resolve), "pixels_with_history": int((t[..., 3] > SPP).sum()),
                              "pixels_the_clamp_changed": int(np.any(t != plain, axis=-1).sum()) if plain is not None else None})
    # the captures last: each one replaces the history (the accumulation keeps running here, which a real host would have restarted)
    for k in range(blocks * len(SETTINGS)):
        s = setting(k)
        capture = events(r, r.temporal_capture, max(calls // 4, 4))
        out["blocks"].append({"clamp": s, "capture_gpu_ms": summary(capture[1:])})
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
    ap.add_argument("--blocks", type=int, default=3, help="rounds of the four settings per session")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--session", action="store_true", help="run one session in this process and print its figures")
    ap.add_argument("--package-root", default=ROOT, help="the tree whose package a --session imports")
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_clamp_timing.json"))
    args = ap.parse_args()
    H.load_library()
    if args.session:
        print(json.dumps(session(args.blocks, args.calls)))
        return
    import torch
    res = {"what": "temporal reprojection with the history clamp (scripts/temporal_clamp_timing.py): configs[3] 1920x1080, 64 samples, capture, "
                   "one instance moved, 4 samples; blocks alternate the clamp off / radius 1 / 2 / 3 (gamma 2) within a session",
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
            print(name, [(b["clamp"], round(b["resolve_gpu_ms"]["median"], 4)) for b in s["blocks"] if "resolve_gpu_ms" in b], flush=True)
            save()

    def medians(build, key):
        out = {}
        for s in res["sessions"]:
            for b in s["blocks"]:
                if s["build"] == build and key in b:
                    out.setdefault("off" if b["clamp"] is None else f"radius_{b['clamp'][0]}", []).append(b[key]["median"])
        return out

    for key in ("resolve_gpu_ms", "capture_gpu_ms"):
        res[key + "_block_medians"] = {"this": medians("this", key), "parent": medians("parent", key)}
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
