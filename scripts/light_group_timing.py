"""Time the light groups (hala_rt_set_light_groups, docs/RENDER_SPEC.md 14) and the relight, and write profiles/light_group_timing.json.

configs[3] (atrium) at 1920x1080, 4 spp per step (update_batch(4)), untimed updates (the production path: overlapped tails).  Two
renderers of the same scene, one with four light groups (quad light 0, quad light 1, the environment, all materials) and one with the
feature off, alternate `--rounds` times in one process.  A round times `--steps` steps of one renderer after `--warmup` steps: the host
clock around the updates and a synchronise at the end, and two HIP events on the renderer's stream around the same steps (run()).
hala_rt_relight of the 1080p frame is timed with HIP events around `--relights` calls.

With --parent-root, the feature-off bench.py of this tree and of the parent commit's tree (built there) also alternate, `--bench-rounds`
times, each as its own process: bench.py --gpus 1 --steps K --warmup W.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import hala_renderer_amd as H  # noqa: E402
from hala_renderer_amd import workloads  # noqa: E402

W, HGT, SPP = 1920, 1080, 4


def make(cfg, groups):
    r = H.HalaRenderer("light-group-timing", W, HGT, cfg["max_depth"], cfg["rr_depth"], False, False, False, 0)
    if cfg["env"] is not None:
        r.set_envmap(cfg["env"], 0.0)
    r.set_scene(cfg["scene"])
    r.commit()
    r.set_launch_timing_period(0)
    if groups:
        n = len(r.packed_lights()[0])
        r.set_light_groups(lights=[min(k, 1) for k in range(n)], environment=2, materials=3)
    return r


def time_relight(r, calls):
    """GPU ms per hala_rt_relight call: HIP events on the renderer's stream around `calls` relights of the accumulated frame (the
    calls are stream-ordered; read-back is not timed)"""
    import ctypes as C
    import torch
    scales = (C.c_float * 12)(1.0, 0.9, 0.8, 0.5, 0.5, 1.0, 2.0, 2.0, 2.0, 1.0, 1.0, 0.0)
    relight = lambda: r._check(r._lib.hala_rt_relight(r._h, C.c_uint32(0), scales, C.c_uint32(4)))  # noqa: E731
    relight()
    r.wait_idle()
    stream = torch.cuda.ExternalStream(r.stream_handle())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(calls):
        relight()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def run(r, steps):
    """(host ms per step, GPU ms per step).  The GPU figure is a pair of HIP events on the renderer's stream around all the steps: the
    end event follows the last update's tail, which stream_handle() joins into that stream.  (The updates' own frame_begin -> frame_end
    spans overlap with two updates in flight and do not add up to the frame time.)"""
    import torch
    r.wait_idle()
    stream = torch.cuda.ExternalStream(r.stream_handle())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record(stream)
    for _ in range(steps):
        r.update_batch(SPP)
        r.render()
    stream = torch.cuda.ExternalStream(r.stream_handle())  # joins the second frame slot
    e1.record(stream)
    e1.synchronize()
    host = 1e3 * (time.perf_counter() - t0) / steps
    return host, e0.elapsed_time(e1) / steps


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def bench(root, steps, warmup):
    env = dict(os.environ)
    env.pop("HALART_LIB", None)
    root = os.path.abspath(root)
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                       cwd=root, env=env, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise RuntimeError(f"bench.py in {root} failed ({p.returncode}): {p.stderr[-2000:]}")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    return json.loads(line)["ms_per_step"]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=5)
    ap.add_argument("--relights", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "light_group_timing.json"))
    args = ap.parse_args()
    H.load_library()
    cfg = workloads.baseline_config(3)
    rs = {"off": make(cfg, False), "on": make(cfg, True)}
    for r in rs.values():
        run(r, args.warmup)
    rounds = []
    for k in range(args.rounds):  # alternate the order, so that neither form always runs on a warmer chip
        order = ["off", "on"] if k % 2 == 0 else ["on", "off"]
        rec = {}
        for name in order:
            host, gpu = run(rs[name], args.steps)
            rec[name] = {"host_ms_per_step": host, "gpu_ms_per_step": gpu}
        rounds.append(rec)
        print(f"round {k}: off {rec['off']['host_ms_per_step']:.3f} / {rec['off']['gpu_ms_per_step']:.3f} ms, "
              f"on {rec['on']['host_ms_per_step']:.3f} / {rec['on']['gpu_ms_per_step']:.3f} ms (host / GPU)", flush=True)
    relight_ms = [time_relight(rs["on"], args.relights) for _ in range(3)]
    print("hala_rt_relight, 1920x1080, 4 groups: " + ", ".join(f"{x * 1e3:.1f} us" for x in relight_ms), flush=True)
    res = {"what": "configs[3] 1920x1080, 4 spp per step, light groups off vs on (G = 4: quad light 0, quad light 1, environment, "
                   "all materials; scripts/light_group_timing.py)", "steps": args.steps,
           "warmup": args.warmup, "rounds": rounds}
    for name in ("off", "on"):
        res[name] = {m: summary([r[name][m] for r in rounds]) for m in ("host_ms_per_step", "gpu_ms_per_step")}
    res["on_minus_off_ms"] = {m: statistics.median([r["on"][m] - r["off"][m] for r in rounds]) for m in ("host_ms_per_step", "gpu_ms_per_step")}
    res["relight_gpu_ms"] = {"calls_per_sample": args.relights, "samples": relight_ms, **summary(relight_ms)}
    for r in rs.values():
        r.close()
    print("light groups on - off (median of paired rounds):", res["on_minus_off_ms"], flush=True)
    if args.parent_root:
        runs = []
        for k in range(args.bench_rounds):
            order = [("parent", args.parent_root), ("this", ROOT)]
            if k % 2:
                order.reverse()
            rec = {}
            for name, root in order:
                rec[name] = bench(root, args.bench_steps, args.bench_warmup)
            runs.append(rec)
            print(f"bench.py round {k}: parent {rec['parent']:.4f} ms, this build (light groups off) {rec['this']:.4f} ms", flush=True)
        res["bench_feature_off"] = {"cmd": f"bench.py --gpus 1 --steps {args.bench_steps} --warmup {args.bench_warmup}", "rounds": runs,
                                    "parent": summary([r["parent"] for r in runs]), "this": summary([r["this"] for r in runs])}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
