"""Time the Cryptomatte fold (hala_rt_set_cryptomatte, docs/RENDER_SPEC.md 15) and write profiles/cryptomatte_timing.json.

configs[3] (atrium) at 1920x1080, 4 spp per step (update_batch(4)), untimed updates (the production path: overlapped tails).  Three
renderers of the same scene — Cryptomatte off, one layer (object) and all three layers — alternate `--rounds` times in one process.  A round
times `--steps` steps of one renderer after `--warmup` steps: the host clock around the updates and a synchronise at the end, and two HIP
events on the renderer's stream around the same steps (run()).  The ranked read-back of one layer (hala_rt_read_cryptomatte) is timed on
the host.  --kernel-stats takes the kernel_stats.csv of a `rocprofv3 --kernel-trace --stats` run of `--profile-only` (a few steps of the
three-layer renderer) and quotes k_crypto_fold from it.

With --parent-root, the feature-off bench.py of this tree and of the parent commit's tree (built there) also alternate, `--bench-rounds`
times, each as its own process: bench.py --gpus 1 --steps K --warmup W --no-cpu-baseline --no-secondary.
"""
import argparse
import csv
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
FORMS = {"off": None, "object": ("object",), "all": ("object", "material", "asset")}


def make(cfg, layers):
    r = H.HalaRenderer("cryptomatte-timing", W, HGT, cfg["max_depth"], cfg["rr_depth"], False, False, False, 0)
    if cfg["env"] is not None:
        r.set_envmap(cfg["env"], 0.0)
    r.set_scene(cfg["scene"])
    r.commit()
    r.set_launch_timing_period(0)
    if layers is not None:
        r.set_cryptomatte(layers)
    return r

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
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--no-cpu-baseline", "--no-secondary"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise RuntimeError(f"bench.py in {root} failed ({p.returncode}): {p.stderr[-2000:]}")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    return json.loads(line)["ms_per_step"]


def fold_stats(path):
    """k_crypto_fold's row of a rocprofv3 kernel_stats.csv"""
    with open(path) as f:
        for row in csv.DictReader(f):
            if "k_crypto_fold" in row.get("Name", ""):
                return {k: row[k] for k in ("Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs") if k in row}
    return None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cryptomatte_timing.json"))
    args = ap.parse_args()
    H.load_library()
    cfg = workloads.baseline_config(3)
    if args.profile_only:
        r = make(cfg, FORMS["all"])
        run(r, 8)
        r.close()
        return
    rs = {name: make(cfg, layers) for name, layers in FORMS.items()}
    for r in rs.values():
        run(r, args.warmup)
    rounds = []
    for k in range(args.rounds):  # rotate the order, so that no form always runs on a warmer chip
        order = list(FORMS)[k % 3:] + list(FORMS)[:k % 3]
        rec = {}
        for name in order:
            host, gpu = run(rs[name], args.steps)
            rec[name] = {"host_ms_per_step": host, "gpu_ms_per_step": gpu}
        rounds.append(rec)
        print(f"round {k}: " + ", ".join(f"{n} {rec[n]['gpu_ms_per_step']:.3f}" for n in FORMS) + " ms (GPU)", flush=True)
    r = rs["all"]
    r.read_cryptomatte("object")
    t0 = time.perf_counter()
    for _ in range(5):
        r.read_cryptomatte("object")
    read_ms = (time.perf_counter() - t0) * 1e3 / 5
    res = {"what": "configs[3] 1920x1080, 4 spp per step, Cryptomatte off vs the object layer vs all three layers (scripts/cryptomatte_timing.py)",
           "steps": args.steps, "warmup": args.warmup, "rounds": rounds,
           "read_cryptomatte_host_ms": read_ms}
    for name in FORMS:
        res[name] = {m: summary([x[name][m] for x in rounds]) for m in ("host_ms_per_step", "gpu_ms_per_step")}
    for name in ("object", "all"):
        res[f"{name}_minus_off_ms"] = {m: statistics.median([x[name][m] - x["off"][m] for x in rounds]) for m in ("host_ms_per_step", "gpu_ms_per_step")}
        print(f"{name} - off (median of paired rounds):", res[f"{name}_minus_off_ms"], flush=True)
    for x in rs.values():
        x.close()
    if args.kernel_stats:
        res["k_crypto_fold"] = {"source": "rocprofv3 --kernel-trace --stats of --profile-only (three layers, 8 steps of update_batch(4))",
                                "stats": fold_stats(args.kernel_stats)}
        print("k_crypto_fold:", res["k_crypto_fold"]["stats"], flush=True)
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
            print(f"bench.py round {k}: parent {rec['parent']:.4f} ms, this build (Cryptomatte off) {rec['this']:.4f} ms", flush=True)
        res["bench_feature_off"] = {"cmd": f"bench.py --gpus 1 --steps {args.bench_steps} --warmup {args.bench_warmup} --no-cpu-baseline --no-secondary",
                                    "rounds": runs, "parent": summary([x["parent"] for x in runs]), "this": summary([x["this"] for x in runs])}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
