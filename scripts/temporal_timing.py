"""Time temporal reprojection (hala_rt_set_temporal, docs/RENDER_SPEC.md 16), sweep its parameters, and write
profiles/temporal_timing.json.

Timing: configs[3] (atrium) at 1920x1080.  64 samples, capture, one instance moved, refit, 4 samples; then `--calls` resolves back to back,
each timed by the library's own HIP events around k_temporal_resolve (hala_rt_temporal_resolve with gpu_ms); after the sweep, `--calls / 4`
resolves each straight behind an update_batch(4), and `--calls` captures, each between two HIP events on the renderer's stream (the resolve
plus three device-to-device copies).  The 4-spp frame the share is quoted against is
timed the same way (events around update_batch(4), tail joined).

Sweep: tol x max_history on (a) the quality case of tests/test_temporal.py (Cornell box 48 x 36, 64 samples, capture, camera 0 moved,
4 samples) and (b) configs[3] with the moved instance.  One render serves the whole sweep: a resolve reads the accumulation and the history
and writes neither, so hala_rt_set_temporal with new parameters followed by a resolve re-blends the same frame.  Each cell is the mean
squared error in g-space (g(x) = x / (1 + lum(x)), RENDER_SPEC 10) against `--reference` samples of the edited scene, for the temporal
image and for hala_rt_denoise_temporal of it; the 4-sample accumulation and its hala_rt_denoise are the baselines.

With --parent-root, the feature-off bench.py of this tree and of the parent commit's tree (built there) also alternate, `--bench-rounds`
times, each as its own process: bench.py --gpus 1 --steps K --warmup W --no-cpu-baseline --no-secondary."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))  # scene_edits: the base scene of the quality test

import hala_renderer_amd as H  # noqa: E402
import scene_edits as E  # noqa: E402
from hala_renderer_amd import workloads  # noqa: E402

W, HGT, SPP = 1920, 1080, 4
TOLS = (0.002, 0.005, 0.01, 0.02, 0.05, 0.1, 0.2)
HISTORIES = (8.0, 16.0, 32.0, 64.0, 128.0)


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "calls": len(xs)}


def g_space(x):
    x = np.asarray(x[..., :3], np.float64)
    lum = 0.212671 * x[..., 0] + 0.715160 * x[..., 1] + 0.072169 * x[..., 2]
    return x / (1.0 + lum)[..., None]


def translate(t):
    m = np.eye(4, dtype=np.float32)
    m[:3, 3] = t
    return m


def make(cfg, w, h):
    r = H.HalaRenderer("temporal-timing", w, h, cfg["max_depth"], cfg["rr_depth"], False, False, False, 0)
    if cfg["env"] is not None:
        r.set_envmap(cfg["env"], 0.0)
    r.set_scene(cfg["scene"])
    r.commit()
    r.set_launch_timing_period(0)
    r.set_aovs(position=True, ids=True)
    r.set_temporal()
    return r


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


def sweep(r, new_frames, reference_frames):
    """-> the table of one edited frame: r has its history captured, the edit refitted and exactly `new_frames` samples folded"""
    n = int(r.statistics().total_frames)
    if n != new_frames:
        raise RuntimeError(f"the swept frame holds {n} samples, not {new_frames}")
    images = {}
    for tol in TOLS:
        for mh in HISTORIES:
            r.set_temporal(max_history=mh, tol=tol)
            r.temporal_resolve()
            t = r.read_temporal(0)
            r.denoise_temporal()
            images[(tol, mh)] = (t[..., :3].copy(), float((t[..., 3] > new_frames).mean()), r.read_denoised()[..., :3].copy())
    accum = r.read_image(0)
    r.denoise()
    dn = r.read_denoised()
    r.set_temporal()  # the defaults again
    left = reference_frames - new_frames
    while left > 0:
        k = min(left, 16)
        r.update_batch(k); r.render()
        left -= k
    ref = g_space(r.read_image(0))
    mse = lambda x: float(np.mean((g_space(x) - ref) ** 2))  # noqa: E731
    cells = [{"tol": tol, "max_history": mh, "mse_temporal": mse(im[0]), "mse_denoise_temporal": mse(im[2]), "carried": im[1]}
             for (tol, mh), im in images.items()]
    return {"new_samples": new_frames, "reference_samples": reference_frames, "mse_accum": mse(accum), "mse_denoise": mse(dn), "cells": cells}


def moved_instance(r):
    """(node, instance) of the instance that covers the most pixels among those covering less than 15 % of the frame: an object, not a wall"""
    ids = r.read_ids()
    inst = ids[..., 1][ids[..., 1] != 0xFFFFFFFF]
    counts = np.bincount(inst)
    counts[counts > 0.15 * ids.shape[0] * ids.shape[1]] = 0
    k = int(np.argmax(counts))
    node = int(ids[..., 0][ids[..., 1] == k][0])
    return node, k, int(counts[k])


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
    ap.add_argument("--calls", type=int, default=120)
    ap.add_argument("--history", type=int, default=64)
    ap.add_argument("--reference", type=int, default=1024)
    ap.add_argument("--reference-atrium", type=int, default=512)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_timing.json"))
    args = ap.parse_args()
    H.load_library()
    res = {"what": "temporal reprojection (scripts/temporal_timing.py): timing on configs[3] 1920x1080, parameter sweep on the Cornell quality case and on configs[3]",
           "defaults": {k: getattr(H.temporal_default_params(), k) for k in ("max_history", "tol", "min_weight")}}

    def save():  # after every stage: a later one that fails keeps the earlier figures
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)

    # ---- (a) the quality case: Cornell box 48 x 36, camera 0 moved ---------------------------------------------------------------------
    base = E.cornell()  # tests/test_temporal.py quality_case: the same scene, move and sample counts
    cornell = dict(scene=base.scene, env=None, max_depth=base.kw["max_depth"], rr_depth=base.kw["rr_depth"])
    r = make(cornell, base.kw["width"], base.kw["height"])
    node = next(i for i, nd in enumerate(base.scene.nodes) if nd.camera_index == 0)
    r.update_batch(args.history)
    r.temporal_capture()
    r.update_node_transform(node, np.asarray(base.scene.nodes[node].local_transform, np.float32) @ E._translate((0.04 * E._extent(base.scene), 0.0, 0.0)) @ E._rot(ry=0.05))
    r.refit()
    r.update_batch(SPP)
    res["sweep_cornell_camera_move"] = sweep(r, SPP, args.reference)
    r.close()
    save()
    print("cornell sweep done", flush=True)

    # ---- (b) configs[3]: timing and the sweep with a moved instance --------------------------------------------------------------------
    cfg = workloads.baseline_config(3)
    r = make(cfg, W, HGT)
    frame = events(r, lambda: (r.reset_accumulation(), r.update_batch(SPP), r.render()), 12)[2:]
    r.reset_accumulation()
    left = args.history
    while left > 0:
        r.update_batch(min(left, 16)); r.render()
        left -= min(left, 16)
    node, inst, pixels = moved_instance(r)
    r.temporal_capture()
    info = r.bvh_info()
    extent = float(max(b - a for a, b in zip(info.scene_min, info.scene_max)))
    r.update_node_transform(node, np.asarray(cfg["scene"].nodes[node].local_transform, np.float32) @ translate((0.01 * extent, 0.0, 0.005 * extent)))
    t0 = time.perf_counter()
    r.refit()
    r.wait_idle()
    refit_ms = (time.perf_counter() - t0) * 1e3
    r.update_batch(SPP)
    r.temporal_resolve()  # uploads the table
    resolve = [r.temporal_resolve(timed=True) for _ in range(args.calls)]  # back to back: what they read stays in the Infinity Cache
    motion = r.read_temporal(1)
    moved = int((np.abs(motion[..., :2]).max(axis=-1) > 0.05).sum())
    # the sweep next, while the frame still holds exactly SPP new samples (a resolve adds none); it ends on the reference render
    res["sweep_configs3_moved_instance"] = sweep(r, SPP, args.reference_atrium)
    behind = []  # straight behind a frame, whose wavefront buffers have gone through the caches since the last resolve
    for _ in range(args.calls // 4):
        r.update_batch(SPP)
        behind.append(r.temporal_resolve(timed=True))
    res["configs3"] = {"frame": f"{W}x{HGT}", "frame_4spp_gpu_ms": summary(frame), "k_temporal_resolve_gpu_ms": summary(resolve),
                       "moved": {"node": node, "instance": inst, "pixels_before": pixels, "pixels_with_motion": moved, "refit_host_ms": refit_ms},
                       "k_temporal_resolve_behind_a_frame_gpu_ms": summary(behind),
                       "bytes_per_pixel": {"requested_all_taps_valid": 240, "unique_read": 96, "written": 32}}
    for key, name in (("k_temporal_resolve_gpu_ms", "resolve_back_to_back_share_of_frame"), ("k_temporal_resolve_behind_a_frame_gpu_ms", "resolve_behind_a_frame_share_of_frame")):
        res["configs3"][name] = res["configs3"][key]["median"] / res["configs3"]["frame_4spp_gpu_ms"]["median"]
    for key in ("k_temporal_resolve_gpu_ms", "k_temporal_resolve_behind_a_frame_gpu_ms"):  # 96 B of six images read once + 32 B written per pixel
        res["configs3"][key]["GBps_at_128_unique_B_per_pixel"] = 128.0 * W * HGT / (res["configs3"][key]["median"] * 1e6)
    print("resolve:", res["configs3"]["k_temporal_resolve_gpu_ms"], "behind a frame:", res["configs3"]["k_temporal_resolve_behind_a_frame_gpu_ms"],
          "frame:", res["configs3"]["frame_4spp_gpu_ms"], flush=True)
    # capture, last: each one replaces the history (the accumulation keeps running here, which a real host would have restarted)
    capture = events(r, r.temporal_capture, args.calls)
    res["configs3"]["capture_gpu_ms"] = summary(capture)
    res["configs3"]["capture_share_of_frame"] = res["configs3"]["capture_gpu_ms"]["median"] / res["configs3"]["frame_4spp_gpu_ms"]["median"]
    print("capture:", res["configs3"]["capture_gpu_ms"], flush=True)
    r.close()
    save()

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
            print(f"bench.py round {k}: parent {rec['parent']:.4f} ms, this build (feature off) {rec['this']:.4f} ms", flush=True)
        res["bench_feature_off"] = {"cmd": f"bench.py --gpus 1 --steps {args.bench_steps} --warmup {args.bench_warmup} --no-cpu-baseline --no-secondary",
                                    "rounds": runs, "parent": summary([x["parent"] for x in runs]), "this": summary([x["this"] for x in runs])}
    save()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
