"""Time adaptive sampling (hala_rt_set_adaptive_sampling, docs/RENDER_SPEC.md 11) on configs[1] (Cornell box) and configs[3] (atrium)
at 1920x1080 and write profiles/adaptive_timing.json.

Every update is bracketed by two HIP events recorded on the renderer's stream (torch.cuda.ExternalStream) and synchronised, so a
frame's time includes everything it enqueues: the wavefront kernels and, on a check frame, k_adaptive_check, k_adaptive_compact and
the readback of the two counts.

  per_fraction : ms per update against the fraction of pixels still traced (non-check frames, grouped by the active set)
  check_ms     : check + compaction + readback = a check frame minus the frame before it (same active set), averaged
  equal_time   : uniform rendering for `--budget-spp` frames against adaptive rendering for the same GPU time, per threshold, as MSE of
                 accum.rgb against a `--ref-spp` render
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import hala_renderer_amd as H  # noqa: E402
from hala_renderer_amd import workloads  # noqa: E402


class Timer:
    def __init__(self, r):
        import torch
        self.torch = torch
        self.stream = torch.cuda.ExternalStream(r.stream_handle())

    def __call__(self, fn):
        t = self.torch
        a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        a.record(self.stream)
        fn()
        b.record(self.stream)
        b.synchronize()
        return a.elapsed_time(b)


def accum(r):
    r.wait_idle()
    return r.read_image(0)[..., :3].astype(np.float64)


def mse(x, ref):
    return float(np.mean((x - ref) ** 2))


def run_config(index, args):
    cfg = workloads.baseline_config(index)
    w, h = cfg["width"], cfg["height"]
    r = H.HalaRenderer("adaptive_timing", w, h, cfg["max_depth"], cfg["rr_depth"], False, False, False, 0)
    if cfg["env"] is not None:
        r.set_envmap(cfg["env"], 0.0)
    r.set_scene(cfg["scene"])
    r.commit()
    timer = Timer(r)
    d = H.adaptive_default_params()
    out = {"workload": cfg["name"], "width": w, "height": h, "min_samples": d.min_samples, "interval": d.interval}

    # reference
    r.set_adaptive_sampling(None)
    left = args.ref_spp
    while left:
        k = min(left, 16)
        r.update_batch(k)
        left -= k
    ref = accum(r)

    # uniform: the budget
    r.reset_accumulation()
    for _ in range(3):
        r.update()
    r.reset_accumulation()
    uni = [timer(r.update) for _ in range(args.budget_spp)]
    budget = float(sum(uni))
    out["uniform"] = {"spp": args.budget_spp, "gpu_ms": round(budget, 3), "ms_per_update_median": round(float(np.median(uni)), 4),
                      "mse": mse(accum(r), ref)}

    per_fraction = {}
    check_cost = []
    runs = []
    for thr in args.thresholds:
        r.set_adaptive_sampling(thr)
        spent, frames, last, checks = 0.0, 0, None, 0
        while True:
            st = r.adaptive_status()
            frac = st.active_pixels / (w * h)
            if last is not None and spent + last > budget:
                break
            is_check = (frames + 1) >= d.min_samples and ((frames + 1) - d.min_samples) % d.interval == 0
            ms = timer(r.update)
            frames += 1
            spent += ms
            if is_check:  # the frame before it rendered the same active set
                checks += 1
                if last is not None:
                    check_cost.append(ms - last)
            else:
                per_fraction.setdefault(round(frac, 4), []).append(ms)
                last = ms
            if frames >= args.max_frames:
                break
        st = r.adaptive_status()
        runs.append({"threshold": thr, "frames": frames, "checks": checks, "gpu_ms": round(spent, 3),
                     "final_active_fraction": round(st.active_pixels / (w * h), 4), "mean_samples_per_pixel": round(float(r.read_sample_counts().mean()), 2),
                     "mse": mse(accum(r), ref)})
        runs[-1]["mse_ratio_uniform_over_adaptive"] = round(out["uniform"]["mse"] / runs[-1]["mse"], 3) if runs[-1]["mse"] > 0 else None
    r.set_adaptive_sampling(None)
    out["equal_time"] = runs
    out["per_fraction"] = [{"active_fraction": f, "frames": len(v), "ms_median": round(float(np.median(v)), 4)}
                           for f, v in sorted(per_fraction.items(), reverse=True)]
    out["check_ms"] = {"n": len(check_cost), "mean": round(float(np.mean(check_cost)), 4) if check_cost else None,
                       "median": round(float(np.median(check_cost)), 4) if check_cost else None}
    r.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="1,3")
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--budget-spp", type=int, default=64)
    ap.add_argument("--max-frames", type=int, default=1024)
    ap.add_argument("--thresholds", default="0.02,0.05,0.1,0.2,0.3,0.5")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_timing.json"))
    args = ap.parse_args()
    args.thresholds = [float(t) for t in args.thresholds.split(",")]
    res = {"note": "MI355X; event-timed updates (each synchronised); MSE of accum.rgb against a --ref-spp render", "ref_spp": args.ref_spp,
           "budget_spp": args.budget_spp}
    for i in (int(c) for c in args.configs.split(",")):
        res[f"configs[{i}]"] = run_config(i, args)
    text = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
