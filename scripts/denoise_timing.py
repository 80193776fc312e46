"""Time the a-trous denoiser (hala_rt_denoise, docs/RENDER_SPEC.md 10) on configs[3]'s frame: the atrium at 4 spp, filtered with the
default parameters at 1920x1080 and at 3840x2160.  Prints one JSON line.

  ms_event : mean of the event-timed gpu_ms of `--calls` calls (each call times its own launches and waits)
  ms_host  : host clock around `--calls` back-to-back untimed calls ending in one synchronise, per call
  bytes    : unique bytes the filter moves (prepass: 48 B in, 48 B out per pixel; pass: 48 B in, 32 B out; last pass 48 in, 16 out),
             the taps served from the caches not counted; GB/s = bytes / ms_event
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import hala_renderer_amd as H  # noqa: E402
from hala_renderer_amd import workloads  # noqa: E402


def model_bytes(w, h, iterations):
    n = w * h
    return n * (96 + (iterations - 1) * 80 + 64)


def time_frame(scene, env, w, h, spp, calls, warmup):
    r = H.HalaRenderer("denoise_timing", w, h, workloads.MAX_DEPTH, workloads.RR_DEPTH, False, False, False, 0)
    r.set_envmap(env, 0.0)
    r.set_scene(scene)
    r.commit()
    r.update_batch(spp)
    r.wait_idle()
    for _ in range(warmup):
        r.denoise()
    r.wait_idle()
    ev = [r.denoise(timed=True) for _ in range(calls)]
    t0 = time.perf_counter()
    for _ in range(calls):
        r.denoise()
    r.wait_idle()
    host = (time.perf_counter() - t0) * 1e3 / calls
    it = H.denoise_default_params().iterations
    r.close()
    ms = sum(ev) / len(ev)
    b = model_bytes(w, h, it)
    return {"ms_event": round(ms, 4), "ms_event_min": round(min(ev), 4), "ms_event_max": round(max(ev), 4), "ms_host": round(host, 4),
            "bytes": b, "gbps": round(b / (ms * 1e-3) / 1e9, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    args = ap.parse_args()
    cfg = workloads.baseline_config(3)
    d = H.denoise_default_params()
    out = {"workload": "configs[3] frame (atrium, 4 spp), hala_rt_denoise with the default parameters",
           "params": {"iterations": d.iterations, "sigma_color": d.sigma_color, "sigma_albedo": d.sigma_albedo,
                      "normal_power": d.normal_power, "demodulate": d.demodulate},
           "calls": args.calls}
    for name in args.sizes.split(","):
        w, h = (int(v) for v in name.split("x"))
        scene, env = workloads.atrium(aspect=w / h)
        out[name] = time_frame(scene, env, w, h, cfg["spp"], args.calls, args.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
