"""Time views (hala_rt_set_views, docs/RENDER_SPEC.md 12) against separate renderers and write profiles/multiview_timing.json.

For configs[3] (atrium) and configs[1] (Cornell box), each with the cameras of scenes.with_extra_cameras, two forms render the same
cameras with the same paths:
  views    : ONE renderer with set_views(cameras): one update = one sample per pixel of every view, in one wavefront pass
  separate : one renderer per camera (set_views([c])), updated in turn: one pass per camera
at 480x270 with 8 cameras and at 1920x1080 with 4.  After `--warmup` all-views frames, at least `--frames` of them and at least
`--window-ms` of the faster form (the same count for both forms) are timed: the host clock
around the updates of the frames and the synchronisation of every renderer's stream at the end (wait_idle), so a figure holds every
launch, tail and gap, and the renderers of the separate form may overlap each other as they would in an application.  The two forms
alternate `--rounds` times in one process; the JSON keeps every round (ms per all-views frame, Mrays/s from the renderers' ray totals)
and the median and spread over the rounds.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import hala_renderer_amd as H  # noqa: E402
from hala_renderer_amd import scenes, workloads  # noqa: E402

CASES = [(480, 270, 8), (1920, 1080, 4)]


def make(cfg, scene, w, h, cams):
    r = H.HalaRenderer("multiview", w, h, cfg["max_depth"], cfg["rr_depth"], False, False, False, 0)
    if cfg["env"] is not None:
        r.set_envmap(cfg["env"], 0.0)
    r.set_scene(scene)
    r.commit()
    r.set_launch_timing_period(0)  # the production path: untimed updates, overlapped tails
    r.set_views(cams)
    return r


def rays(rs):
    return sum(r.statistics().rays_total for r in rs)


def run(rs, frames):
    """ms per all-views frame, Mrays/s"""
    for r in rs:
        r.wait_idle()
    r0 = rays(rs)
    t0 = time.perf_counter()
    for _ in range(frames):
        for r in rs:
            r.update()
        for r in rs:
            r.render()  # at most two updates in flight per renderer, as an application's frame loop has
    for r in rs:
        r.wait_idle()
    dt = time.perf_counter() - t0
    return 1e3 * dt / frames, (rays(rs) - r0) / dt / 1e6


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def run_config(index, args):
    cfg = workloads.baseline_config(index)
    base = cfg["scene"]
    scene = scenes.with_extra_cameras(base, 7)
    out = []
    for w, h, nv in CASES:
        cams = list(range(nv))
        if index in (0, 1):  # the Cornell box's aspect follows the frame
            scene = scenes.with_extra_cameras(scenes.cornell_box(aspect=w / h), 7)
        views = make(cfg, scene, w, h, cams)
        separate = [make(cfg, scene, w, h, [c]) for c in cams]
        # warm up, and size the timed window: at least `--frames` frames and `--window-ms` of the faster form
        fastest = min(run([views], args.warmup)[0], run(separate, args.warmup)[0])
        frames = max(args.frames, int(args.window_ms / max(fastest, 1e-3)) + 1)
        rounds = []
        for k in range(args.rounds):  # alternate the order, so that neither form always runs on a warmer chip
            order = [("views", [views]), ("separate", separate)]
            if k % 2:
                order.reverse()
            rec = {}
            for name, rs in order:
                ms, mrays = run(rs, frames)
                rec[name] = {"ms_per_frame": ms, "mrays_per_s": mrays}
            rounds.append(rec)
        res = {"width": w, "height": h, "views": nv, "frames_per_round": frames, "rounds": rounds}
        for name in ("views", "separate"):
            res[name] = {"ms_per_frame": summary([r[name]["ms_per_frame"] for r in rounds]),
                         "mrays_per_s": summary([r[name]["mrays_per_s"] for r in rounds])}
        res["speedup_median"] = res["separate"]["ms_per_frame"]["median"] / res["views"]["ms_per_frame"]["median"]
        print(f"configs[{index}] {w}x{h} x{nv} views: one pass {res['views']['ms_per_frame']['median']:.3f} ms "
              f"({res['views']['mrays_per_s']['median']:.0f} Mrays/s), separate {res['separate']['ms_per_frame']['median']:.3f} ms "
              f"({res['separate']['mrays_per_s']['median']:.0f} Mrays/s), x{res['speedup_median']:.3f}", flush=True)
        out.append(res)
        for r in [views] + separate:
            r.close()
    return {"config": cfg["name"], "cases": out}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default="3,1")
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--window-ms", type=float, default=1000.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multiview_timing.json"))
    args = ap.parse_args()
    H.load_library()
    res = {"what": "one renderer with N views vs N single-view renderers updated in turn (scripts/multiview_timing.py)",
           "frames": args.frames, "window_ms": args.window_ms, "warmup": args.warmup, "rounds": args.rounds,
           "configs": [run_config(int(i), args) for i in args.configs.split(",")]}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
