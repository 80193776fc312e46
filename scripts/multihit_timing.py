"""Time multi-hit ray batches (hala_rt_trace_rays_multi, docs/RENDER_SPEC.md 4.7) on configs[3]'s scene and write
profiles/multihit_timing.json.

Ray sets, about 2 M rays each: the 1920 x 1080 camera rays (a pinhole through the pixel centres of the scene's camera), and rays aimed
through the scene box from outside (origins on a sphere of 0.75 diagonals around the box centre, aimed at random points of the box).
Variants, all on device buffers, each between two HIP events on one stream:
  mode0        hala_rt_trace_rays, closest hit, this tree's library
  multi k      hala_rt_trace_rays_multi at k = 1, 2, 4, 8, 16, this tree's library
  peel k       what a caller had to do before: k closest-hit batches, tmin of every ray advanced to its last t on the device between
               two batches (a ray that missed is closed: tmax = -1), on the PARENT's library (--parent-root: the parent commit's tree,
               built there; without it the peel runs on this tree's library and the JSON says so)
  parent k     hala_rt_trace_rays_multi at the same k on the PARENT's library (only with --parent-root)
The two libraries live in one process and the variants alternate, `--rounds` times after `--warmup` rounds; the JSON keeps every round,
the medians, the spread (max - min) of each variant's rounds and Mrays/s.  The summary compares one multi-hit batch with the peel per k:
"wins" only where the gap exceeds the spread of the parent's own repeated runs; and k = 1 with mode 0 (the cost of the list machinery).
With a parent it also compares this tree's multi-hit batch with the parent's per k: "no slower" unless this tree's median exceeds the
parent's by more than the spread of the parent's rounds.
The peel returns the same lists only on rays without ties (4.7); the script counts the rays on which the two differ, it does not mind them."""
import argparse
import ctypes as C
import json
import os
import platform
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, HGT = 1920, 1080
KS = (1, 2, 4, 8, 16)


def renderer_on(H, lib_path, name):
    """a HalaRenderer of this package over another build of the library (the parent's): same ABI for everything used here"""
    lib = C.CDLL(lib_path)
    lib.hala_last_error_message.restype = C.c_char_p
    for fn, (argtypes, restype) in H._abi.PROTOTYPES.items():
        if hasattr(lib, fn):
            getattr(lib, fn).argtypes, getattr(lib, fn).restype = argtypes, restype

    def check(status):
        if status != 0:
            raise H.HalaRendererError(lib.hala_last_error_message().decode(errors="replace"))
    r = H.HalaRenderer.__new__(H.HalaRenderer)
    r._lib, r._check, r._device_ordinal, r._h = lib, check, 0, C.c_void_p()
    check(lib.hala_rt_create(name.encode(), C.c_uint32(64), C.c_uint32(64), C.c_int(0), C.c_uint32(5), C.c_uint32(3), C.c_int(0), C.c_int(0), C.c_int(0),
                             C.c_uint64(0), C.byref(r._h)))
    r.width = r.height = 64
    return r


def camera_rays(H, r):
    import numpy as np
    cam = r.packed_cameras()[0]
    pos, right, up, fwd = (np.array(list(getattr(cam, k)), dtype=np.float32)[:3] for k in ("position", "right", "up", "forward"))
    th = np.tan(0.5 * cam.yfov)
    ys, xs = np.meshgrid(np.arange(HGT), np.arange(W), indexing="ij")
    u = ((xs + 0.5) / W * 2 - 1) * th * (W / HGT); v = (1 - (ys + 0.5) / HGT * 2) * th
    d = fwd[None, None] + right[None, None] * u[..., None] + up[None, None] * v[..., None]
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    rays = np.zeros(W * HGT, dtype=H._abi.RAY_DTYPE)
    rays["origin"] = pos; rays["direction"] = d.reshape(-1, 3); rays["tmax"] = 3e38
    return rays


def through_rays(H, r, n):
    import numpy as np
    i = r.bvh_info()
    mn, mx = np.array(list(i.scene_min), np.float64), np.array(list(i.scene_max), np.float64)
    c, diag = 0.5 * (mn + mx), np.linalg.norm(mx - mn)
    rng = np.random.RandomState(7)
    u = rng.randn(n, 3); u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = c + u * 0.75 * diag
    d = mn + rng.rand(n, 3) * (mx - mn) - o
    rays = np.zeros(n, dtype=H._abi.RAY_DTYPE)
    rays["origin"] = o.astype(np.float32); rays["direction"] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32); rays["tmax"] = 3e38
    return rays


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--config", type=int, default=3, help="index of the baseline config whose scene is traced (a small one for a quick look)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multihit_timing.json"))
    args = ap.parse_args()
    import numpy as np
    import torch

    import hala_renderer_amd as H
    from hala_renderer_amd import workloads
    cfg = workloads.baseline_config(args.config)
    mine = H.HalaRenderer("multihit-timing", 64, 64, 5, 3, False, False, False, 0)
    parent_lib = os.path.join(os.path.abspath(args.parent_root), "hala-renderer_amd", "lib", "libhalart.so") if args.parent_root else None
    other = renderer_on(H, parent_lib, "multihit-timing-parent") if parent_lib else mine
    for r in {id(mine): mine, id(other): other}.values():
        r.set_scene(cfg["scene"])
        r.commit()
    info = mine.bvh_info()
    stream = torch.cuda.Stream()
    sets = {"camera": camera_rays(H, mine), "through": through_rays(H, mine, W * HGT)}
    res = {"what": f"multi-hit ray batches against the k-batch peel (scripts/multihit_timing.py) on {cfg['name']}: GPU ms between two HIP events, device buffers",
           "box": {"gpu": torch.cuda.get_device_name(0), "host": platform.processor() or platform.machine(), "hip": torch.version.hip},
           "scene": {"triangles": int(info.triangle_count), "lds_node_count": int(info.lds_node_count), "instance_ref_count": int(info.instance_ref_count)},
           "peel_library": "parent" if parent_lib else "this tree (no --parent-root)", "rounds": args.rounds, "warmup": args.warmup, "sets": {}}
    for name, rays in sets.items():
        n = len(rays)
        d_rays = torch.from_numpy(rays.view(np.float32).reshape(n, 8).copy()).cuda()
        d_work = torch.empty_like(d_rays)
        d_hits = torch.zeros((max(KS), n, 4), dtype=torch.float32, device="cuda")  # peel: layer j at d_hits[j]; multi: the first n * k records
        d_counts = torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def mode0():
            mine.trace_rays(d_rays.data_ptr(), d_hits.data_ptr(), n, 0, 0, stream.cuda_stream)

        def multi(k):
            mine.trace_rays_multi(d_rays.data_ptr(), d_hits.data_ptr(), n, k, d_counts.data_ptr(), stream.cuda_stream)

        def parent_multi(k):
            other.trace_rays_multi(d_rays.data_ptr(), d_hits.data_ptr(), n, k, d_counts.data_ptr(), stream.cuda_stream)

        def peel(k):
            with torch.cuda.stream(stream):
                d_work.copy_(d_rays)
                for j in range(k):
                    other.trace_rays(d_work.data_ptr(), d_hits[j].data_ptr(), n, 0, 0, stream.cuda_stream)
                    if j + 1 < k:
                        t = d_hits[j, :, 0]
                        hit = t > 0
                        d_work[:, 3] = torch.where(hit, t, d_work[:, 3])
                        d_work[:, 7] = torch.where(hit, d_work[:, 7], torch.full_like(t, -1.0))

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        variants = [("mode0", mode0)] + [(f"multi_{k}", lambda k=k: multi(k)) for k in KS] + [(f"peel_{k}", lambda k=k: peel(k)) for k in KS]
        if parent_lib:
            variants += [(f"parent_{k}", lambda k=k: parent_multi(k)) for k in KS]
        ms = {v: [] for v, _ in variants}
        for rnd in range(args.warmup + args.rounds):
            for v, fn in variants:  # the variants alternate: one call each per round
                x = timed(fn)
                if rnd >= args.warmup:
                    ms[v].append(x)
        # what the two ways return (not timed): hit counts, and on how many rays the peel's list differs from the multi-hit one
        differ = {}
        for k in KS:
            multi(k); stream.synchronize()
            a = d_hits.reshape(-1, 4)[: n * k].reshape(n, k, 4).view(torch.int32).clone()
            counts = d_counts.clone()
            peel(k); stream.synchronize()
            b = d_hits[:k].permute(1, 0, 2).contiguous().view(torch.int32)
            differ[str(k)] = {"rays_with_k_hits": int((counts == k).sum()), "mean_hits": float(counts.float().mean()),
                              "rays_where_peel_differs": int((a != b).reshape(n, -1).any(dim=1).sum())}
        rows = {v: {"ms": x, "median_ms": statistics.median(x), "spread_ms": max(x) - min(x), "mrays_per_s": n / statistics.median(x) / 1e3} for v, x in ms.items()}
        summary = {}
        for k in KS:
            m, p = rows[f"multi_{k}"], rows[f"peel_{k}"]
            gap = p["median_ms"] - m["median_ms"]
            summary[str(k)] = {"multi_ms": m["median_ms"], "peel_ms": p["median_ms"], "peel_spread_ms": p["spread_ms"], "peel_over_multi": p["median_ms"] / m["median_ms"],
                               "verdict": "multi wins" if gap > p["spread_ms"] else ("peel wins" if -gap > p["spread_ms"] else "within the peel's spread")}
            if parent_lib:
                q = rows[f"parent_{k}"]
                summary[str(k)].update(parent_multi_ms=q["median_ms"], parent_multi_spread_ms=q["spread_ms"], multi_minus_parent_ms=m["median_ms"] - q["median_ms"],
                                       against_parent="no slower" if m["median_ms"] - q["median_ms"] <= q["spread_ms"] else "SLOWER than the parent")
        summary["k1_over_mode0"] = rows["multi_1"]["median_ms"] / rows["mode0"]["median_ms"]
        res["sets"][name] = {"rays": n, "variants": rows, "lists": differ, "summary": summary}
        print(name, json.dumps(summary, indent=1), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    if other is not mine:
        other.close()
    mine.close()


if __name__ == "__main__":
    main()
