"""Time closest-point query batches (hala_rt_closest_points, docs/RENDER_SPEC.md 4.8) on configs[1] (Cornell box, the LDS-staged form)
and configs[3] (the ~1 M-triangle atrium, the large one-level form) and write profiles/closest_point_timing.json.

Query sets, 2 M queries each, radius +inf, made from the triangles the renderer holds (hala_rt_download_bvh):
  surface   points on triangles (a triangle picked at random, uniform barycentrics)
  near      such points moved along the triangle's normal by up to 1 % of the scene diagonal, either side
  box       uniform points in twice the scene box
Each batch runs on device buffers between two HIP events on one stream, `--rounds` times after `--warmup` rounds, the sets alternating;
the JSON keeps every round, the median, the spread (max - min) and Mqueries/s.  Node visits and triangle tests per query come from one
run of each set through the counting variant of the kernel (hala_rt_closest_points_counted), not timed.
For scale: 2 M closest-hit camera rays (1920 x 1080, a pinhole through the pixel centres of the scene's camera) through
hala_rt_trace_rays with its step counters, on the PARENT's library with --parent-root (the parent commit's tree, built there), else on
this tree's library — the JSON says which.  No ratio is asserted: nobody has measured this operator before."""
import argparse
import json
import os
import platform
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
N = 1920 * 1080


def triangles(r):
    import numpy as np
    w = r.download_bvh()[1].reshape(-1, 12).view(np.float32)
    return w[:, 0:3].astype(np.float64), w[:, 4:7].astype(np.float64), w[:, 8:11].astype(np.float64)


def query_sets(r, n):
    import numpy as np
    v0, e1, e2 = triangles(r)
    i = r.bvh_info()
    mn, mx = np.array(list(i.scene_min), np.float64), np.array(list(i.scene_max), np.float64)
    c, ext = 0.5 * (mn + mx), mx - mn
    diag = np.linalg.norm(ext)
    rng = np.random.RandomState(11)
    t = rng.randint(0, len(v0), n)
    a, b = rng.rand(n), rng.rand(n)
    flip = a + b > 1.0
    a, b = np.where(flip, 1.0 - a, a), np.where(flip, 1.0 - b, b)
    on = v0[t] + a[:, None] * e1[t] + b[:, None] * e2[t]
    nrm = np.cross(e1[t], e2[t])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
    near = on + nrm * (rng.uniform(-0.01, 0.01, n) * diag)[:, None]
    box = c + (rng.rand(n, 3) - 0.5) * 2.0 * ext
    return {"surface": on.astype(np.float32), "near": near.astype(np.float32), "box": box.astype(np.float32)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--configs", type=int, nargs="+", default=[1, 3])
    ap.add_argument("--queries", type=int, default=N)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "closest_point_timing.json"))
    args = ap.parse_args()
    import numpy as np
    import torch

    import hala_renderer_amd as H
    from hala_renderer_amd import workloads
    from multihit_timing import camera_rays, renderer_on
    A = H._abi
    parent_lib = os.path.join(os.path.abspath(args.parent_root), "hala-renderer_amd", "lib", "libhalart.so") if args.parent_root else None
    res = {"what": "closest-point query batches (scripts/closest_point_timing.py): GPU ms between two HIP events, device buffers, radius +inf",
           "box": {"gpu": torch.cuda.get_device_name(0), "host": platform.processor() or platform.machine(), "hip": torch.version.hip},
           "ray_library": "parent" if parent_lib else "this tree (no --parent-root)", "rounds": args.rounds, "warmup": args.warmup, "configs": {}}
    stream = torch.cuda.Stream()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    for index in args.configs:
        cfg = workloads.baseline_config(index)
        mine = H.HalaRenderer("closest-point-timing", 64, 64, 5, 3, False, False, False, 0)
        other = renderer_on(H, parent_lib, "closest-point-timing-parent") if parent_lib else mine
        for r in {id(mine): mine, id(other): other}.values():
            r.set_scene(cfg["scene"])
            r.commit()
        info = mine.bvh_info()
        n = args.queries
        d_sets = {}
        for name, pts in query_sets(mine, n).items():
            q = np.empty(n, dtype=A.POINT_QUERY_DTYPE)
            q["point"] = pts; q["radius"] = np.inf
            d_sets[name] = torch.from_numpy(q.view(np.uint8).copy()).cuda()
        d_out = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
        d_ctr = torch.zeros(2, dtype=torch.int64, device="cuda")
        rays = camera_rays(H, mine)
        d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
        d_hits = torch.zeros(len(rays) * 16, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        variants = [(name, lambda d=d: mine.closest_points(d, out=d_out, count=n, stream=stream.cuda_stream)) for name, d in d_sets.items()]
        variants.append(("camera_rays", lambda: other.trace_rays(d_rays.data_ptr(), d_hits.data_ptr(), len(rays), 0, 0, stream.cuda_stream)))
        ms = {v: [] for v, _ in variants}
        for rnd in range(args.warmup + args.rounds):
            for v, fn in variants:  # the variants alternate: one call each per round
                x = timed(fn)
                if rnd >= args.warmup:
                    ms[v].append(x)
        rows = {}
        for v, x in ms.items():
            count = len(rays) if v == "camera_rays" else n
            rows[v] = {"ms": x, "median_ms": statistics.median(x), "spread_ms": max(x) - min(x), "mqueries_per_s": count / statistics.median(x) / 1e3}
        for name, d in d_sets.items():  # not timed: the counting variant, and what the answers look like
            mine.closest_points(d, out=d_out, count=n, stream=stream.cuda_stream, d_counters=d_ctr.data_ptr())
            stream.synchronize()
            nodes, tris = (int(x) for x in d_ctr.cpu())
            rec = d_out.cpu().numpy().view(A.CLOSEST_POINT_DTYPE)
            rows[name].update(nodes_per_query=nodes / n, tris_per_query=tris / n, answered=int((rec["prim"] != 0xFFFFFFFF).sum()),
                              regions=np.bincount(rec["region"], minlength=7).tolist(), mean_distance=float(rec["distance"].astype(np.float64).mean()))
        other.trace_rays(d_rays.data_ptr(), d_hits.data_ptr(), len(rays), 0, d_ctr.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        nodes, tris = (int(x) for x in d_ctr.cpu())
        rows["camera_rays"].update(nodes_per_query=nodes / len(rays), tris_per_query=tris / len(rays))
        res["configs"][cfg["name"]] = {"triangles": int(info.triangle_count), "lds_node_count": int(info.lds_node_count), "queries": n, "rays": len(rays), "variants": rows}
        print(cfg["name"], json.dumps({v: {k: w for k, w in row.items() if k != "ms"} for v, row in rows.items()}, indent=1), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        if other is not mine:
            other.close()
        mine.close()


if __name__ == "__main__":
    main()
