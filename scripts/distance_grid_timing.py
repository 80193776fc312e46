"""Time signed distance grids (hala_rt_distance_grid, docs/RENDER_SPEC.md 4.9) on configs[1] (Cornell box, the LDS-staged form) and
configs[3] (the ~1 M-triangle atrium, the large one-level form) and write profiles/distance_grid_timing.json.

Sets: cubic grids of 64, 128 and 256 voxels a side over 1.1 times the scene box's largest extent, centred on the box (64 is the coarse
case: the same box, voxels four times the size of 256's), and 512 a side on the last config without the baseline (its query batch
would be 2 GB); band +inf and band = four spacings; method 1 (a voxel per lane) and method 2 (a brick per wave); unsigned and signed.
The row pass is not callable alone: its time is reported as signed minus unsigned, from the medians of the same round set.  Which
method an automatic grid runs is read off the counters of one more run (only method 2 fetches per wave) and stands beside the faster.
Each grid runs on device buffers between two HIP events on one stream, `--rounds` times after `--warmup` rounds, the sets alternating;
the JSON keeps every round, the median, the spread (max - min) and Mvoxels/s.  Node visits and triangle tests per voxel come from one run
of each set through the counting variants (hala_rt_distance_grid_counted; include/halart.h says what one count is in each method), not
timed.
Baseline, what a host does without this entry point: hala_rt_closest_points on the same points with the same radius, in x-fastest order
and in random order, on the PARENT's library with --parent-root (the parent commit's tree, built there), else on this tree's — the
JSON says which.  The sign has no baseline.  No ratio is asserted: nobody has measured this operator before."""
import argparse
import json
import os
import platform
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def grid_of(info, n):
    import numpy as np
    mn, mx = np.array(list(info.scene_min), np.float64), np.array(list(info.scene_max), np.float64)
    spacing = np.float32(1.1 * (mx - mn).max() / (n - 1))
    origin = (0.5 * (mn + mx) - 0.5 * (n - 1) * np.float64(spacing) + np.array([0.0137, 0.0071, -0.0093]) * np.float64(spacing)).astype(np.float32)
    return origin, spacing


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--configs", type=int, nargs="+", default=[1, 3])
    ap.add_argument("--sides", type=int, nargs="+", default=[64, 128, 256, 512])
    ap.add_argument("--baseline-max-side", type=int, default=256, help="larger grids run the two methods only (a 512-cubed batch of queries is 2 GB)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distance_grid_timing.json"))
    args = ap.parse_args()
    import numpy as np
    import torch

    import hala_renderer_amd as H
    from hala_renderer_amd import workloads
    from multihit_timing import renderer_on
    A = H._abi
    parent_lib = os.path.join(os.path.abspath(args.parent_root), "hala-renderer_amd", "lib", "libhalart.so") if args.parent_root else None
    res = {"what": "signed distance grids (scripts/distance_grid_timing.py): GPU ms between two HIP events, device buffers",
           "box": {"gpu": torch.cuda.get_device_name(0), "host": platform.processor() or platform.machine(), "hip": torch.version.hip},
           "baseline_library": "parent" if parent_lib else "this tree (no --parent-root)", "rounds": args.rounds, "warmup": args.warmup, "configs": {}}
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
        mine = H.HalaRenderer("distance-grid-timing", 64, 64, 5, 3, False, False, False, 0)
        other = renderer_on(H, parent_lib, "distance-grid-timing-parent") if parent_lib else mine
        for r in {id(mine): mine, id(other): other}.values():
            r.set_scene(cfg["scene"])
            r.commit()
        info = mine.bvh_info()
        mn, mx = np.array(list(info.scene_min), np.float64), np.array(list(info.scene_max), np.float64)
        out_cfg = {"triangles": int(info.triangle_count), "lds_node_count": int(info.lds_node_count), "scene_min": mn.tolist(), "scene_max": mx.tolist(), "grids": {}}
        res["configs"][cfg["name"]] = out_cfg
        for side in args.sides:
            origin, spacing = grid_of(info, side)
            n = side ** 3
            d_dist = torch.zeros(n, dtype=torch.float32, device="cuda")
            d_ctr = torch.zeros(6, dtype=torch.int64, device="cuda")
            baseline = side <= args.baseline_max_side
            if not baseline and index != args.configs[-1]:
                continue  # the finest grid: on the last (the large) config only
            d_rec = torch.zeros(n * 32 if baseline else 32, dtype=torch.uint8, device="cuda")
            ax = [(np.arange(side, dtype=np.float32) * spacing + origin[a]).astype(np.float32) for a in range(3)]
            if baseline:
                zz, yy, xx = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
                q = np.empty(n, dtype=A.POINT_QUERY_DTYPE)
                q["point"] = np.stack([xx.ravel(), yy.ravel(), zz.ravel()], axis=1)
                perm = np.random.RandomState(5).permutation(n)
            for band_name, band in (("inf", np.float32(np.inf)), ("4_spacings", np.float32(4.0) * spacing)):
                d_q = d_q_random = None
                if baseline:
                    q["radius"] = band
                    d_q = torch.from_numpy(q.view(np.uint8).copy()).cuda()
                    d_q_random = torch.from_numpy(q[perm].view(np.uint8).copy()).cuda()
                torch.cuda.synchronize()

                def grid_call(method, signed, ctr=0):
                    mine.distance_grid(origin, spacing, (side, side, side), band=band, signed=signed, method=method, out=d_dist, stream=stream.cuda_stream,
                                       d_counters=ctr)
                variants = [(f"method{m}_{'signed' if s else 'unsigned'}", lambda m=m, s=s: grid_call(m, s)) for m in (1, 2) for s in (False, True)]
                if baseline:
                    variants.append(("closest_points_x_fastest", lambda: other.closest_points(d_q, out=d_rec, count=n, stream=stream.cuda_stream)))
                    variants.append(("closest_points_random", lambda: other.closest_points(d_q_random, out=d_rec, count=n, stream=stream.cuda_stream)))
                ms = {v: [] for v, _ in variants}
                for rnd in range(args.warmup + args.rounds):
                    for v, fn in variants:  # the variants alternate: one call each per round
                        x = timed(fn)
                        if rnd >= args.warmup:
                            ms[v].append(x)
                rows = {v: {"ms": x, "median_ms": statistics.median(x), "spread_ms": max(x) - min(x), "mvoxels_per_s": n / statistics.median(x) / 1e3}
                        for v, x in ms.items()}
                for m in (1, 2):  # not timed: the counting variants
                    grid_call(m, True, d_ctr.data_ptr())
                    stream.synchronize()
                    c = [int(x) for x in d_ctr.cpu()]
                    rows[f"method{m}_signed"].update(nodes_per_voxel=c[0] / n, tris_per_voxel=c[1] / n, row_nodes_per_voxel=c[2] / n, row_tris_per_voxel=c[3] / n,
                                                     wave_node_fetches_per_voxel=c[4] / n, wave_tri_fetches_per_voxel=c[5] / n)
                    rows[f"rows_method{m}"] = {"median_ms": rows[f"method{m}_signed"]["median_ms"] - rows[f"method{m}_unsigned"]["median_ms"],
                                               "how": "signed minus unsigned, medians"}
                grid_call(None, True, d_ctr.data_ptr())  # which method an automatic grid runs: only method 2 fetches per wave
                stream.synchronize()
                rows["automatic"] = {"method": 2 if int(d_ctr.cpu()[4]) > 0 else 1,
                                     "faster": min((1, 2), key=lambda m: rows[f"method{m}_unsigned"]["median_ms"])}
                d = d_dist.cpu().numpy()
                rows["grid"] = {"inside": int(np.signbit(d).sum()), "by_band": int((np.abs(d) == band).sum()) if np.isfinite(band) else 0}
                out_cfg["grids"].setdefault(str(side), {"spacing": float(spacing), "voxels": n, "bands": {}})["bands"][band_name] = rows
                print(cfg["name"], side, band_name, json.dumps({v: {k: w for k, w in row.items() if k != "ms"} for v, row in rows.items()}), flush=True)
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    json.dump(res, f, indent=1)
                del d_q, d_q_random
        if other is not mine:
            other.close()
        mine.close()


if __name__ == "__main__":
    main()
