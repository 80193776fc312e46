"""Time occlusion batches (hala_rt_occlusion, docs/RENDER_SPEC.md 4.10) on configs[1] (Cornell box, the LDS-staged form) and configs[3]
(the ~1 M-triangle atrium, the large one-level form) and write profiles/occlusion_timing.json.

Samples: the first hits of the 1920 x 1080 camera rays (a pinhole through the pixel centres of the scene's camera), evenly thinned to
about 2 M / N of them, each with the hit triangle's geometric normal turned towards the ray, bias = ray_eps and reach +inf; N = 16, 64
and 256 rays per sample, so every batch traces about 2 M rays.
Variants, `--rounds` times after `--warmup` rounds, alternating (each timed GPU call directly behind an untimed call of the same variant,
so that neither pays for the chip the host variant left idle):
  occlusion   r.occlusion() on device buffers, the masks in the renderer's own buffer: the ray generation, the traversal, the mask
              atomics and the reduction, between two HIP events on one stream
  resident    baseline (a): the same rays, expanded by the twin (tests/occlusion_ref.py) and resident in device memory, through
              hala_rt_trace_rays in mode 1 on the PARENT's library (--parent-root: the parent commit's tree, built there; without it this
              tree's library, and the JSON says so), between two HIP events: what the traversal alone costs when a host has already paid for
              the rays (k_rebase_batch copies every ray once more; the hit records stay on the device, unreduced)
  host        baseline (b): what a host does without the operator, on the host's clock from the samples in host memory to the visibilities
              in host memory: generate the count x N rays (vectorised numpy float32 with numpy's own generator: a host is not held to the
              spec's stream), upload 32 B per ray, the same mode-1 batch, read 16 B per ray back and reduce
The JSON keeps every round, the medians, the spread (max - min) and Mrays/s; the summary says per N whether the operator's time differs
from (a) by more than the spread of (a)'s own rounds.  Not timed: the operator's masks are checked against the mode-1 answers of the
expanded batch, ray for ray.  No ratio is asserted: nobody has measured this operator before."""
import argparse
import json
import os
import platform
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
TOTAL = 1 << 21
RAY_COUNTS = (16, 64, 256)
SEED = 1


def first_hit_samples(H, r, rays, hits):
    """every camera ray that hit: the point, the hit triangle's normal turned towards the ray, bias = ray_eps, reach +inf"""
    import numpy as np
    w = r.download_bvh()[1].reshape(-1, 12)
    f = w.view(np.float32)
    normal_of = np.zeros((int(w[:, 3].max()) + 1, 3), np.float32)
    normal_of[w[:, 3]] = np.cross(f[:, 4:7], f[:, 8:11])
    found = np.nonzero(hits["prim"] != 0xFFFFFFFF)[0]
    d = rays["direction"][found]
    n = normal_of[hits["prim"][found]]
    n = np.where(((n * d).sum(axis=1) < 0)[:, None], n, -n)
    s = np.zeros(len(found), dtype=H._abi.OCCLUSION_SAMPLE_DTYPE)
    s["point"] = rays["origin"][found] + d * hits["t"][found][:, None]
    s["normal"], s["bias"], s["reach"] = n, r.ray_eps(), np.inf
    return s[(n * n).sum(axis=1) > 0]


def host_rays(H, samples, n_rays, rng):
    """what a host writes itself: cosine-distributed directions around every sample's normal, vectorised float32"""
    import numpy as np
    f32 = np.float32
    count = len(samples)
    n = samples["normal"] / np.sqrt((samples["normal"] ** 2).sum(axis=1, dtype=f32))[:, None]
    sign = np.copysign(f32(1.0), n[:, 2])
    a = f32(-1.0) / (sign + n[:, 2])
    bb = n[:, 0] * n[:, 1] * a
    t = np.stack([f32(1.0) + sign * n[:, 0] * n[:, 0] * a, sign * bb, -sign * n[:, 0]], axis=1)
    b = np.stack([bb, sign + n[:, 1] * n[:, 1] * a, -n[:, 1]], axis=1)
    u = rng.random((2, count, n_rays), dtype=f32)
    rad, phi = np.sqrt(u[0]), f32(2.0 * np.pi) * u[1]
    lx, ly, lz = rad * np.cos(phi), rad * np.sin(phi), np.sqrt(f32(1.0) - u[0])
    rays = np.zeros((count, n_rays), dtype=H._abi.RAY_DTYPE)
    rays["direction"] = t[:, None, :] * lx[..., None] + b[:, None, :] * ly[..., None] + n[:, None, :] * lz[..., None]
    rays["origin"] = (samples["point"] + n * samples["bias"][:, None])[:, None, :]
    rays["tmax"] = samples["reach"][:, None]
    return rays.reshape(-1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--configs", type=int, nargs="+", default=[1, 3])
    ap.add_argument("--total", type=int, default=TOTAL, help="rays per batch, about")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occlusion_timing.json"))
    args = ap.parse_args()
    import numpy as np
    import torch

    import hala_renderer_amd as H
    import occlusion_ref as OR
    from hala_renderer_amd import workloads
    from multihit_timing import camera_rays, renderer_on
    A = H._abi
    parent_lib = os.path.join(os.path.abspath(args.parent_root), "hala-renderer_amd", "lib", "libhalart.so") if args.parent_root else None
    res = {"what": "occlusion batches (scripts/occlusion_timing.py): GPU ms between two HIP events on device buffers (occlusion, resident); host ms from "
                   "samples in host memory to visibilities in host memory (host)",
           "box": {"gpu": torch.cuda.get_device_name(0), "host": platform.processor() or platform.machine(), "hip": torch.version.hip},
           "ray_library": "parent" if parent_lib else "this tree (no --parent-root)", "rounds": args.rounds, "warmup": args.warmup, "configs": {}}
    stream = torch.cuda.Stream()

    def timed(fn):
        """one untimed call, then the timed one: a GPU variant that follows the host variant's tens of ms on the CPU would otherwise be the one
        that pays for the idle chip (clocks, cold lines), whichever it is"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    for index in args.configs:
        cfg = workloads.baseline_config(index)
        mine = H.HalaRenderer("occlusion-timing", 64, 64, 5, 3, False, False, False, 0)
        other = renderer_on(H, parent_lib, "occlusion-timing-parent") if parent_lib else mine
        for r in {id(mine): mine, id(other): other}.values():
            r.set_scene(cfg["scene"])
            r.commit()
        info = mine.bvh_info()
        cam = camera_rays(H, mine)
        pool = first_hit_samples(H, mine, cam, mine.trace_rays_host(cam, 0))
        rows = {}
        for n_rays in RAY_COUNTS:
            count = min(args.total // n_rays, len(pool))
            samples = np.ascontiguousarray(pool[np.linspace(0, len(pool) - 1, count).astype(np.int64)])
            n = count * n_rays
            expanded, ok = OR.expand(samples, n_rays, SEED)
            assert ok.all()
            d_samples = torch.from_numpy(samples.view(np.uint8).copy()).cuda()
            d_out = torch.zeros(count * 16, dtype=torch.uint8, device="cuda")
            d_masks = torch.zeros(count * ((n_rays + 31) // 32), dtype=torch.int32, device="cuda")
            d_rays = torch.from_numpy(expanded.view(np.uint8).copy()).cuda()
            d_hits = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            rng = np.random.default_rng(5)

            def occlusion():
                mine.occlusion(d_samples, rays=n_rays, seed=SEED, out=d_out, count=count, stream=stream.cuda_stream)

            def resident():
                other.trace_rays(d_rays.data_ptr(), d_hits.data_ptr(), n, 1, 0, stream.cuda_stream)

            def host():
                t0 = time.perf_counter()
                rays = host_rays(H, samples, n_rays, rng)
                up = torch.from_numpy(rays.view(np.uint8)).cuda()
                other.trace_rays(up.data_ptr(), d_hits.data_ptr(), n, 1, 0, stream.cuda_stream)
                stream.synchronize()
                back = d_hits.cpu().numpy().view(A.HIT_DTYPE)
                visibility = (back["t"] < 0).reshape(count, n_rays).mean(axis=1, dtype=np.float32)
                assert visibility.shape == (count,)
                return (time.perf_counter() - t0) * 1e3

            variants = [("occlusion", lambda: timed(occlusion)), ("resident", lambda: timed(resident)), ("host", host)]
            ms = {v: [] for v, _ in variants}
            for rnd in range(args.warmup + args.rounds):
                for v, fn in variants:  # the variants alternate: one call each per round
                    x = fn()
                    if rnd >= args.warmup:
                        ms[v].append(x)
            row = {v: {"ms": x, "median_ms": statistics.median(x), "spread_ms": max(x) - min(x), "mrays_per_s": n / statistics.median(x) / 1e3} for v, x in ms.items()}
            # not timed: the operator's masks against the mode-1 answers of the expanded batch, and what the answers look like
            mine.occlusion(d_samples, rays=n_rays, seed=SEED, out=d_out, out_masks=d_masks, count=count, stream=stream.cuda_stream)
            resident()
            stream.synchronize()
            bits = OR.bits_of(d_masks.cpu().numpy().view(np.uint32).reshape(count, -1), n_rays)
            own = (d_hits.cpu().numpy().view(A.HIT_DTYPE)["t"] > 0).reshape(count, n_rays)
            rec = d_out.cpu().numpy().view(A.OCCLUSION_DTYPE)
            gap = row["occlusion"]["median_ms"] - row["resident"]["median_ms"]
            spread = row["resident"]["spread_ms"]
            row["summary"] = {"samples": count, "rays": n, "rays_where_masks_differ_from_mode_1": int((bits != own).sum()),
                              "occluded_share": float(own.mean()), "mean_visibility": float(rec["visibility"].astype(np.float64).mean()),
                              "occlusion_minus_resident_ms": gap, "resident_spread_ms": spread,
                              "against_resident": "faster" if -gap > spread else ("slower" if gap > spread else "within the spread of the resident batch"),
                              "host_over_occlusion": row["host"]["median_ms"] / row["occlusion"]["median_ms"]}
            rows[str(n_rays)] = row
            print(cfg["name"], n_rays, json.dumps({**{v: {k: w for k, w in row[v].items() if k != "ms"} for v, _ in variants}, "summary": row["summary"]}, indent=1),
                  flush=True)
            del d_rays, d_hits, d_samples, d_out, d_masks
        res["configs"][cfg["name"]] = {"triangles": int(info.triangle_count), "lds_node_count": int(info.lds_node_count), "camera_hits": len(pool), "rays_per_sample": rows}
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        if other is not mine:
            other.close()
        mine.close()


if __name__ == "__main__":
    main()
