"""Time transfer bakes (hala_rt_bake_transfer, docs/RENDER_SPEC.md 4.13) on configs[3] (the ~1 M-triangle atrium, committed flattened,
with scripts/bake_timing.py's ceiling quad) and write profiles/bake_transfer_timing.json.

The receiver is the tessellated floor (instance 0; its triangles wind downwards, so it is baked with the flip: the rays start above it
and run down into it), the targets are the default set: every other instance.  Maps of --sizes, `front` = --fronts (shares of the scene's
diagonal), back = front.  Variants, `--rounds` times after `--warmup` rounds, alternating, each timed call directly behind an untimed
call of the same variant, between two HIP events on one stream, all buffers on the device:
  samples       r.bake_samples(): the rasteriser alone
  transfer_m0   r.bake_transfer(margin=0): rasteriser, trace and resolve; transfer_m0 - samples is trace + resolve
  transfer_m16  r.bake_transfer(margin=16): the whole call; transfer_m16 - transfer_m0 is the dilation
  mode0         the SAME rays (made on the host from the sample buffer, resident on the device) through hala_rt_trace_rays, mode 0, on the
                parent's library: another answer (every triangle is seen, the floor first of all), a rays/s yardstick for what the
                filter and the in-lane ray generation cost
The kernels apart come from a kernel trace: `--kernel-trace-csv FILE` folds the per-dispatch rows of a `rocprofv3 --kernel-trace` run of
this script with --trace-run into the JSON, by kernel name per case.
The workaround a host has without the operator, on the PARENT's library (--parent-root: the parent commit's tree, built there; without it
this tree's library, and the JSON says so), on the host's clock from nothing to the records in host memory, maps of --host-sizes:
bake_samples in its host form, the rays in numpy, trace_rays_multi(k = 16) in its host form, a numpy filter by instance, no normals and no
gutter fill; beside it the whole call in its host form, r.bake_transfer() to host arrays, and how many texels the workaround gets wrong
(its list was full before a target came).
Nothing here is a threshold: no number existed for any of it."""
import argparse
import csv
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
KERNELS = ("k_bake_count", "k_bake_cover", "k_bake_sample", "k_trace_transfer", "k_transfer_resolve", "k_bake_blocks", "k_bake_dilate_transfer")


def fold_trace(path, cases):
    """per case (in launch order, one k_bake_count each) the microseconds of each kernel of KERNELS, summed over its launches in the case"""
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    out, cur = [], None
    for start, end, name in rows:
        if "k_bake_count" in name:
            cur = {"other_us": 0.0}
            out.append(cur)
        if cur is None:
            continue
        key = next((k + "_us" for k in sorted(KERNELS, key=len, reverse=True) if k in name), "other_us")
        cur[key] = cur.get(key, 0.0) + (end - start) / 1e3
    return [{"case": c, **k} for c, k in zip(cases, out)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--fronts", type=float, nargs="+", default=[0.01, 0.1], help="shares of the scene's diagonal")
    ap.add_argument("--host-sizes", type=int, nargs="+", default=[1024])
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--trace-run", action="store_true", help="one bake_transfer(margin=16) per case and nothing else: what a kernel trace should see")
    ap.add_argument("--kernel-trace-csv", default=None, help="fold the kernel trace of a --trace-run into --out and exit (no GPU needed)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bake_transfer_timing.json"))
    args = ap.parse_args()
    cases = [(size, share) for size in args.sizes for share in args.fronts]
    if args.kernel_trace_csv:
        with open(args.out) as f:
            res = json.load(f)
        res["kernels_us"] = {"what": "rocprofv3 --kernel-trace of --trace-run: one bake_transfer(margin = 16) per case, microseconds per kernel",
                             "cases": fold_trace(args.kernel_trace_csv, ["/".join(map(str, c)) for c in cases])}
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        return
    import numpy as np
    import torch

    import bake_transfer_ref as TR
    import hala_renderer_amd as H
    from bake_timing import scene_with_ceiling
    from multihit_timing import renderer_on
    A = H._abi
    scene, _, instance = scene_with_ceiling(H)
    inst = instance["floor"]
    parent_lib = os.path.join(os.path.abspath(args.parent_root), "hala-renderer_amd", "lib", "libhalart.so") if args.parent_root else None
    mine = H.HalaRenderer("transfer-timing", 64, 64, 5, 3, False, False, False, 0)
    mine.set_build_options(instancing=False)
    mine.set_scene(scene)
    mine.commit()
    info = mine.bvh_info()
    assert info.instance_ref_count == 0
    ext = np.array(info.scene_max[:], np.float64) - np.array(info.scene_min[:], np.float64)
    diag = float(np.sqrt((ext * ext).sum()))
    firsts = np.cumsum([0] + [len(pr.indices) // 3 for nd in scene.nodes if nd.mesh_index != A.INVALID_INDEX for pr in scene.meshes[nd.mesh_index].primitives])
    other = mine
    if parent_lib and not args.trace_run:
        other = renderer_on(H, parent_lib, "transfer-timing-parent")
        other.set_build_options(instancing=False)
        other.set_scene(scene)
        other.commit()
    stream = torch.cuda.Stream()
    res = {"what": "transfer bakes (scripts/bake_transfer_timing.py): GPU ms between two HIP events on device buffers; host ms on the host's clock",
           "box": {"gpu": torch.cuda.get_device_name(0), "host": platform.processor() or platform.machine(), "hip": torch.version.hip},
           "parent_library": "parent" if parent_lib else "this tree (no --parent-root)", "rounds": args.rounds, "warmup": args.warmup,
           "scene": {"triangles": int(info.triangle_count), "receiver_triangles": int(firsts[inst + 1] - firsts[inst]), "diagonal": diag,
                     "staged": bool(info.lds_node_count > 0)},
           "cases": {}, "host": {}}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    for size in args.sizes:
        count = size * size
        d_s = torch.zeros(count * 32, dtype=torch.uint8, device="cuda")
        d_o = torch.zeros(count * 32, dtype=torch.uint8, device="cuda")
        d_t = torch.zeros(count * 16, dtype=torch.uint8, device="cuda")
        d_h = torch.zeros(count * 16, dtype=torch.uint8, device="cuda")
        for share in args.fronts:
            front = float(np.float32(share * diag))
            kw = dict(flip=True, out_texels=d_t, stream=stream.cuda_stream)
            if args.trace_run:
                mine.bake_transfer(inst, size, size, front, margin=16, out=d_o, **kw)
                stream.synchronize()
                continue
            mine.bake_samples(inst, size, size, bias=0.0, out=d_s, **kw)
            stream.synchronize()
            rays, valid = TR.Twin.rays(d_s.cpu().numpy().view(A.OCCLUSION_SAMPLE_DTYPE), front, front)
            d_r = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
            torch.cuda.synchronize()
            variants = [("samples", lambda: mine.bake_samples(inst, size, size, bias=0.0, out=d_s, **kw)),
                        ("transfer_m0", lambda: mine.bake_transfer(inst, size, size, front, margin=0, out=d_o, **kw)),
                        ("transfer_m16", lambda: mine.bake_transfer(inst, size, size, front, margin=16, out=d_o, **kw)),
                        ("mode0", lambda: other.trace_rays(d_r.data_ptr(), d_h.data_ptr(), count, 0, 0, stream.cuda_stream))]
            ms = {v: [] for v, _ in variants}
            for rnd in range(args.warmup + args.rounds):
                for v, fn in variants:
                    x = timed(fn)
                    if rnd >= args.warmup:
                        ms[v].append(x)
            row = {v: {"ms": x, "median_ms": statistics.median(x), "spread_ms": max(x) - min(x)} for v, x in ms.items()}
            stream.synchronize()
            tex = d_t.cpu().numpy().view(A.BAKE_TEXEL_DTYPE)
            rec = d_o.cpu().numpy().view(A.BAKE_TRANSFER_HIT_DTYPE)
            owned = tex["prim"] != 0xFFFFFFFF
            trace_ms = row["transfer_m0"]["median_ms"] - row["samples"]["median_ms"]
            row["summary"] = {"texels": count, "front": front, "owned_share": float(owned.mean()), "rays": int(valid.sum()),
                              "hit_share_of_owned": float((rec["t"][owned] >= 0).mean()) if owned.any() else None,
                              "trace_and_resolve_ms": trace_ms, "dilation_ms": row["transfer_m16"]["median_ms"] - row["transfer_m0"]["median_ms"],
                              "mrays_per_s_transfer": float(valid.sum()) / trace_ms / 1e3,
                              "mrays_per_s_mode0": float(valid.sum()) / row["mode0"]["median_ms"] / 1e3}
            res["cases"][f"{size}/{share}"] = row
            print(size, share, json.dumps({**{v: round(row[v]["median_ms"], 4) for v, _ in variants}, **row["summary"]}), flush=True)
            del d_r
        del d_s, d_o, d_t, d_h
    if not args.no_host and not args.trace_run:
        for size in args.host_sizes:
            for share in args.fronts:
                front = float(np.float32(share * diag))
                t0 = time.perf_counter()
                samples, _ = other.bake_samples(inst, size, size, flip=True, bias=0.0)
                t1 = time.perf_counter()
                rays, valid = TR.Twin.rays(samples.reshape(-1), front, front)
                t2 = time.perf_counter()
                lists, counts = other.trace_rays_multi_host(rays, 16)
                t3 = time.perf_counter()
                listed = lists["prim"] != 0xFFFFFFFF
                target = listed & ((np.searchsorted(firsts, np.where(listed, lists["prim"], 0), side="right") - 1) != inst)
                found = target.any(axis=1)
                hit = lists[np.arange(len(rays)), np.argmax(target, axis=1)]
                t4 = time.perf_counter()
                got_r, got_t = mine.bake_transfer(inst, size, size, front, flip=True)
                t5 = time.perf_counter()
                got = got_r.reshape(-1)
                wrong = (found != (got["t"] >= 0)) | (found & ((hit["t"] != got["t"]) | (hit["prim"] != got["prim"])))
                row = {"bake_samples_host_form_ms": (t1 - t0) * 1e3, "rays_ms": (t2 - t1) * 1e3, "multi_hit_k16_host_form_ms": (t3 - t2) * 1e3,
                       "filter_ms": (t4 - t3) * 1e3, "workaround_ms": (t4 - t0) * 1e3, "bake_transfer_host_form_ms": (t5 - t4) * 1e3,
                       "texels_the_workaround_gets_wrong": int(wrong.sum()), "lists_full_without_a_target": int(((counts == 16) & ~found).sum())}
                res["host"][f"{size}/{share}"] = row
                print("host", size, share, json.dumps(row), flush=True)
    if other is not mine:
        other.close()
    if not args.trace_run:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    mine.close()


if __name__ == "__main__":
    main()
