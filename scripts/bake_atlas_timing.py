"""Time bake atlases (hala_rt_bake_atlas_samples / hala_rt_bake_atlas_occlusion, docs/RENDER_SPEC.md 4.12) against the bake maps of the
PARENT's library on configs[3] (the ~1 M-triangle atrium, committed flattened; scripts/bake_timing.py's scene: the tessellated floor and
a quad above the walls) and write profiles/bake_atlas_timing.json.

The parent (--parent-root: the parent commit's tree, built there) has no charts: its quarter charts are made as scripts/bake_timing.py
makes them, UVs halved by update_vertices + refit.  This tree's renderer keeps the UVs and places the charts by scale and offset.  Per
case, `--rounds` times after `--warmup` rounds, the variants alternating, each timed call directly behind an untimed call of itself,
between two HIP events on one stream, all buffers on the device; medians and spreads (max - min):
  quarter/<which>/<size>/<N>   the chart on a quarter of a size x size map
      parent_samples, parent_occlusion, parent_whole    bake_samples, occlusion on that buffer, bake_occlusion(margin=0) of the parent
      atlas_samples, atlas_whole                        bake_atlas_samples, bake_atlas_occlusion(margin=0): one chart, scale 0.5
      half_full                                         this tree's plain bake_occlusion of the full chart on the (size/2)^2 map: the same
                                                        covered texels, nothing empty — the floor for what compaction can gain
      the listed pass with its list is atlas_whole - atlas_samples; the parent's pass is parent_occlusion
  full/<which>/<size>/<N>      the chart fills the map (nothing empty): what decides which pass hala_rt_bake_occlusion uses
      parent_whole, plain_whole (this tree's bake_occlusion), listed_whole (an atlas of one identity chart)
  both/<size>/<N>              floor and quad at a quarter each in ONE atlas, against two parent calls into two size x size maps
`--trace-run` makes one bake_atlas_occlusion(margin=16) per quarter case and nothing else, for a `rocprofv3 --kernel-trace` run of its
own; `--kernel-trace-csv FILE` folds that trace into the JSON by kernel name per case (no GPU needed).
Nothing here is a threshold."""
import argparse
import csv
import json
import os
import platform
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
SEED = 1
KERNELS = ("k_bake_atlas_count", "k_bake_atlas_cover", "k_bake_atlas_sample", "k_bake_blocks", "k_bake_list_count", "k_bake_list", "k_trace_occlusion_listed",
           "k_occlusion_resolve_listed", "k_bake_dilate", "DeviceScan", "scan")


def fold_trace(path, cases):
    """per case (in launch order, one k_bake_atlas_count each) the microseconds of each kernel, summed over its launches in the case"""
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    out, cur = [], None
    for start, end, name in rows:
        if "k_bake_atlas_count" in name:
            cur = {}
            out.append(cur)
        if cur is None:
            continue
        key = next((k for k in KERNELS if k in name), "other")
        key = "scan" if key == "DeviceScan" else key
        cur[key + "_us"] = cur.get(key + "_us", 0.0) + (end - start) / 1e3
    return [{"case": c, **k} for c, k in zip(cases, out)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 4096])
    ap.add_argument("--full-sizes", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--rays", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--kernel-trace-csv", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bake_atlas_timing.json"))
    args = ap.parse_args()
    quarter_cases = [(which, size, n) for which in ("floor", "quad") for size in args.sizes for n in args.rays]
    if args.kernel_trace_csv:
        with open(args.out) as f:
            res = json.load(f)
        res["kernels_us"] = {"what": "rocprofv3 --kernel-trace of --trace-run: one bake_atlas_occlusion(margin = 16) per quarter case, microseconds per kernel",
                             "cases": fold_trace(args.kernel_trace_csv, ["/".join(map(str, c)) for c in quarter_cases])}
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        return
    import numpy as np
    import torch

    import hala_renderer_amd as H
    from bake_timing import scene_with_ceiling
    from multihit_timing import renderer_on
    A = H._abi
    scene, where, instance = scene_with_ceiling(H)
    mine = H.HalaRenderer("atlas-timing", 64, 64, 5, 3, False, False, False, 0)
    mine.set_build_options(instancing=False)
    mine.set_scene(scene)
    mine.commit()
    eps = float(mine.ray_eps())
    stream = torch.cuda.Stream()
    parent = None
    if args.parent_root and not args.trace_run:
        parent = renderer_on(H, os.path.join(os.path.abspath(args.parent_root), "hala-renderer_amd", "lib", "libhalart.so"), "atlas-timing-parent")
        parent.set_build_options(instancing=False)
        parent.set_scene(scene)
        parent.commit()
    res = {"what": "bake atlases (scripts/bake_atlas_timing.py): GPU ms between two HIP events on device buffers",
           "box": {"gpu": torch.cuda.get_device_name(0), "host": platform.processor() or platform.machine(), "hip": torch.version.hip},
           "parent_library": bool(parent), "rounds": args.rounds, "warmup": args.warmup, "cases": {}}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def measure(name, variants, summary=None):
        ms = {v: [] for v, _ in variants}
        for rnd in range(args.warmup + args.rounds):
            for v, fn in variants:
                x = timed(fn)
                if rnd >= args.warmup:
                    ms[v].append(x)
        row = {v: {"ms": x, "median_ms": statistics.median(x), "spread_ms": max(x) - min(x)} for v, x in ms.items()}
        stream.synchronize()
        if summary:
            row["summary"] = summary()
        res["cases"][name] = row
        print(name, json.dumps({v: [round(row[v]["median_ms"], 4), round(row[v]["spread_ms"], 4)] for v, _ in variants}), json.dumps(row.get("summary")), flush=True)

    def chart(which, scale, offset):
        return (instance[which], (scale, scale), offset, False, which == "floor")

    def set_parent_uvs(factor):
        if parent is None:
            return
        for k, (m, p) in where.items():
            v = scene.meshes[m].primitives[p].vertices.copy()
            v["tex_coord"] = v["tex_coord"] * np.float32(factor)
            parent.update_vertices(m, p, v)
        parent.refit()

    big = max(args.sizes + args.full_sizes)
    d_s = torch.zeros(big * big * 32, dtype=torch.uint8, device="cuda")
    d_o = torch.zeros(big * big * 16, dtype=torch.uint8, device="cuda")
    d_o2 = torch.zeros(big * big * 16, dtype=torch.uint8, device="cuda")
    d_t = torch.zeros(big * big * 16, dtype=torch.uint8, device="cuda")
    kw = dict(bias=eps, stream=stream.cuda_stream)

    if args.trace_run:
        for which, size, n_rays in quarter_cases:
            mine.bake_atlas_occlusion([chart(which, 0.5, (0.0, 0.0))], size, size, n_rays, SEED, margin=16, out=d_o, out_texels=d_t, **kw)
            stream.synchronize()
        mine.close()
        return

    # ---- the chart fills the map: plain pass against listed pass ------------------------------------------------------------------------
    for which in ("floor", "quad"):
        inst, flip = instance[which], which == "floor"
        for size in args.full_sizes:
            for n_rays in args.rays:
                variants = [("plain_whole", lambda: mine.bake_occlusion(inst, size, size, n_rays, SEED, flip=flip, out=d_o, out_texels=d_t, **kw)),
                            ("listed_whole", lambda: mine.bake_atlas_occlusion([chart(which, 1.0, (0.0, 0.0))], size, size, n_rays, SEED, out=d_o2, out_texels=d_t, **kw))]
                if parent:
                    variants.insert(0, ("parent_whole", lambda: parent.bake_occlusion(inst, size, size, n_rays, SEED, flip=flip, out=d_o, out_texels=d_t, **kw)))

                def same():
                    n = size * size * 16
                    return {"listed_equals_plain": bool(torch.equal(d_o[:n], d_o2[:n]))}
                measure(f"full/{which}/{size}/{n_rays}", variants, same)

    # ---- a quarter of the map: the parent's pass over every texel against the listed pass -------------------------------------------------
    set_parent_uvs(0.5)
    for which, size, n_rays in quarter_cases:
        inst, flip, count, half = instance[which], which == "floor", size * size, size // 2
        table = [chart(which, 0.5, (0.0, 0.0))]
        variants = [("atlas_samples", lambda: mine.bake_atlas_samples(table, size, size, out=d_s, out_texels=d_t, **kw)),
                    ("atlas_whole", lambda: mine.bake_atlas_occlusion(table, size, size, n_rays, SEED, out=d_o2, out_texels=d_t, **kw)),
                    ("half_full", lambda: mine.bake_occlusion(inst, half, half, n_rays, SEED, flip=flip, out=d_o, out_texels=d_t, **kw))]
        if parent:
            variants += [("parent_samples", lambda: parent.bake_samples(inst, size, size, flip=flip, out=d_s, out_texels=d_t, **kw)),
                         ("parent_occlusion", lambda: parent.occlusion(d_s, rays=n_rays, seed=SEED, out=d_o, count=count, stream=stream.cuda_stream)),
                         ("parent_whole", lambda: parent.bake_occlusion(inst, size, size, n_rays, SEED, flip=flip, out=d_o, out_texels=d_t, **kw))]

        def summary():
            n = count * 16
            tex = d_t[:n].cpu().numpy().view(A.BAKE_TEXEL_DTYPE)
            return {"texels": count, "owned_share": float((tex["prim"] != 0xFFFFFFFF).mean()),
                    "atlas_equals_parent": bool(torch.equal(d_o[:n], d_o2[:n])) if parent else None}
        measure(f"quarter/{which}/{size}/{n_rays}", variants, summary)

    # ---- two instances in one atlas against two parent calls ----------------------------------------------------------------------------
    for size in args.sizes:
        for n_rays in args.rays:
            table = [chart("floor", 0.5, (0.0, 0.0)), chart("quad", 0.5, (0.5, 0.5))]
            variants = [("atlas_whole", lambda: mine.bake_atlas_occlusion(table, size, size, n_rays, SEED, out=d_o2, out_texels=d_t, **kw))]
            if parent:
                def two_calls():
                    parent.bake_occlusion(instance["floor"], size, size, n_rays, SEED, flip=True, out=d_o, out_texels=d_t, **kw)
                    parent.bake_occlusion(instance["quad"], size, size, n_rays, SEED, out=d_o, out_texels=d_t, **kw)
                variants.append(("parent_two_calls", two_calls))
            measure(f"both/{size}/{n_rays}", variants)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    if parent:
        parent.close()
    mine.close()


if __name__ == "__main__":
    main()
