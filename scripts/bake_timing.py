"""Time bake maps (hala_rt_bake_samples / hala_rt_bake_occlusion, docs/RENDER_SPEC.md 4.11) on configs[3] (the ~1 M-triangle atrium,
committed flattened) and write profiles/bake_timing.json.

Two instances are baked: the tessellated floor (instance 0, 120 k small triangles, one chart over [0, 1]^2; its triangles wind downwards,
so it is baked with the flip) and a quad added to the scene as a ceiling above the walls (the last instance: two triangles as large as
the map, wound downwards too, baked as it is: its rays go down into the atrium), into 1024^2, 2048^2 and 4096^2 maps with N = 16 and 64
rays per texel, bias = ray_eps, reach +inf.  First with the charts as they are (they fill the map), then with the
same charts scaled to a quarter of it (UVs halved by update_vertices + refit): three quarters of the texels are then empty.
Variants, `--rounds` times after `--warmup` rounds, alternating, each timed call directly behind an untimed call of the same variant,
between two HIP events on one stream, all buffers on the device:
  samples     r.bake_samples(): owner-map clear, block counts, prefix sum, coverage, samples and texel records
  occlusion   r.occlusion() on the sample buffer bake_samples left: the occlusion pass alone
  bake_m0     r.bake_occlusion(margin=0): the whole call without dilation
  bake_m16    r.bake_occlusion(margin=16): the whole call; bake_m16 - bake_m0 is the dilation pass
The kernels of the first pass apart (coverage beside samples) come from a kernel trace: `--kernel-trace-csv FILE` folds the per-dispatch
rows of a `rocprofv3 --kernel-trace` run of this script (with --rounds 1 --warmup 0 --no-host) into the JSON, by kernel name per case.
What empty texels cost the occlusion pass: occlusion on the quarter chart at W x W beside occlusion on the full chart at W/2 x W/2 (the
same covered texels at the same density, no empty ones).
The workaround a host has without the operator, on the PARENT's library (--parent-root: the parent commit's tree, built there; without it
this tree's library, and the JSON says so), on the host's clock from nothing to the records in host memory: rasterise the UV layout with
the numpy twin's edge functions (tests/bake_ref.py; boxes per triangle, vectorised over the triangles), interpolate points and normals,
r.occlusion() on host arrays (upload of 32 B per texel, read-back of 16 B), no gutter fill; beside it the whole call in its host form,
r.bake_occlusion() to host arrays.  At N = 16, maps of --host-sizes.
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
SEED = 1
KERNELS = ("k_bake_count", "k_bake_cover", "k_bake_sample", "k_trace_occlusion", "k_occlusion_resolve", "k_bake_blocks", "k_bake_dilate")


def scene_with_ceiling(H):
    """configs[3] plus one quad over the whole room at y = 12.5, its normal down like the floor's: -> (scene, (mesh, primitive) of floor and quad, their instances)"""
    import numpy as np
    from hala_renderer_amd import scenes, workloads
    scene = workloads.baseline_config(3)["scene"]
    room = next(nd.mesh_index for nd in scene.nodes if nd.name == "room")
    quad = scenes._grid_mesh(1, 1, lambda u, v: np.stack([u * 40.0 - 20.0, 12.5 + 0.0 * u, v * 24.0 - 12.0], 1))
    quad.material_index = 0
    scene.meshes.append(H.HalaMesh([quad]))
    scene.nodes.append(H.HalaNode(name="ceiling", parent=0, mesh_index=len(scene.meshes) - 1))
    instances = sum(len(scene.meshes[nd.mesh_index].primitives) for nd in scene.nodes if nd.mesh_index != H._abi.INVALID_INDEX)
    first = next(k for k, nd in enumerate(nd for nd in scene.nodes if nd.mesh_index != H._abi.INVALID_INDEX) if nd.name == "room")
    assert first == 0
    return scene, {"floor": (room, 0), "quad": (len(scene.meshes) - 1, 0)}, {"floor": 0, "quad": instances - 1}


def host_raster(BR, uv, first, w, h):
    """the owner of every texel (0xffffffff: none) by the twin's rule, the candidates of a triangle bounded by its box: triangles up to 32
    texels wide are tested together, offset by offset of their boxes; larger ones one by one over their own box"""
    import numpy as np
    f32 = np.float32
    t = (uv * np.array([w, h], f32)).astype(f32)
    ax, ay, bx, by, cx, cy = (t[:, k, c] for k in range(3) for c in range(2))
    area = BR.edge(ax, ay, bx, by, cx, cy)
    x0 = np.clip(np.floor(t[:, :, 0].min(axis=1)) - 1, 0, w - 1).astype(np.int64); x1 = np.clip(np.floor(t[:, :, 0].max(axis=1)), 0, w - 1).astype(np.int64)
    y0 = np.clip(np.floor(t[:, :, 1].min(axis=1)) - 1, 0, h - 1).astype(np.int64); y1 = np.clip(np.floor(t[:, :, 1].max(axis=1)), 0, h - 1).astype(np.int64)
    owner = np.full(w * h, 0xFFFFFFFF, dtype=np.uint32)
    ids = (np.arange(len(uv)) + first).astype(np.uint32)

    def fold(sel, px, py, xi, yi, ok):
        a = [z[sel] if np.ndim(px) == 1 else z[sel][:, None] for z in (ax, ay, bx, by, cx, cy)]
        ar = area[sel] if np.ndim(px) == 1 else area[sel][:, None]
        cov = ok & BR.covers(ar, BR.edge(a[2], a[3], a[4], a[5], px, py), BR.edge(a[4], a[5], a[0], a[1], px, py), BR.edge(a[0], a[1], a[2], a[3], px, py))
        tri = ids[sel] if np.ndim(px) == 1 else np.broadcast_to(ids[sel][:, None], cov.shape)
        np.minimum.at(owner, (yi * w + xi)[cov], tri[cov])
    small = np.nonzero((x1 - x0 < 32) & (y1 - y0 < 32))[0]
    if len(small):
        for dy in range(int((y1 - y0)[small].max()) + 1):
            for dx in range(int((x1 - x0)[small].max()) + 1):
                xi, yi = x0[small] + dx, y0[small] + dy
                fold(small, xi.astype(f32) + f32(0.5), yi.astype(f32) + f32(0.5), xi, yi, (xi <= x1[small]) & (yi <= y1[small]))
    for k in np.nonzero(~((x1 - x0 < 32) & (y1 - y0 < 32)))[0]:
        yi, xi = np.mgrid[y0[k]:y1[k] + 1, x0[k]:x1[k] + 1]
        xi, yi = xi.reshape(1, -1), yi.reshape(1, -1)
        fold(np.array([k]), xi.astype(f32) + f32(0.5), yi.astype(f32) + f32(0.5), xi, yi, np.ones(xi.shape, bool))
    return owner, t, area


def host_samples(BR, A, owner, t, area, first, tris, w, h, bias, flip):
    """points and (geometric) normals at the owned texels, as a host would interpolate them"""
    import numpy as np
    f32 = np.float32
    v0, e1, e2 = tris
    owned = owner != 0xFFFFFFFF
    k = np.where(owned, owner - np.uint32(first), 0).astype(np.int64)
    px, py = BR.centres(w, h)
    c = [t[k, i, j] for i in range(3) for j in range(2)]
    with np.errstate(all="ignore"):
        inv = f32(1.0) / area[k]
        u = BR.edge(c[4], c[5], c[0], c[1], px, py) * inv
        v = BR.edge(c[0], c[1], c[2], c[3], px, py) * inv
    g = k + first
    s = np.zeros(w * h, dtype=A.OCCLUSION_SAMPLE_DTYPE)
    s["point"] = np.where(owned[:, None], v0[g] + e1[g] * u[:, None] + e2[g] * v[:, None], 0)
    n = np.cross(e1[g], e2[g])
    s["normal"] = np.where(owned[:, None], -n if flip else n, 0)
    s["bias"], s["reach"] = np.where(owned, bias, 0), np.where(owned, np.inf, 0)
    return s


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
        key = next((k for k in KERNELS if k in name), "other_us")
        cur[key if key == "other_us" else key + "_us"] = cur.get(key if key == "other_us" else key + "_us", 0.0) + (end - start) / 1e3
    return [{"case": c, **k} for c, k in zip(cases, out)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048, 4096])
    ap.add_argument("--rays", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--host-sizes", type=int, nargs="+", default=[1024])
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--trace-run", action="store_true", help="one bake_occlusion(margin=16) per case and nothing else: what a kernel trace should see")
    ap.add_argument("--kernel-trace-csv", default=None, help="fold the kernel trace of a --trace-run into --out and exit (no GPU needed)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bake_timing.json"))
    args = ap.parse_args()
    cases = [(phase, which, size, n) for phase in ("full", "quarter") for which in ("floor", "quad") for size in args.sizes for n in args.rays]
    if args.kernel_trace_csv:
        with open(args.out) as f:
            res = json.load(f)
        res["kernels_us"] = {"what": "rocprofv3 --kernel-trace of --trace-run: one bake_occlusion(margin = 16) per case, microseconds per kernel",
                             "cases": fold_trace(args.kernel_trace_csv, ["/".join(map(str, c)) for c in cases])}
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        return
    import numpy as np
    import torch

    import bake_ref as BR
    import closest_point_ref as CR
    import hala_renderer_amd as H
    from multihit_timing import renderer_on
    A = H._abi
    scene, where, instance = scene_with_ceiling(H)
    parent_lib = os.path.join(os.path.abspath(args.parent_root), "hala-renderer_amd", "lib", "libhalart.so") if args.parent_root else None
    mine = H.HalaRenderer("bake-timing", 64, 64, 5, 3, False, False, False, 0)
    mine.set_build_options(instancing=False)
    mine.set_scene(scene)
    mine.commit()
    info = mine.bvh_info()
    assert info.instance_ref_count == 0
    eps = float(mine.ray_eps())
    stream = torch.cuda.Stream()
    res = {"what": "bake maps (scripts/bake_timing.py): GPU ms between two HIP events on device buffers; host ms on the host's clock",
           "box": {"gpu": torch.cuda.get_device_name(0), "host": platform.processor() or platform.machine(), "hip": torch.version.hip},
           "workaround_library": "parent" if parent_lib else "this tree (no --parent-root)", "rounds": args.rounds, "warmup": args.warmup,
           "scene": {"triangles": int(info.triangle_count), "floor_triangles": int(len(scene.meshes[where["floor"][0]].primitives[0].indices) // 3)},
           "cases": {}, "host": {}}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    rest = {k: scene.meshes[m].primitives[p].vertices.copy() for k, (m, p) in where.items()}
    for phase in ("full", "quarter"):
        for k, (m, p) in where.items():
            v = rest[k].copy()
            if phase == "quarter":
                v["tex_coord"] = v["tex_coord"] * np.float32(0.5)
            mine.update_vertices(m, p, v)
        mine.refit()
        for which in ("floor", "quad"):
            inst, flip = instance[which], which == "floor"
            for size in args.sizes:
                count = size * size
                d_s = torch.zeros(count * 32, dtype=torch.uint8, device="cuda")
                d_o = torch.zeros(count * 16, dtype=torch.uint8, device="cuda")
                d_t = torch.zeros(count * 16, dtype=torch.uint8, device="cuda")
                for n_rays in args.rays:
                    kw = dict(flip=flip, bias=eps, out_texels=d_t, stream=stream.cuda_stream)
                    variants = [("samples", lambda: mine.bake_samples(inst, size, size, out=d_s, **kw)),
                                ("occlusion", lambda: mine.occlusion(d_s, rays=n_rays, seed=SEED, out=d_o, count=count, stream=stream.cuda_stream)),
                                ("bake_m0", lambda: mine.bake_occlusion(inst, size, size, n_rays, SEED, margin=0, out=d_o, **kw)),
                                ("bake_m16", lambda: mine.bake_occlusion(inst, size, size, n_rays, SEED, margin=16, out=d_o, **kw))]
                    if args.trace_run:
                        variants[3][1]()
                        stream.synchronize()
                        continue
                    ms = {v: [] for v, _ in variants}
                    for rnd in range(args.warmup + args.rounds):
                        for v, fn in variants:
                            x = timed(fn)
                            if rnd >= args.warmup:
                                ms[v].append(x)
                    row = {v: {"ms": x, "median_ms": statistics.median(x), "spread_ms": max(x) - min(x)} for v, x in ms.items()}
                    stream.synchronize()
                    tex = d_t.cpu().numpy().view(A.BAKE_TEXEL_DTYPE)
                    rec = d_o.cpu().numpy().view(A.OCCLUSION_DTYPE)
                    owned = tex["prim"] != 0xFFFFFFFF
                    row["summary"] = {"texels": count, "owned_share": float(owned.mean()), "filled_by_dilation": int(((tex["source"] != 0xFFFFFFFF) & ~owned).sum()),
                                      "mean_visibility_of_owned": float(rec["visibility"][owned].astype(np.float64).mean()) if owned.any() else None,
                                      "dilation_ms": row["bake_m16"]["median_ms"] - row["bake_m0"]["median_ms"],
                                      "mrays_per_s_of_owned": float(owned.sum()) * n_rays / row["occlusion"]["median_ms"] / 1e3}
                    res["cases"]["/".join(map(str, (phase, which, size, n_rays)))] = row
                    print(phase, which, size, n_rays, json.dumps({**{v: round(row[v]["median_ms"], 4) for v, _ in variants}, **row["summary"]}), flush=True)
                del d_s, d_o, d_t
        if phase == "full" and not args.no_host and not args.trace_run:
            other = renderer_on(H, parent_lib, "bake-timing-parent") if parent_lib else mine
            if other is not mine:
                other.set_build_options(instancing=False)
                other.set_scene(scene)
                other.commit()
            tris = CR.bvh_triangles(mine.download_bvh()[1])
            firsts = np.cumsum([0] + [len(pr.indices) // 3 for nd in scene.nodes if nd.mesh_index != A.INVALID_INDEX for pr in scene.meshes[nd.mesh_index].primitives])
            for which in ("floor", "quad"):
                m, p = where[which]
                pr = scene.meshes[m].primitives[p]
                uv = np.ascontiguousarray(pr.vertices["tex_coord"], dtype=np.float32)[np.asarray(pr.indices, np.int64).reshape(-1, 3)]
                first = int(firsts[instance[which]])
                for size in args.host_sizes:
                    t0 = time.perf_counter()
                    owner, t, area = host_raster(BR, uv, first, size, size)
                    t1 = time.perf_counter()
                    samples = host_samples(BR, A, owner, t, area, first, tris, size, size, eps, which == "floor")
                    t2 = time.perf_counter()
                    rec = other.occlusion(samples, rays=16, seed=SEED)
                    t3 = time.perf_counter()
                    got_r, got_t = mine.bake_occlusion(instance[which], size, size, 16, SEED, flip=which == "floor", bias=eps)
                    t4 = time.perf_counter()
                    row = {"raster_ms": (t1 - t0) * 1e3, "interpolate_ms": (t2 - t1) * 1e3, "occlusion_upload_readback_ms": (t3 - t2) * 1e3,
                           "workaround_ms": (t3 - t0) * 1e3, "bake_occlusion_host_form_ms": (t4 - t3) * 1e3,
                           "owners_equal": bool(np.array_equal(owner, got_t["prim"].reshape(-1))),
                           "visibility_max_abs_diff": float(np.abs(rec["visibility"] - got_r["visibility"].reshape(-1)).max())}
                    res["host"][f"{which}/{size}/16"] = row
                    print("host", which, size, json.dumps(row), flush=True)
            if other is not mine:
                other.close()
        if not args.trace_run:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
    mine.close()


if __name__ == "__main__":
    main()
