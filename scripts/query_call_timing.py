"""Time the host side of small query batches: what a device-form call costs the caller, where the batch itself is next to nothing.

Three cases on the Cornell box with two charted carpets (a one-level tree staged in LDS), device buffers, the renderer's own stream:
  closest_points   64 queries
  occlusion        64 samples x 16 rays, the renderer's own mask buffer
  bake_atlas       a 16 x 16 atlas of the two carpets x 16 rays
A round is `--calls` back-to-back device-form calls and ONE synchronisation at the end, timed with the host clock around both; the
figure is microseconds per call.  With --parent-root (the parent commit's tree, built there) the parent's package — its renderer.py over
its own library — and this tree's run every round alternately in one process, the one that goes first alternating too; the JSON keeps
every round, the median and the spread (max - min) of both sides.  The margin for a difference is the parent's own spread.
The renderer that is created second measured 4-6 us per call slower than the first whichever build it was (--parent-root . runs this
tree against itself and shows it: the second renderer's stream), which is more than either side's spread: compare the builds over two
runs, one of them with --this-first, so that each is once the first."""
import argparse
import importlib.util
import json
import os
import platform
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = 11


def load_package(root, name):
    """the package of the tree at `root` under the module name `name` (its LIB_PATH is its own tree's library)"""
    d = os.path.join(os.path.abspath(root), "hala-renderer_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def carpets(H):
    """scenes.cornell_box() with two 4 x 4 grids over the floor as instances 6 and 7, UVs in [0, 1]^2"""
    import numpy as np
    from importlib import import_module
    scenes = import_module(H.__name__ + ".scenes")
    s = scenes.cornell_box()
    for k, lift in enumerate((2.0, 60.0)):
        p = scenes._grid_mesh(4, 4, lambda u, v: np.stack([2.0 * u - 1.0, 0.0 * u, 1.0 - 2.0 * v], 1))
        p.material_index = 0
        m = np.diag([200.0, 1.0, 200.0, 1.0]).astype(np.float32)
        m[:3, 3] = (278.0, lift, 280.0)
        s.meshes.append(H.HalaMesh([p]))
        s.nodes.append(H.HalaNode(name=f"carpet{k}", mesh_index=len(s.meshes) - 1, local_transform=m))
    return s


def cases(H, r, torch):
    """name -> a function that makes one device-form call"""
    import numpy as np
    A = H._abi
    rng = np.random.RandomState(3)
    q = np.zeros(64, dtype=A.POINT_QUERY_DTYPE)
    q["point"] = rng.uniform(20.0, 535.0, size=(64, 3))
    q["radius"] = np.inf
    n = rng.normal(size=(64, 3))
    s = np.zeros(64, dtype=A.OCCLUSION_SAMPLE_DTYPE)
    s["point"] = rng.uniform(20.0, 535.0, size=(64, 3))
    s["normal"] = n / np.linalg.norm(n, axis=1, keepdims=True)
    s["bias"] = 0.05
    s["reach"] = 150.0
    d_q, d_s = (torch.from_numpy(a.view(np.uint8).copy()).cuda() for a in (q, s))
    d_cp = torch.zeros(64 * 32, dtype=torch.uint8, device="cuda")
    d_ao = torch.zeros(64 * 16, dtype=torch.uint8, device="cuda")
    d_map = torch.zeros(256 * 16, dtype=torch.uint8, device="cuda")
    d_tex = torch.zeros(256 * 16, dtype=torch.uint8, device="cuda")
    charts = r._bake_charts([(6, (0.5, 0.5), (0.0, 0.0)), (7, (0.5, 0.5), (0.5, 0.5))])
    torch.cuda.synchronize()
    return {"closest_points": lambda: r.closest_points(d_q, out=d_cp),
            "occlusion": lambda: r.occlusion(d_s, rays=16, seed=SEED, out=d_ao),
            "bake_atlas": lambda: r.bake_atlas_occlusion(charts, 16, 16, 16, SEED, bias=0.05, reach=150.0, out=d_map, out_texels=d_tex)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--this-first", action="store_true", help="create this tree's renderer (and run its first round) ahead of the parent's")
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_call_timing.json"))
    args = ap.parse_args()
    import torch

    import hala_renderer_amd as H
    if not torch.cuda.is_available():
        raise SystemExit("query_call_timing.py needs a GPU: a call cost is measured, not estimated")
    sides = {"this": H}
    if args.parent_root:
        sides["parent"] = load_package(args.parent_root, "hala_renderer_amd_parent")
    if not args.this_first:
        sides = dict(reversed(list(sides.items())))
    runs = {}
    for side, pkg in sides.items():
        pkg.load_library()
        r = pkg.HalaRenderer("call-timing-" + side, 64, 64, 5, 3, False, False, False, 0)
        r.set_build_options(instancing=False)
        r.set_scene(carpets(pkg))
        r.commit()
        runs[side] = (r, cases(pkg, r, torch))
    res = {"what": "host side of small query batches (scripts/query_call_timing.py): microseconds per device-form call, "
                   f"{args.calls} back-to-back calls and one synchronisation, host clock",
           "box": {"gpu": torch.cuda.get_device_name(0), "host": platform.processor() or platform.machine(), "hip": torch.version.hip},
           "libraries": {side: pkg.LIB_PATH.replace(ROOT, ".") for side, pkg in sides.items()},
           "created_first": next(iter(sides)), "calls": args.calls, "rounds": args.rounds, "warmup": args.warmup, "cases": {}}
    for name in ("closest_points", "occlusion", "bake_atlas"):
        us = {side: [] for side in runs}
        for rnd in range(args.warmup + args.rounds):
            for side, (r, fns) in (list(runs.items()) if rnd % 2 == 0 else reversed(list(runs.items()))):  # who goes first alternates too
                fn = fns[name]
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    fn()
                r.wait_idle()
                dt = time.perf_counter() - t0
                if rnd >= args.warmup:
                    us[side].append(dt / args.calls * 1e6)
        res["cases"][name] = {side: {"us_per_call": v, "median_us": statistics.median(v), "spread_us": max(v) - min(v)} for side, v in us.items()}
        print(name, {side: (round(c["median_us"], 2), round(c["spread_us"], 2)) for side, c in res["cases"][name].items()}, flush=True)
    for r, _ in runs.values():
        r.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
