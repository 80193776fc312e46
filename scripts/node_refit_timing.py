"""Time hala_rt_refit_nodes (docs/RENDER_SPEC.md 20) against the ordinary sequence and write profiles/node_refit_timing.json.

The scene is the one of scripts/instance_levels_timing.py: N instances of one 1 280-triangle blob, N = 1 024, 16 384 and 131 072, a
two-level tree with the instance levels built on the GPU, the automatic builder and LBVH.  Every figure is host wall time in ms until
the renderer's stream is idle, for moving ALL N nodes, the median of --reps calls:
  a   N x hala_rt_update_node_transform + hala_rt_refit   (through ctypes with prepared matrices; a_calls is the share of the N calls)
  b   hala_rt_refit_nodes from a numpy array
  c   hala_rt_refit_nodes from a device tensor produced on the renderer's stream
With --parent-root (the parent commit's tree, built there) variant a also runs on the parent's library, --parent-rounds sessions per N with
the automatic builder; their spread is the margin of the comparisons in the summary.  This build's automatic builder runs as many sessions
(the first is the one the table quotes for b and c; the summary compares the median of its a with the parent's)."""
import argparse
import ctypes as C
import json
import os
import platform
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from instance_levels_timing import HGT, SIZES, W, scene_of  # noqa: E402


def session(n, builder, variants, reps):
    """one library, one N, one builder in this process; a JSON line per variant"""
    import numpy as np
    sys.path.insert(0, os.getcwd())
    import hala_renderer_amd as H
    lib = H.load_library()
    s = scene_of(H, n)
    r = H.HalaRenderer("nodes", W, HGT, 5, 3, False, False, False, 0)
    r.set_build_options(instancing=True, builder=builder, instance_levels="gpu")
    r.set_scene(s)
    r.commit()
    base = np.stack([np.asarray(nd.local_transform, dtype=np.float32) for nd in s.nodes[:n]])
    step = [0]

    def next_pose():
        step[0] += 1
        m = base.copy()
        m[:, 0, 3] += np.float32(0.25 * (step[0] % 5))
        return m

    def timed(fn):
        r.wait_idle()
        t0 = time.perf_counter()
        fn()
        r.wait_idle()
        return (time.perf_counter() - t0) * 1e3

    def say(name, **kw):
        print(json.dumps(dict(variant=name, **kw)), flush=True)

    med = statistics.median
    if "a" in variants:
        fn = lib.hala_rt_update_node_transform
        fn.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        total, calls = [], []
        for _ in range(reps + 1):
            cols = np.ascontiguousarray(next_pose().transpose(0, 2, 1))
            ptr = cols.ctypes.data
            r.wait_idle()
            t0 = time.perf_counter()
            for k in range(n):
                fn(r._h, k, ptr + 64 * k)
            t1 = time.perf_counter()
            r.refit()
            r.wait_idle()
            t2 = time.perf_counter()
            total.append((t2 - t0) * 1e3); calls.append((t1 - t0) * 1e3)
        say("a", ms=med(total[1:]), calls_ms=med(calls[1:]), all=total[1:])
    if "b" in variants or "c" in variants:
        r.bind_nodes(list(range(n)))
    if "b" in variants:
        t = [timed(lambda m=next_pose(): r.refit_nodes(m)) for _ in range(reps + 1)]
        st = r.node_refit_status()
        say("b", ms=med(t[1:]), all=t[1:], last_path=st.last_path, last_reason=st.last_reason)
    if "c" in variants:
        import torch
        ext = torch.cuda.ExternalStream(r.get_stream())
        d_base = torch.from_numpy(np.ascontiguousarray(base.transpose(0, 2, 1)).reshape(n, 16)).cuda()
        shift = torch.zeros(16, dtype=torch.float32)
        shift[12] = 0.25
        d_shift = shift.cuda()
        torch.cuda.synchronize()

        def from_device(k):
            with torch.cuda.stream(ext):
                d = d_base + d_shift * float(k % 5)
                r.refit_nodes(d)

        t = [timed(lambda k=k: from_device(k)) for k in range(reps + 1)]
        st = r.node_refit_status()
        say("c", ms=med(t[1:]), all=t[1:], last_path=st.last_path, last_reason=st.last_reason)
    r.close()


def run_session(root, n, builder, variants, reps, cap):
    env = dict(os.environ)
    env.pop("HALART_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--session", "--n", str(n), "--builder", builder or "auto", "--variants", variants, "--reps", str(reps)]
    t0 = time.perf_counter()
    try:
        p = subprocess.run(cmd, cwd=os.path.abspath(root), env=env, capture_output=True, text=True, timeout=cap)
    except subprocess.TimeoutExpired:
        return {"not finished": f"capped after {cap} s"}, time.perf_counter() - t0
    if p.returncode != 0:
        raise RuntimeError(f"the session {cmd[3:]} in {root} failed ({p.returncode}): {p.stderr[-2000:]}")
    res = {}
    for ln in p.stdout.splitlines():
        if ln.startswith("{"):
            d = json.loads(ln)
            res[d.pop("variant")] = d
    return res, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--builders", nargs="*", default=["auto", "lbvh"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cap", type=float, default=240.0, help="wall seconds one session may take")
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--parent-rounds", type=int, default=3)
    ap.add_argument("--session", action="store_true", help="one library, N and builder in this process")
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--builder", default="auto")
    ap.add_argument("--variants", default="abc")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "node_refit_timing.json"))
    args = ap.parse_args()
    if args.session:
        session(args.n, None if args.builder == "auto" else args.builder, args.variants, args.reps)
        return
    import torch
    res = {"what": "hala_rt_refit_nodes against N x hala_rt_update_node_transform + hala_rt_refit (scripts/node_refit_timing.py): all N instances of a "
                   "1 280-triangle blob move; host wall ms until the stream is idle, median of the calls after a warm-up call",
           "box": {"gpu": torch.cuda.get_device_name(0), "host": platform.processor() or platform.machine(), "hip": torch.version.hip}, "sizes": {}}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)

    for n in args.sizes:
        rows = res["sizes"].setdefault(str(n), {})
        for b in args.builders:
            rows[b], wall = run_session(ROOT, n, None if b == "auto" else b, "abc", args.reps, args.cap)
            print(f"N={n} {b}: {wall:.1f} s " + " ".join(f"{k}={v.get('ms')}" for k, v in rows[b].items() if isinstance(v, dict)), flush=True)
            save()
        rows["auto again"] = []
        for k in range(1, args.parent_rounds if args.parent_root else 1):
            one, wall = run_session(ROOT, n, None, "a", args.reps, args.cap)
            rows["auto again"].append(one)
            print(f"N={n} auto #{k}: {wall:.1f} s a={one.get('a', {}).get('ms')}", flush=True)
            save()
        if args.parent_root:
            rows["parent auto"] = []
            for k in range(args.parent_rounds):
                one, wall = run_session(args.parent_root, n, None, "a", args.reps, args.cap)
                rows["parent auto"].append(one)
                print(f"N={n} parent auto #{k}: {wall:.1f} s a={one.get('a', {}).get('ms')}", flush=True)
                save()
    out = {}
    for n in args.sizes:
        rows = res["sizes"][str(n)]
        parent = [x["a"]["ms"] for x in rows.get("parent auto", []) if "a" in x]
        mine = rows.get("auto", {})
        get = lambda v: mine.get(v, {}).get("ms")  # noqa: E731
        a_runs = [x for x in [get("a")] + [x.get("a", {}).get("ms") for x in rows.get("auto again", [])] if x is not None]
        o = {"parent a runs": parent, "a runs": a_runs, "a": statistics.median(a_runs) if a_runs else None, "b": get("b"), "c": get("c")}
        if len(parent) > 1 and None not in (o["a"], o["b"], o["c"]):
            spread, mid = max(parent) - min(parent), statistics.median(parent)
            o["margin (spread of the parent's runs)"] = spread
            o["b faster than the parent's a by more than the margin"] = mid - o["b"] > spread
            o["c faster than the parent's a by more than the margin"] = mid - o["c"] > spread
            o["a equals the parent's a within the margin"] = min(parent) - spread <= o["a"] <= max(parent) + spread
        out[str(n)] = o
    res["summary"] = out
    save()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
