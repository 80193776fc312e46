"""Time shutter motion blur (hala_rt_set_shutter, docs/RENDER_SPEC.md 18) and write profiles/shutter_timing.json and the measured block of DESIGN.md 18.

configs[3] (atrium) at 1920 x 1080, 4 frames per call.  One session is one process with one renderer; within it the variants alternate,
`--blocks` times, `--calls` calls each, and every figure is a median with its spread.  GPU ms are taken between two HIP events on the
renderer's stream around the call (a step waits on the host, so the events span it); host ms are wall time until the stream is idle.
  (a) update_batch(4) with the shutter off and with it on but inactive (no key): the same code path.  With --parent-root a session of the
      parent commit's library (built there; it has no shutter and runs both variants "off") alternates with this build's, `--rounds`
      times: the parent's spread is the margin for the difference.
  (b) update_batch(4) with the shutter active at stride 4 (one step per call) and stride 1 (four): one node key on the instance that
      scripts/temporal_timing.py moves; vertex keys and deformer keys on the largest primitive (the rig of tests/deform_ref.py).
  (c) one step against hala_rt_refit on the same node edit, host ms: update_batch(1) with a step minus update_batch(1) without one.
  (d) k_shutter_lerp alone, from the kernel trace of `--child` (the vertex-key loop in a process of its own under
      `rocprofv3 --kernel-trace --output-format csv`): 132 B per vertex moved, next to k_deform's figure of profiles/deform_timing.json."""
import argparse
import csv
import glob
import json
import os
import platform
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# a --session of the parent's library imports the parent's package
PKG_ROOT = os.path.abspath(sys.argv[sys.argv.index("--package-root") + 1]) if "--package-root" in sys.argv[:-1] else ROOT
sys.path.insert(0, PKG_ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))  # deform_ref (needs the test tree): the rig, the poses and the posed array of the vertex keys

import numpy as np  # noqa: E402

import deform_ref as D  # noqa: E402
import hala_renderer_amd as H  # noqa: E402
from hala_renderer_amd import workloads  # noqa: E402

W, HGT, SPP = 1920, 1080, 4
TARGETS, JOINTS = 2, 32


def summary(xs):
    return {"median": statistics.median(xs), "mean": statistics.fmean(xs), "min": min(xs), "max": max(xs), "stdev": statistics.pstdev(xs), "calls": len(xs)}


def translate(t):
    m = np.eye(4, dtype=np.float32)
    m[:3, 3] = t
    return m


def events(r, fn, calls):
    """GPU ms of each of `calls` calls of fn(), between two HIP events on the renderer's stream (stream_handle() joins the second frame slot)"""
    import torch
    out = []
    for _ in range(calls):
        stream = torch.cuda.ExternalStream(r.stream_handle())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        stream = torch.cuda.ExternalStream(r.stream_handle())
        e1.record(stream)
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def wall(r, fn, calls):
    out = []
    for _ in range(calls):
        r.wait_idle()
        t0 = time.perf_counter()
        fn()
        r.wait_idle()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def moved_instance(r):
    """(node, instance) of the instance that covers the most pixels among those covering less than 15 % of the frame: an object, not a wall"""
    ids = r.read_ids()
    inst = ids[..., 1][ids[..., 1] != 0xFFFFFFFF]
    counts = np.bincount(inst)
    counts[counts > 0.15 * ids.shape[0] * ids.shape[1]] = 0
    k = int(np.argmax(counts))
    return int(ids[..., 0][ids[..., 1] == k][0]), k


def setup():
    cfg = workloads.baseline_config(3)
    scene = cfg["scene"]
    r = H.HalaRenderer("shutter-timing", W, HGT, cfg["max_depth"], cfg["rr_depth"], False, False, False, 0)
    if cfg["env"] is not None:
        r.set_envmap(cfg["env"], 0.0)
    r.set_scene(scene)
    r.commit()
    r.set_launch_timing_period(0)
    return r, scene


def largest_primitive(scene):
    mesh, prim = max(((m, p) for m in range(len(scene.meshes)) for p in range(len(scene.meshes[m].primitives))),
                     key=lambda mp: len(scene.meshes[mp[0]].primitives[mp[1]].vertices))
    rest = scene.meshes[mesh].primitives[prim].vertices
    pos = rest["position"].astype(np.float64)
    extent = float(np.ptp(pos, axis=0).max())
    rig = D.random_rig(len(rest), targets=TARGETS, joint_count=JOINTS, normals=True, seed=17, scale=0.02 * extent)
    poses = [D.random_pose(rig, seed=k, zero_some=False, centre=0.5 * (pos.min(0) + pos.max(0)), scale=0.05 * extent) for k in (1, 2)]
    return mesh, prim, rest, rig, poses


def session(blocks, calls):
    """one process, one renderer -> the figures of (a), (b) and (c)"""
    r, scene = setup()
    has_feature = hasattr(r, "set_shutter")
    out = {"shutter_available": has_feature, "a": [], "b": [], "c": []}
    r.update_batch(SPP); r.render()
    batch = lambda: (r.update_batch(SPP), r.render())  # noqa: E731
    # (a) off / on but inactive, alternating
    for k in range(2 * blocks):
        variant = ("off", "inactive")[k % 2]
        if has_feature:
            r.set_shutter(None) if variant == "off" else r.set_shutter()
        r.refit()
        batch()
        out["a"].append({"variant": variant, "gpu_ms": summary(events(r, batch, calls))})
    if not has_feature:
        r.close()
        return out
    # (b) active: node, vertex and deformer keys at strides 4 and 1, alternating
    r.set_aovs(position=False, ids=True)
    r.update_batch(1)
    node, inst = moved_instance(r)
    r.set_aovs(position=False, ids=False)
    info = r.bvh_info()
    extent = float(max(b - a for a, b in zip(info.scene_min, info.scene_max)))
    m0 = np.asarray(scene.nodes[node].local_transform, np.float32)
    m1 = m0 @ translate((0.01 * extent, 0.0, 0.005 * extent))
    mesh, prim, rest, rig, poses = largest_primitive(scene)
    out["primitive"] = {"mesh": mesh, "primitive": prim, "vertices": len(rest), "scene_triangles": int(info.triangle_count)}
    out["moved"] = {"node": node, "instance": inst}

    def clear():
        r.set_node_keys(node, None, None)
        r.set_vertex_keys(mesh, prim, None, None)
        try:
            r.set_deformer_keys(mesh, prim, None, None)
        except H.HalaRendererError:
            pass  # no deformer registered
        r.set_shutter(None)
        r.refit()
        try:
            r.clear_deformer(mesh, prim)
        except H.HalaRendererError:
            pass
        r.update_vertices(mesh, prim, rest)
        r.refit()

    def keys_node():
        r.set_node_keys(node, m0, m1)

    def keys_vertices():
        r.set_vertex_keys(mesh, prim, rest, close_vertices)

    def keys_deformer():
        r.set_deformer(mesh, prim, **rig)
        r.set_deformer_keys(mesh, prim, open=poses[0], close=poses[1])

    close_vertices = D.pose_vertices(rest, rig, poses[0])
    for b in range(blocks):
        for name, setter in (("node", keys_node), ("vertices", keys_vertices), ("deformer", keys_deformer)):
            for stride in (4, 1):
                clear()
                setter()
                r.set_shutter(time_stride=stride)
                r.refit()
                batch()
                before = r.shutter_status().steps
                gpu = events(r, batch, calls)
                out["b"].append({"keys": name, "stride": stride, "gpu_ms_per_4_frames": summary(gpu),
                                 "steps_per_call": (r.shutter_status().steps - before) / calls})
    # (c) one step against the refit on the same node edit (host ms)
    clear()
    for b in range(blocks):
        refit_ms = []
        for k in range(calls):
            r.update_node_transform(node, m1 if k % 2 == 0 else m0)
            refit_ms += wall(r, r.refit, 1)
        r.update_node_transform(node, m0); r.refit()
        one = lambda: (r.update_batch(1), r.render())  # noqa: E731
        one()
        still = wall(r, one, calls)
        keys_node(); r.set_shutter(time_stride=1); r.refit()
        one()
        before = r.shutter_status().steps
        stepped = wall(r, one, calls)
        steps = r.shutter_status().steps - before
        clear()
        out["c"].append({"refit_host_ms": summary(refit_ms), "update_1_frame_host_ms": summary(still), "update_1_frame_with_a_step_host_ms": summary(stepped),
                         "steps": steps, "step_host_ms_by_difference_of_medians": statistics.median(stepped) - statistics.median(still)})
    r.close()
    return out


def child(calls):
    r, scene = setup()
    mesh, prim, rest, rig, poses = largest_primitive(scene)
    r.set_vertex_keys(mesh, prim, rest, D.pose_vertices(rest, rig, poses[0]))
    r.set_shutter()
    r.refit()
    for _ in range(calls):
        r.update_batch(1)
    r.wait_idle()
    r.close()


def kernel_trace(calls):
    """-> the durations (ms) of every k_shutter_lerp launch of a --child run under rocprofv3"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "t", "--", sys.executable, os.path.abspath(__file__), "--child", str(calls)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            raise RuntimeError(f"the traced run failed ({p.returncode}): {p.stderr[-2000:]}")
        out = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    if "k_shutter_lerp" in row["Kernel_Name"]:
                        out.append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6)
    if not out:
        raise RuntimeError("the kernel trace holds no k_shutter_lerp launch")
    return out


def run_session(root, blocks, calls):
    env = dict(os.environ)
    env.pop("HALART_LIB", None)
    root = os.path.abspath(root)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--session", "--blocks", str(blocks), "--calls", str(calls), "--package-root", root],
                       cwd=root, env=env, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise RuntimeError(f"the session in {root} failed ({p.returncode}): {p.stderr[-2000:]}")
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


BEGIN, END = "<!-- shutter_timing.py: begin -->", "<!-- shutter_timing.py: end -->"


def design_text(res):
    """the figures of a result file as the paragraph between the two markers of DESIGN.md 18"""
    this = [s for s in res["sessions"] if s["library"] == "this"]
    a = res["a_summary"]
    ms = lambda x: f"{x:.3f}"  # noqa: E731
    out = [f"(`scripts/shutter_timing.py` -> `profiles/shutter_timing.json`; {res['box']['gpu']}, HIP {res['box']['hip']}; configs[3] at {W} x {HGT}, "
           f"{SPP} frames per call, medians of block medians.)", ""]
    par = "no parent session" if a["parent_median"] is None else f"parent commit's library {ms(a['parent_median'])} ms with a spread of {ms(a['parent_spread'])} ms over its blocks"
    out += [f"- (a) `update_batch(4)`: shutter off {ms(a['this_off'])} ms, on but inactive {ms(a['this_inactive'])} ms, difference {a['difference']:+.3f} ms; "
            f"spread of this build's blocks {ms(a['this_spread'])} ms; {par}."]
    rows = {}
    for s in this:
        for b in s.get("b", []):
            rows.setdefault((b["keys"], b["stride"]), []).append((b["gpu_ms_per_4_frames"]["median"], b["steps_per_call"]))
    for (keys, stride), v in sorted(rows.items()):
        m = [x for x, _ in v]
        out += [f"- (b) {keys} keys, stride {stride}: {ms(statistics.median(m))} ms per 4 frames (blocks {ms(min(m))} ... {ms(max(m))}), {v[0][1]:g} step(s) per call."]
    c = [x for s in this for x in s.get("c", [])]
    if c:
        med = lambda k: statistics.median(x[k]["median"] for x in c)  # noqa: E731
        spread = max(x["refit_host_ms"]["max"] for x in c) - min(x["refit_host_ms"]["min"] for x in c)
        out += [f"- (c) host ms: `hala_rt_refit` on the node edit {ms(med('refit_host_ms'))} (its calls span {ms(spread)}); a one-frame update {ms(med('update_1_frame_host_ms'))}, "
                f"with a step {ms(med('update_1_frame_with_a_step_host_ms'))}: a step costs {ms(statistics.median(x['step_host_ms_by_difference_of_medians'] for x in c))} by difference."]
    if "d_k_shutter_lerp_ms" in res:
        d, g = res["d_k_shutter_lerp_ms"], res["d_k_shutter_lerp_gb_per_s"]
        nv = next(s["primitive"]["vertices"] for s in this if "primitive" in s)
        out += [f"- (d) `k_shutter_lerp` alone on {nv} vertices: median {d['median'] * 1e3:.1f} us, min {d['min'] * 1e3:.1f} us over {d['calls']} launches: "
                f"{g['at_median']:.0f} GB/s at the median, {g['at_min']:.0f} GB/s at the minimum, by the 132-B model; `k_deform`'s figure of "
                f"`profiles/deform_timing.json`: {json.dumps(res.get('k_deform_gb_per_s_of_profiles_deform_timing'))}."]
    return "\n".join(out)


def write_design(res):
    path = os.path.join(ROOT, "DESIGN.md")
    text = open(path).read()
    a, b = text.index(BEGIN) + len(BEGIN), text.index(END)
    with open(path, "w") as f:
        f.write(text[:a] + "\n" + design_text(res) + "\n" + text[b:])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=24)
    ap.add_argument("--blocks", type=int, default=2, help="rounds of the variants per session")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--session", action="store_true", help="one session in this process: prints its figures as one JSON line")
    ap.add_argument("--package-root", default=None)
    ap.add_argument("--child", type=int, default=0, help="only run the vertex-key loop with this many one-frame updates (what the kernel trace wraps)")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--design-from", default=None, help="only rewrite the measured block of DESIGN.md 18 from this result file")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shutter_timing.json"))
    args = ap.parse_args()
    if args.design_from:
        with open(args.design_from) as f:
            write_design(json.load(f))
        return
    H.load_library()
    if args.child:
        child(args.child)
        return
    if args.session:
        print(json.dumps(session(args.blocks, args.calls)))
        return
    import torch
    res = {"what": f"shutter motion blur (scripts/shutter_timing.py): configs[3] at {W} x {HGT}, {SPP} frames per call; medians over the blocks of every session",
           "box": {"gpu": torch.cuda.get_device_name(0), "host": platform.processor() or platform.machine(), "hip": torch.version.hip}, "sessions": []}

    def save():  # after every stage: a later one that fails keeps the earlier figures
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)

    for k in range(args.rounds):
        order = [("parent", args.parent_root), ("this", ROOT)] if args.parent_root else [("this", ROOT)]
        for name, root in (order if k % 2 == 0 else order[::-1]):
            res["sessions"].append({"library": name, **run_session(root, args.blocks, args.calls)})
            save()

    def medians(lib, variant):
        return [b["gpu_ms"]["median"] for s in res["sessions"] if s["library"] == lib for b in s["a"] if b["variant"] == variant]

    a = {lib: {v: medians(lib, v) for v in ("off", "inactive")} for lib in ("this", "parent")}
    res["a_block_medians_gpu_ms"] = a
    every = {lib: a[lib]["off"] + a[lib]["inactive"] for lib in a}
    res["a_summary"] = {"this_off": statistics.median(a["this"]["off"]), "this_inactive": statistics.median(a["this"]["inactive"]),
                        "difference": statistics.median(a["this"]["inactive"]) - statistics.median(a["this"]["off"]),
                        "parent_median": statistics.median(every["parent"]) if every["parent"] else None,
                        "parent_spread": max(every["parent"]) - min(every["parent"]) if every["parent"] else None,
                        "this_spread": max(every["this"]) - min(every["this"])}
    save()
    if not args.no_trace:
        ms = kernel_trace(args.calls)
        nv = next(s["primitive"]["vertices"] for s in res["sessions"] if "primitive" in s)
        res["d_k_shutter_lerp_ms"] = summary(ms)
        res["d_k_shutter_lerp_gb_per_s"] = {"bytes_per_vertex": 132, "at_median": 132 * nv / (statistics.median(ms) * 1e-3) / 1e9, "at_min": 132 * nv / (min(ms) * 1e-3) / 1e9}
        try:
            with open(os.path.join(ROOT, "profiles", "deform_timing.json")) as f:
                res["k_deform_gb_per_s_of_profiles_deform_timing"] = json.load(f).get("c_k_deform_gb_per_s")
        except OSError:
            pass
        save()
    print(json.dumps({k: v for k, v in res.items() if k != "sessions"}, indent=1))
    if os.path.abspath(args.out) == os.path.join(ROOT, "profiles", "shutter_timing.json"):
        write_design(res)


if __name__ == "__main__":
    main()
