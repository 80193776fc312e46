"""Time recomputed normals of deformed meshes (hala_rt_set_deformer_normals, docs/RENDER_SPEC.md 17 "Recomputed normals") and write
profiles/deform_normals_timing.json.

The setup of scripts/deform_timing.py: configs[3], its largest primitive, the same rig (2 morph targets + 32 joints).  Per pose change,
over `--poses` poses, host wall time until the renderer's stream is idle, on three renderers of the same scene, the order of the three
alternating from one pose to the next:
  (a) update_deformer + refit in mode 0: k_deform, the refit;
  (b) the same in mode 1: k_deform, the face pass, the vertex pass, the refit;
  (c) the workaround without the feature: the posed vertices and their normals made on the host (tests/deform_ref.py and
      tests/deform_normals_ref.py), update_vertices, refit — with and without the host's arithmetic in the time;
  (d) the two normals kernels alone, from the kernel trace of `--child` (the (b) loop in a process of its own under
      `rocprofv3 --kernel-trace --output-format csv`), with the achieved GB/s against the byte model of DESIGN.md 20."""
import argparse
import csv
import glob
import json
import os
import platform
import re
import statistics
import subprocess
import sys
import tempfile
import time


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))    # deform_ref, deform_normals_ref: the twins make the arrays of (c)
sys.path.insert(0, os.path.join(ROOT, "scripts"))  # deform_timing: the scene, the primitive, the rig and the poses

import deform_normals_ref as N  # noqa: E402
import deform_ref as D  # noqa: E402
import deform_timing as T  # noqa: E402
import hala_renderer_amd as H  # noqa: E402

KERNELS = ("k_deform_faces", "k_deform_vertex_normals")


def model_bytes(vertices, triangles):
    """DESIGN.md 20.  Face pass, per triangle: 12 B of indices, 3 x 12 B of positions, 16 B written.  Vertex pass, per vertex: 4 B class,
    8 B of offsets, 12 B tangent read, 24 B written; per list entry (3 per triangle): 4 B entry + 16 B face record"""
    return {"face_pass": triangles * (12 + 36 + 16), "vertex_pass": vertices * (4 + 8 + 12 + 24) + 3 * triangles * (4 + 16)}


def child(poses):
    r, _, mesh, prim, _, rig, centre, extent = T.setup()
    r.set_deformer(mesh, prim, **rig)
    r.set_deformer_normals(mesh, prim, 1)
    for k in range(poses):
        r.update_deformer(mesh, prim, **T.pose_of(rig, k, centre, extent))
        r.refit()
    r.wait_idle()
    r.close()


def kernel_trace(poses):
    """-> {kernel: durations (ms) of its launches} of a --child run under rocprofv3"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "t", "--", sys.executable, os.path.abspath(__file__), "--child", str(poses)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            raise RuntimeError(f"the traced run failed ({p.returncode}): {p.stderr[-2000:]}")
        out = {k: [] for k in KERNELS}
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    for k in KERNELS:
                        if re.search(r"\b" + k + r"\(", row["Kernel_Name"]):
                            out[k].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6)
    if not all(out.values()):
        raise RuntimeError("the kernel trace lacks a normals kernel")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--poses", type=int, default=24)
    ap.add_argument("--child", type=int, default=0, help="only run the (b) loop with this many poses (what the kernel trace wraps)")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deform_normals_timing.json"))
    args = ap.parse_args()
    H.load_library()
    if args.child:
        child(args.child)
        return
    import torch
    res = {"what": "recomputed normals (scripts/deform_normals_timing.py): one pose change of the largest primitive of configs[3], "
                   f"{T.TARGETS} morph targets + {T.JOINTS} joints; host wall ms until the stream is idle; the order of (a), (b), (c) rotates per pose",
           "box": {"gpu": torch.cuda.get_device_name(0), "host": platform.processor() or platform.machine(), "hip": torch.version.hip}}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)

    ra, scene, mesh, prim, rest, rig, centre, extent = T.setup()
    rb, rc = T.setup()[0], T.setup()[0]
    idx = scene.meshes[mesh].primitives[prim].indices
    nv, nt = len(rest), len(idx) // 3
    model = model_bytes(nv, nt)
    res["primitive"] = {"mesh": mesh, "primitive": prim, "vertices": nv, "triangles": nt, "model_bytes_per_pose": model}
    t0 = time.perf_counter()
    cl = N.classes(rest, idx)
    res["host_twin_classes_ms"] = (time.perf_counter() - t0) * 1e3
    poses = [T.pose_of(rig, k, centre, extent) for k in range(args.poses + 2)]
    for r in (ra, rb):
        r.set_deformer(mesh, prim, **rig)
    t0 = time.perf_counter()
    rb.set_deformer_normals(mesh, prim, 1)
    res["set_deformer_normals_ms"] = (time.perf_counter() - t0) * 1e3
    info = rb.get_deformer_normals(mesh, prim)
    res["primitive"].update(classes=info.class_count, entries=info.entry_count)

    def host_array(p):
        return N.recompute(D.pose_vertices(rest, rig, p), idx, cl)

    def run_a(p):
        return T.timed(ra, lambda: (ra.update_deformer(mesh, prim, **p), ra.refit()))

    def run_b(p):
        return T.timed(rb, lambda: (rb.update_deformer(mesh, prim, **p), rb.refit()))

    def run_c(p):
        t0 = time.perf_counter()
        v = host_array(p)
        host = (time.perf_counter() - t0) * 1e3
        return host, T.timed(rc, lambda: (rc.update_vertices(mesh, prim, v), rc.refit()))

    for p in poses[:2]:  # warm-up: first launches, allocations
        run_a(p); run_b(p); run_c(p)
    a, b, c_host, c_upload = [], [], [], []
    for k, p in enumerate(poses[2:]):
        for which in ("abc", "bca", "cab")[k % 3]:
            if which == "a":
                a.append(run_a(p))
            elif which == "b":
                b.append(run_b(p))
            else:
                h, u = run_c(p)
                c_host.append(h); c_upload.append(u)
    want = host_array(poses[-1])
    res["kernels_equal_the_twin_on_the_last_pose"] = bool(rb.read_vertices(mesh, prim).tobytes() == want.tobytes())
    res["a_mode0_update_deformer_refit_ms"] = T.summary(a)
    res["b_mode1_update_deformer_refit_ms"] = T.summary(b)
    res["c_update_vertices_refit_ms"] = T.summary(c_upload)
    res["c_host_twin_ms"] = T.summary(c_host)
    res["c_total_ms"] = T.summary([h + u for h, u in zip(c_host, c_upload)])
    res["b_minus_a_median_ms"] = res["b_mode1_update_deformer_refit_ms"]["median"] - res["a_mode0_update_deformer_refit_ms"]["median"]
    for r in (ra, rb, rc):
        r.close()
    save()
    if not args.no_trace:
        ms = kernel_trace(args.poses)
        res["d_kernels_ms"] = {k: T.summary(v) for k, v in ms.items()}
        res["d_kernels_gb_per_s_at_median"] = {"k_deform_faces": model["face_pass"] / (statistics.median(ms["k_deform_faces"]) * 1e-3) / 1e9,
                                               "k_deform_vertex_normals": model["vertex_pass"] / (statistics.median(ms["k_deform_vertex_normals"]) * 1e-3) / 1e9}
        save()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
