"""Overlap of a frame's tail with the next frame's camera-ray launch, from a rocprofv3 --kernel-trace CSV.

The tail of a frame = the traversal launches between its last k_shade and its k_resolve, plus that k_resolve (in dispatch order).  For
every k_trace_primary that follows such a tail: how long before the tail's end the camera-ray launch started (> 0: they overlapped), and
the interval from one camera-ray launch to the next.   usage: python scripts/tail_overlap.py <kernel_trace.csv> [label]"""
import csv
import statistics
import sys


def frames(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Dispatch_Id"]))
    out, tail, prev_primary = [], [], None
    for r in rows:
        name, s, e = r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        if "k_shade" in name:
            tail = []
        elif "k_trace_shadow" in name or "k_trace_batch" in name or "k_resolve" in name:
            tail.append((s, e, r.get("Queue_Id", "?")))
        elif "k_trace_primary" in name:
            if prev_primary is not None and tail:
                tail_end = max(e_ for _, e_, _ in tail)
                out.append({"lead_us": (tail_end - s) / 1e3, "period_us": (s - prev_primary) / 1e3,
                            "tail_us": (tail_end - min(s_ for s_, _, _ in tail)) / 1e3,
                            "queues": (tail[-1][2], r.get("Queue_Id", "?"))})
            prev_primary = s
    return out


def main():
    path, label = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else "")
    fr = frames(path)
    if not fr:
        sys.exit("no frame with a tail followed by a camera-ray launch in " + path)
    over = sum(f["lead_us"] > 0 for f in fr)
    print(f"{label}: {len(fr)} frame boundaries; the next k_trace_primary started before the tail (last shadow launch + k_resolve) "
          f"ended at {over} of them")
    print(f"  tail (first tail launch start -> resolve end): median {statistics.median(f['tail_us'] for f in fr):.1f} us")
    print(f"  camera-ray launch started before the tail's end by: median {statistics.median(f['lead_us'] for f in fr):.1f} us, "
          f"min {min(f['lead_us'] for f in fr):.1f}, max {max(f['lead_us'] for f in fr):.1f}")
    print(f"  queues (tail, next primary): {sorted(set(f['queues'] for f in fr))}")
    for i, f in enumerate(fr):
        print(f"  {i:3d}  lead {f['lead_us']:8.1f} us  tail {f['tail_us']:7.1f} us  primary-to-primary {f['period_us']:9.1f} us")


if __name__ == "__main__":
    main()
