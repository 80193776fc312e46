"""Two updates in flight, from a rocprofv3 --kernel-trace CSV: which kernels of two different updates were resident together.

An update = the launches of one queue from a k_trace_primary to the next k_resolve (k_crypto_fold included), in dispatch order.  Per
update: its span, and for how long one of its kernels ran while a kernel of ANOTHER update ran (the union of those intervals).  Per kernel
symbol: the median duration of the launches that ran alone and of those that ran beside a kernel of another update, and with which
symbols they shared the chip.   usage: python scripts/frame_overlap.py <kernel_trace.csv> [label]"""
import collections
import csv
import re
import statistics
import sys

FRAME_KERNELS = ("k_trace_primary", "k_trace_batch", "k_trace_shadow", "k_shade", "k_resolve", "k_crypto_fold")


def symbol(name):
    m = re.search(r"(k_[a-z_]+)(<[a-z]+)?", name)
    base = m.group(1) if m else name
    if base == "k_shade":  # the camera-ray shade and the bounce shades are different kernels in all but name
        return "k_shade<true>" if "k_shade<true" in name.replace(" ", "") else "k_shade<false>"
    return base


def updates(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Dispatch_Id"]))
    open_, out = {}, []
    for r in rows:
        name = r["Kernel_Name"]
        if not any(k in name for k in FRAME_KERNELS):
            continue
        q = r.get("Queue_Id", "?")
        k = (symbol(name), int(r["Start_Timestamp"]), int(r["End_Timestamp"]))
        if "k_trace_primary" in name:
            open_[q] = {"queue": q, "kernels": [k]}
            out.append(open_[q])
        elif q in open_:
            open_[q]["kernels"].append(k)
    return [u for u in out if any(s == "k_resolve" for s, _, _ in u["kernels"])]


def union_length(iv):
    total, end = 0, None
    for s, e in sorted(iv):
        if end is None or s > end:
            total += e - s
            end = e
        elif e > end:
            total += e - end
            end = e
    return total


def main():
    path, label = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else "")
    ups = updates(path)
    if len(ups) < 2:
        sys.exit("fewer than two updates in " + path)
    alone, beside, partners = collections.defaultdict(list), collections.defaultdict(list), collections.defaultdict(collections.Counter)
    shared = []
    for i, u in enumerate(ups):
        near = [k for j in (i - 2, i - 1, i + 1, i + 2) if 0 <= j < len(ups) for k in ups[j]["kernels"]]
        iv = []
        for sym, s, e in u["kernels"]:
            hit = [(max(s, s2), min(e, e2), sym2) for sym2, s2, e2 in near if min(e, e2) > max(s, s2)]
            (beside if hit else alone)[sym].append((e - s) / 1e3)
            iv += [(a, b) for a, b, _ in hit]
            for _, _, sym2 in hit:
                partners[sym][sym2] += 1
        span = (max(e for _, _, e in u["kernels"]) - min(s for _, s, _ in u["kernels"])) / 1e3
        shared.append((span, union_length(iv) / 1e3, u["queue"]))
    starts = [min(s for _, s, _ in u["kernels"]) for u in ups]
    periods = [(b - a) / 1e3 for a, b in zip(starts, starts[1:])]
    print(f"{label}: {len(ups)} updates on queues {sorted(set(q for _, _, q in shared))}; update start to next update start: median "
          f"{statistics.median(periods):.1f} us")
    print(f"  span of an update: median {statistics.median(s for s, _, _ in shared):.1f} us; of it beside kernels of another update: median "
          f"{statistics.median(o for _, o, _ in shared):.1f} us, max {max(o for _, o, _ in shared):.1f} us; updates that shared the chip: "
          f"{sum(o > 0 for _, o, _ in shared)}")
    print("  per symbol: launches and median duration alone | beside a kernel of another update (with which)")
    for sym in sorted(set(alone) | set(beside)):
        a, b = alone.get(sym, []), beside.get(sym, [])
        fa = f"{len(a):4d} x {statistics.median(a):8.1f} us" if a else "   0 x        - us"
        fb = f"{len(b):4d} x {statistics.median(b):8.1f} us" if b else "   0 x        - us"
        print(f"    {sym:28s} {fa} | {fb}  {dict(partners[sym].most_common(3)) if b else ''}")
    for i, (span, o, q) in enumerate(shared):
        print(f"  {i:3d}  queue {q}  span {span:9.1f} us  beside another update {o:8.1f} us")


if __name__ == "__main__":
    main()
