#!/usr/bin/env python3
"""Static instruction census of one kernel of the path tracer (trace_closest.hip, trace_shadow.hip, shade.hip, resolve.hip),
attributed to source functions and lines (no GPU needed).
Compiles the unit that defines the kernel with -gline-tables-only into a scratch directory, disassembles the gfx950 code object with source
line markers and counts instructions per inlined function and per line, by kind: vector ALU, LDS, vector memory, and — a wave issues
one instruction of ANY kind at a time, so they cost its stream as much — scalar ALU / scalar memory, branches and waits.  The kind is read
off the mnemonic's prefix alone (v_, ds_, global_/buffer_/flat_/scratch_, s_cbranch/s_branch/s_setpc/s_call, s_waitcnt/s_nop/s_barrier/
s_sleep, s_load/s_buffer_load, everything else on s_ is scalar ALU).  This is how the node step of traverse.h was put on its diet in
round 3 (profiles/r03_experiments.txt) and its control flow in profiles/scalar_diet.txt: the counts are static — a branch that is rarely
taken counts in full — so read them next to the PMC figures of profiles/*_pmc_*.txt.

usage: scripts/isa_attr.py '<mangled-name prefix or demangled substring>' [source file to list the top lines of] [-D... passed to hipcc]
  e.g. scripts/isa_attr.py _ZN2rt7k_shadeILb0ELb0ELb0E shading.h
       scripts/isa_attr.py 'k_trace_shadow_then_batch<false, false, false>' traverse.h
"""
import bisect
import collections
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hala-renderer_amd", "csrc")
LLVM = "/opt/rocm/lib/llvm/bin"
UNITS = ("trace_closest.hip", "trace_shadow.hip", "shade.hip", "resolve.hip")


KINDS = ("valu", "lds", "vmem", "salu", "smem", "branch", "wait")
SCALAR_SIDE = ("salu", "smem", "branch", "wait")


def kind_of(mnemonic):
    """by prefix only"""
    if mnemonic.startswith("v_"):
        return "valu"
    if mnemonic.startswith("ds_"):
        return "lds"
    if mnemonic.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if mnemonic.startswith(("s_cbranch", "s_branch", "s_setpc", "s_swappc", "s_call", "s_endpgm")):
        return "branch"
    if mnemonic.startswith(("s_waitcnt", "s_nop", "s_barrier", "s_sleep")):
        return "wait"
    if mnemonic.startswith(("s_load", "s_buffer_load")):
        return "smem"
    return "salu"


def code_object(obj, out):
    data = open(obj, "rb").read()
    i = data.find(b"__CLANG_OFFLOAD_BUNDLE__")
    cnt = struct.unpack_from("<Q", data, i + 24)[0]
    off = i + 32
    for _ in range(cnt):
        eo, es, ts = struct.unpack_from("<QQQ", data, off); off += 24
        triple = data[off:off + ts].decode(); off += ts
        if "gfx" in triple:
            open(out, "wb").write(data[i + eo:i + eo + es])
            return
    raise SystemExit("no gfx code object in " + obj)


def functions(path):
    out = []
    for n, l in enumerate(open(path), 1):
        m = re.search(r"RT_DI\s+[\w:<>\*& ]+?\s+(\w+)\s*\(", l) or re.search(r"\)\s+(k_\w+)\(", l) or re.match(r"^__global__.*\s(k_\w+)\(", l)
        if m and not l.strip().startswith("//"):
            out.append((n, m.group(1)))
    return out


def unit_of(want):
    """the unit that defines the kernel `want` names (a mangled name holds the kernel's name, too)"""
    m = re.search(r"k_[a-z_]+", want)
    for unit in UNITS:
        if m and re.search(r"\b%s\(" % m.group(0), open(os.path.join(CSRC, unit)).read()):
            return unit
    raise SystemExit("no unit of " + ", ".join(UNITS) + " defines a kernel named in " + want)


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    defines = [a for a in sys.argv[1:] if a.startswith("-D")]
    sys.argv = [a for a in sys.argv if not a.startswith("-D")]
    want = sys.argv[1]
    tmp = tempfile.mkdtemp(prefix="isa_attr_")
    obj = os.path.join(tmp, "unit.o")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-mfma",
                           "-gline-tables-only", *defines, "-x", "hip", "-c", os.path.join(CSRC, unit_of(want)), "-o", obj])
    co = os.path.join(tmp, "unit.co")
    code_object(obj, co)
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "-l", "--mcpu=gfx950", co], capture_output=True, text=True, check=True).stdout.split("\n")
    start = end = None
    for i, l in enumerate(dis):
        m = re.match(r"^[0-9a-f]+ <(.*)>:", l)
        if not m:
            continue
        name = m.group(1)
        pretty = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        if start is None and (name.startswith(want) or want in pretty):
            start = i
            print("kernel:", pretty[:160])
        elif start is not None:
            end = i
            break
    if start is None:
        raise SystemExit("no kernel matches " + want)
    cur = None
    by_line = collections.defaultdict(collections.Counter)
    kinds = collections.Counter()
    for l in dis[start:end]:
        m = re.match(r"^; (/[^:]+):(\d+)", l)
        if m:
            cur = (os.path.basename(m.group(1)), int(m.group(2)))
            continue
        t = l.strip().split()
        if t and "//" in l:
            k = kind_of(t[0])
            kinds[k] += 1
            by_line[cur][k] += 1
    print("instructions:", {k: kinds[k] for k in KINDS}, "scalar side:", sum(kinds[k] for k in SCALAR_SIDE))
    src = {f: functions(os.path.join(CSRC, f)) for f in os.listdir(CSRC) if f.endswith((".h", ".hip"))}
    by_fn = collections.defaultdict(collections.Counter)
    for k, c in by_line.items():
        if k is None:
            by_fn[("?", "?")].update(c)
            continue
        fl = src.get(k[0], [])
        idx = bisect.bisect_right([x[0] for x in fl], k[1]) - 1
        by_fn[(k[0], fl[idx][1] if idx >= 0 else "?")].update(c)
    head = "   all " + " ".join(f"{k:>6s}" for k in KINDS)
    row = lambda c: f"{sum(c.values()):6d} " + " ".join(f"{c[k]:6d}" for k in KINDS)
    print("instructions by (inlined) function:")
    print(head)
    for k, c in sorted(by_fn.items(), key=lambda x: -sum(x[1].values()))[:40]:
        print(f"{row(c)}  {k[0]}:{k[1]}")
    if len(sys.argv) > 2:
        print("top lines of", sys.argv[2])
        print(head)
        for k, c in sorted(by_line.items(), key=lambda x: -sum(x[1].values())):
            if k and k[0] == sys.argv[2]:
                print(f"{row(c)}  {k[0]}:{k[1]}")
                if sum(c.values()) < 8:
                    break


if __name__ == "__main__":
    main()
