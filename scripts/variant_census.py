#!/usr/bin/env python3
"""Which compiled kernel instantiations does the GPU suite launch when tests/test_kernel_variants.py is left out?

Resets the library's variant ledger (hala_rt_variant_ledger), runs the GPU tier of tests/ in this process without that module, and prints,
per kernel family, the built instantiations that no test launched, by their flag values.  Evidence for what that module adds, not a test.

  python scripts/variant_census.py [-o profiles/variant_census.txt] [extra pytest arguments]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--output", help="also write the report to this file")
    args, extra = ap.parse_known_args()
    import pytest

    import hala_renderer_amd as H
    families = H._abi.VARIANT_FAMILIES
    for f in range(len(families)):
        H.variant_ledger(f, reset=True)
    os.chdir(ROOT)
    rc = pytest.main(["tests", "-m", "gpu", "--deselect", "tests/test_kernel_variants.py"] + extra)
    lines = [f"GPU tier of tests/ without tests/test_kernel_variants.py: pytest exit code {int(rc)}", ""]
    total_built = total_missed = 0
    for f, (name, flags) in enumerate(families):
        launched, built = H.variant_ledger(f)
        missed = [i for i in range(64) if ((built & ~launched) >> i) & 1]
        total_built += bin(built).count("1"); total_missed += len(missed)
        lines.append(f"{name}: {bin(built).count('1')} built, {bin(built & launched).count('1')} launched, {len(missed)} never launched")
        for i in missed:
            lines.append("    " + name + "<" + ", ".join(f"{fl}={(i >> k) & 1}" for k, fl in enumerate(flags)) + ">")
    lines += ["", f"total: {total_missed} of {total_built} built instantiations never launched"]
    report = "\n".join(lines) + "\n"
    print(report, end="")
    if args.output:
        with open(args.output, "w") as fh:
            fh.write(report)
    return 0 if int(rc) == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
