"""Generates tests/golden/sweep_host_golden.json: what every chain of tests/sweep_host_cases.py returns with the library of the commit
the fixture pins -- the parent of the commit that gave the sweep's host side one plan, named stages and one prior fill for both widths
(csrc/sweep_plan.hpp, csrc/jwas_hip.hip).  Run on the GPU with that commit's library:

    python tests/golden/make_sweep_host_golden.py --commit HASH [--lib path/to/libjwas_hip.so] [--out FILE] [--same-as FILE]

HASH names the commit whose library is loaded; the fixture records it.  --same-as FILE: after writing, compare case by case with an
earlier writing and exit non-zero naming the cases that differ (the fixture is written twice, by two processes, and only a chain that
comes out the same both times is pinned by hash).

tests/test_gpu_sweep_host_golden.py replays the same chains on the current library and requires equal values and digests."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", ".."), os.path.join(HERE, "..")]
import sweep_host_cases as G  # noqa: E402
from jwas_jl_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True)
    ap.add_argument("--lib", default="")
    ap.add_argument("--out", default=os.path.join(HERE, "sweep_host_golden.json"))
    ap.add_argument("--same-as", default="")
    args = ap.parse_args()
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    try:
        import torch
        rocm = str(torch.version.hip)
    except Exception:
        rocm = "unknown"
    blob = {"commit": args.commit, "rocm": rocm, "cases": {}}
    for name in G.CASES:
        blob["cases"][name] = G.run_case(name)
        print("ran", name, flush=True)
    with open(args.out, "w") as fh:
        json.dump(blob, fh, separators=(",", ":"), sort_keys=True)
        fh.write("\n")
    print("wrote", args.out, os.path.getsize(args.out), "bytes")
    if args.same_as:
        with open(args.same_as) as fh:
            other = json.load(fh)["cases"]
        differ = [k for k in blob["cases"] if blob["cases"][k] != other.get(k)]
        print("cases that differ between the two writings:", differ or "none")
        return 1 if differ else 0
    return 0


if __name__ == "__main__":
    sys.exit(main())
