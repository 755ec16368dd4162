"""Generates tests/golden/session_golden.json: what every device session (tests/session_golden_cases.py) computes with the library
of the commit the fixture pins -- the parent of the commit that moved the sessions out of csrc/jwas_hip.hip.  Run once on the GPU
with that commit's library:

    python tests/golden/make_session_golden.py --commit HASH [--lib path/to/libjwas_hip.so] [--cases block|output|mtj] [--out FILE]

HASH names the commit whose library is loaded; the fixture records it.  --cases block writes tests/golden/block_session_golden.json
instead: the sessions with a block sweep of their own (BLOCK_CASES), pinned to the parent of the commit that gave them one copy of
their shared code.  --cases output writes tests/golden/output_side_golden.json: the output side of a context (OUTPUT_CASES), pinned to the
parent of the commit that gave its Float32 and Float64 halves one body (csrc/output.hip).  --cases mtj writes
tests/golden/mtj_session_golden.json: the joint multi-trait session (MTJ_CASES), pinned to the parent of the commit that gave it and the
mega-trait session one host body (csrc/block_session.hpp).

tests/test_gpu_session_golden.py replays the same calls on the current library and requires equal values and digests."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", ".."), os.path.join(HERE, "..")]
import session_golden_cases as G  # noqa: E402
from jwas_jl_amd import _lib  # noqa: E402


def _both(cases):
    return [(name, prec) for name in cases for prec in G.PRECISIONS]


FIXTURES = {"session": (_both(G.CASES), "session_golden.json"), "block": (_both(G.BLOCK_CASES), "block_session_golden.json"),
            "output": (G.output_keys(), "output_side_golden.json"), "mtj": (_both(G.MTJ_CASES), "mtj_session_golden.json")}


def rocm_version():
    try:
        import torch
        return str(torch.version.hip)
    except Exception:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True)
    ap.add_argument("--lib", default="")
    ap.add_argument("--cases", choices=sorted(FIXTURES), default="session")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    cases, default_out = FIXTURES[args.cases]
    args.out = args.out or os.path.join(HERE, default_out)
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    blob = {"commit": args.commit, "rocm": rocm_version(), "cases": {f"{name}/{prec}": G.run_case(name, prec) for name, prec in cases}}
    with open(args.out, "w") as fh:
        json.dump(blob, fh, separators=(",", ":"), sort_keys=True)
        fh.write("\n")
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
