"""Writes tests/golden/chain_output_golden.json: what the chain drivers of ONE commit write and return for the cases of
tests/chain_output_cases.py.

    python tests/golden/make_chain_output_golden.py PACKAGE_ROOT COMMIT [OUT [session_driver]]

A fourth argument `session_driver` records chain_output_cases.SESSION_DRIVER_CASES (run_mtjoint, run_chains and the output rows of
run_megatrait) into tests/golden/session_driver_golden.json instead.

PACKAGE_ROOT is a checkout of the commit to record (its jwas_jl_amd.py and jwas.jl_amd/ are imported, not this tree's), COMMIT its
40-character hash.  The cases, the stand-in engines and the oracle library are this tree's."""
import json
import os
import pathlib
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def main():
    package_root, commit = os.path.abspath(sys.argv[1]), sys.argv[2]
    if len(commit) != 40:
        raise SystemExit("COMMIT must be the 40-character hash of the recorded checkout")
    sys.path[:0] = [package_root, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
    import numpy as np
    import jwas_jl_amd
    if os.path.dirname(os.path.abspath(jwas_jl_amd.__file__)) != os.path.join(package_root, "jwas.jl_amd"):
        raise SystemExit(f"imported {jwas_jl_amd.__file__}, not the package under {package_root}")
    import chain_output_cases as C
    which = sys.argv[4] if len(sys.argv) > 4 else "chain_output"
    selected = {"chain_output": C.CASES, "session_driver": C.SESSION_DRIVER_CASES}[which]
    cases = {}
    for name in selected:
        with tempfile.TemporaryDirectory() as tmp:
            cases[name] = C.run_case(name, pathlib.Path(tmp), selected)
        print(f"{name}: {len(cases[name]['sha256'])} files, {len(cases[name]['tables'])} tables", file=sys.stderr)
    out = sys.argv[3] if len(sys.argv) > 3 and sys.argv[3] else os.path.join(HERE, which + "_golden.json")
    with open(out, "w") as fh:
        dumps = lambda obj: json.dumps(obj, sort_keys=True, separators=(",", ":"))      # noqa: E731
        fh.write('{"commit":%s,"numpy":%s,"cases":{\n' % (dumps(commit), dumps(np.__version__)))      # one case per line
        fh.write(",\n".join(f"{dumps(name)}:{dumps(cases[name])}" for name in sorted(cases)))
        fh.write("\n}}\n")


if __name__ == "__main__":
    main()
