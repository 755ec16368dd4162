"""The host side of the sweep enqueues what the parent commit enqueued: every chain comes out bit for bit.

csrc/jwas_hip.hip's sweep_enqueue and f64_sweep became a sequence of named stages on one schedule plan (csrc/sweep_plan.hpp) and one prior
fill for both widths, with no kernel touched and the order of the enqueued work kept.  tests/golden/sweep_host_golden.json holds what the
parent commit's library returned for the chains of tests/sweep_host_cases.py (written twice on the GPU by
tests/golden/make_sweep_host_golden.py, the two writings equal): per sweep n_events, the schedule word and every statistic but the
milliseconds, and after the last sweep SHA-256 digests of alpha, beta, delta and the residual per trait.  The replay must be EQUAL:
there is no tolerance, the reference is the parent's own output."""
import json
import os

import pytest

import sweep_host_cases as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "sweep_host_golden.json")) as fh:
        return json.load(fh)


def test_fixture_covers_every_case(golden):
    assert sorted(golden["cases"]) == sorted(G.CASES)
    assert golden["rocm"] and len(golden["commit"]) == 40                   # (the commit whose library wrote it)


@pytest.mark.parametrize("name", sorted(G.CASES))
def test_sweep_is_the_parent_commits_bit_for_bit(golden, name):
    want = golden["cases"][name]
    got = G.run_case(name)
    assert len(got["sweeps"]) == len(want["sweeps"])
    for it, (g, w) in enumerate(zip(got["sweeps"], want["sweeps"]), 1):
        assert sorted(g) == sorted(w)
        for key in sorted(w):
            assert g[key] == w[key], (f"sweep {it}", key, g[key], w[key])
    assert got["final"] == want["final"]
    if name.startswith("timing/"):                                         # (the bracket around every second launch counted and sized)
        assert all(s["update_kernel_samples"][0] > 0 and s["update_kernel_bytes"][0] > 0 for s in got["sweeps"])
