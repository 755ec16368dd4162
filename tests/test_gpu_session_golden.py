"""Every device session computes what the parent commit computed, bit for bit.

The sessions' host code moved out of csrc/jwas_hip.hip into one unit each on shared plumbing (csrc/ctx.hpp), and their kernels onto
shared device helpers (csrc/device_util.hpp), with the order of every floating-point operation kept.  tests/golden/session_golden.json
holds what the parent commit's library returned for the calls of tests/session_golden_cases.py (written by
tests/golden/make_session_golden.py on the GPU): the small outputs in full, SHA-256 digests of the large ones, and the code and message
of the guards.  The replay must be EQUAL: there is no tolerance, the reference is the parent's own output.

tests/golden/block_session_golden.json does the same for the sessions that sweep blocks of markers themselves (mega-trait models, several
BayesR chains, random regression, GBLUP; G.BLOCK_CASES): written by the parent of the commit that gave them one copy of their shared
device helpers (csrc/device_util.hpp), marker state (csrc/marker_state.hpp) and block walk (csrc/mega.hpp).

tests/golden/output_side_golden.json does it for the output side of a context (G.OUTPUT_CASES: state, residual and posterior transfer,
X alpha, output rows, sparse samples, window sums, the GWAS session, marker covariances, and their guards): written by the parent of the
commit that gave the Float32 and Float64 halves of that surface one kernel and one host body each (csrc/output.hpp, csrc/output.hip).

tests/golden/mtj_session_golden.json does it for the joint multi-trait session at 5 and 8 traits (G.MTJ_CASES), with the refusals that
only the bare C ABI reaches: written by the parent of the commit that gave that session and the mega-trait session one host body
(csrc/block_session.hpp)."""
import json
import os

import pytest

import session_golden_cases as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(fixture):
    with open(os.path.join(ROOT, "tests", "golden", fixture)) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def golden():
    return _load("session_golden.json")


@pytest.fixture(scope="module")
def block_golden():
    return _load("block_session_golden.json")


def _covers(golden, cases):
    assert sorted(golden["cases"]) == sorted(f"{name}/{prec}" for name in cases for prec in G.PRECISIONS)
    assert golden["rocm"] and len(golden["commit"]) == 40                   # (the commit whose library wrote it)


def test_fixture_covers_every_case(golden):
    _covers(golden, G.CASES)


def test_block_fixture_covers_every_case(block_golden):
    _covers(block_golden, G.BLOCK_CASES)


@pytest.mark.parametrize("precision", G.PRECISIONS)
@pytest.mark.parametrize("name", G.CASES + G.BLOCK_CASES)
def test_session_is_the_parent_commits_bit_for_bit(golden, block_golden, name, precision):
    want = (block_golden if name in G.BLOCK_CASES else golden)["cases"][f"{name}/{precision}"]
    got = G.run_case(name, precision)
    assert got["inputs"] == want["inputs"], "the generated inputs differ from the fixture's (numpy's generator, not the library)"
    assert sorted(got["values"]) == sorted(want["values"]) and sorted(got["digests"]) == sorted(want["digests"])
    for key in sorted(want["values"]):
        assert got["values"][key] == want["values"][key], (key, got["values"][key], want["values"][key])      # (the doubles' reprs)
    for key in sorted(want["digests"]):
        assert got["digests"][key] == want["digests"][key], key
    assert got["errors"] == want["errors"]
    assert len(got["errors"]) == (2 if precision == 32 else 1) and all(code != 0 and msg for code, msg in got["errors"])


@pytest.fixture(scope="module")
def mtj_golden():
    return _load("mtj_session_golden.json")


def test_mtj_fixture_covers_every_case(mtj_golden):
    _covers(mtj_golden, G.MTJ_CASES)


@pytest.mark.parametrize("precision", G.PRECISIONS)
@pytest.mark.parametrize("name", G.MTJ_CASES)
def test_mtj_session_is_the_parent_commits_bit_for_bit(mtj_golden, name, precision):
    want = mtj_golden["cases"][f"{name}/{precision}"]
    got = G.run_case(name, precision)
    assert got["inputs"] == want["inputs"], "the generated inputs differ from the fixture's (numpy's generator, not the library)"
    assert sorted(got["values"]) == sorted(want["values"]) and sorted(got["digests"]) == sorted(want["digests"])
    for key in sorted(want["values"]):
        assert got["values"][key] == want["values"][key], (key, got["values"][key], want["values"][key])
    for key in sorted(want["digests"]):
        assert got["digests"][key] == want["digests"][key], key
    assert got["errors"] == want["errors"]
    assert len(got["errors"]) == G.MTJ_GUARDS + (2 if precision == 32 else 1) and all(code != 0 and msg for code, msg in got["errors"])


@pytest.fixture(scope="module")
def output_golden():
    return _load("output_side_golden.json")


# the guard records of every output case: the sparse list that does not fit the caller's arrays in each context case, and the guards
# case itself -- 14 (Float64 context) or 15 (Float32: set_marker_covariances_f64 too) entry points of the other precision, 2 x 9 calls
# with a trait out of range, 4 without output rows, 9 on arguments and sessions, 10 before init_state
OUTPUT_GUARDS = {"out_BayesC": 1, "out_MTBayesC": 1, "out_BayesR": 1, "out_guards": {32: 15 + 18 + 4 + 9 + 10, 64: 14 + 18 + 4 + 9 + 10}}


def test_output_fixture_covers_every_case(output_golden):
    assert sorted(output_golden["cases"]) == sorted(f"{name}/{prec}" for name, prec in G.output_keys())
    assert output_golden["rocm"] and len(output_golden["commit"]) == 40


@pytest.mark.parametrize("name,precision", G.output_keys())
def test_output_side_is_the_parent_commits_bit_for_bit(output_golden, name, precision):
    want = output_golden["cases"][f"{name}/{precision}"]
    got = G.run_case(name, precision)
    assert got["inputs"] == want["inputs"], "the generated inputs differ from the fixture's (numpy's generator, not the library)"
    assert sorted(got["values"]) == sorted(want["values"]) and sorted(got["digests"]) == sorted(want["digests"])
    for key in sorted(want["values"]):
        assert got["values"][key] == want["values"][key], (key, got["values"][key], want["values"][key])
    for key in sorted(want["digests"]):
        assert got["digests"][key] == want["digests"][key], key
    assert got["errors"] == want["errors"]
    nguards = OUTPUT_GUARDS.get(name, 0)
    assert len(got["errors"]) == (nguards[precision] if isinstance(nguards, dict) else nguards)
    assert all(code != 0 and msg for code, msg in got["errors"])
