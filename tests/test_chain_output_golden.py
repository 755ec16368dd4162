"""The four chain drivers write and return what the parent commit wrote and returned, byte for byte.

The bookkeeping around the samplers of mcmc.run_chain, multigeno.run_multigeno, megatrait.run_megatrait and rrm.run_rrm (sample
files, running means, result tables) moved into jwas.jl_amd/chain_output.py.  tests/golden/chain_output_golden.json holds what the
parent commit's drivers produced for the runs of tests/chain_output_cases.py on the CPU stand-in engines (written by
tests/golden/make_chain_output_golden.py): the names and SHA-256 digests of every file in the output folder, every returned table
(its columns and the repr of every Estimate / SD / EBV / PEV / Model_Frequency: short columns in full, longer ones as the SHA-256
of their reprs), the keys of _timing and everything printed.  The
replay must be EQUAL: there is no tolerance, the reference is the parent's own output.

tests/golden/session_driver_golden.json holds the same for C.SESSION_DRIVER_CASES -- megatrait.run_megatrait with output rows and missing
cells, mtjoint.run_mtjoint and chains.run_chains -- written by the parent of the commit that gave those three drivers one copy of their
record alignment, engine set-up and outputs (jwas.jl_amd/session_driver.py)."""
import json
import os
import re

import numpy as np
import pytest

import chain_output_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every family of MCMC_samples_* file the drivers know: at least one case must write each
FAMILIES = {
    "residual variance": r"MCMC_samples_residual_variance\.txt",
    "common marker-effect variance": r"MCMC_samples_marker_effects_variances_\w+\.txt",
    "pi": r"MCMC_samples_pi_\w+\.txt",
    "genetic variance": r"MCMC_samples_genetic_variance\.txt",
    "heritability": r"MCMC_samples_heritability\.txt",
    "location-parameter term (outputMCMCsamples)": r"MCMC_samples_\w+\.(herd|age|ID)\.txt",
    "single-step J and ϵ": r"MCMC_samples_y\.(J|ϵ)\.txt",
    "marker effects, text": r"MCMC_samples_marker_effects_(?!variances_)\w+\.txt",
    "marker effects, sparse binary": r"MCMC_samples_marker_effects_\w+\.bin",
    "indirect marker effects, text": r"MCMC_samples_indirect_marker_effects_\w+\.txt",
    "indirect marker effects, sparse binary": r"MCMC_samples_indirect_marker_effects_\w+\.bin",
    "overall marker effects, text": r"MCMC_samples_overall_marker_effects_\w+\.txt",
    "overall marker effects, sparse binary": r"MCMC_samples_overall_marker_effects_\w+\.bin",
    "set_random variances": r"MCMC_samples_(y1:x2|y:ϵ)_variances\.txt",
    "polygenic variance": r"MCMC_samples_polygenic_effects_variance\.txt",
    "liabilities": r"MCMC_samples_liabilities_\w+\.txt",
    "thresholds": r"MCMC_samples_threshold_\w+\.txt",
    "RRM EBV samples": r"MCMC_samples_EBV_[123]\.txt",
}


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "chain_output_golden.json")) as fh:
        return json.load(fh)


def test_fixture_covers_every_case(golden):
    assert sorted(golden["cases"]) == sorted(C.CASES)
    assert len(golden["commit"]) == 40 and golden["numpy"]                 # (the commit whose drivers wrote it)
    names = {f for rec in golden["cases"].values() for f in rec["sha256"]}
    for family, pattern in FAMILIES.items():
        assert any(re.fullmatch(pattern, f) for f in names), f"no case writes a file of the family: {family}"
    samples = {f for f in names if f.startswith("MCMC_samples_")}
    known = {f for f in samples if any(re.fullmatch(pattern, f) for pattern in FAMILIES.values())}
    assert samples == known, f"files of a family the list above does not name: {sorted(samples - known)}"


@pytest.fixture(scope="module")
def driver_golden():
    with open(os.path.join(ROOT, "tests", "golden", "session_driver_golden.json")) as fh:
        return json.load(fh)


def test_session_driver_fixture_covers_every_case(driver_golden):
    assert sorted(driver_golden["cases"]) == sorted(C.SESSION_DRIVER_CASES)
    assert len(driver_golden["commit"]) == 40 and driver_golden["numpy"]
    for name, rec in driver_golden["cases"].items():                     # (every run wrote its samples and its tables)
        assert any("MCMC_samples_" in f for f in rec["sha256"]) and rec["tables"], name


@pytest.mark.parametrize("name", C.CASES)
def test_driver_output_is_the_parent_commits_byte_for_byte(golden, name, tmp_path):
    _replay(golden, name, tmp_path, C.CASES)


@pytest.mark.parametrize("name", C.SESSION_DRIVER_CASES)
def test_session_driver_output_is_the_parent_commits_byte_for_byte(driver_golden, name, tmp_path):
    _replay(driver_golden, name, tmp_path, C.SESSION_DRIVER_CASES)


def _replay(golden, name, tmp_path, cases):
    want = golden["cases"][name]
    got = C.run_case(name, tmp_path, cases)
    assert got["inputs"] == want["inputs"], (f"the generated inputs differ from the fixture's (the data generators under numpy "
                                             f"{np.__version__}, fixture written under {golden['numpy']}; not the drivers)")
    assert sorted(got["sha256"]) == sorted(want["sha256"])               # the files of the output folder
    for f in sorted(want["sha256"]):
        assert got["sha256"][f] == want["sha256"][f], f
    assert sorted(got["tables"]) == sorted(want["tables"])
    for key in sorted(want["tables"]):
        assert got["tables"][key] == want["tables"][key], key
    assert got["timing_keys"] == want["timing_keys"]
    assert got["stdout"] == want["stdout"]
