"""The MULTI-TRAIT device sweeps AT THE GEOMETRIES `bench.py --workload config4` TIMES against the LITERAL per-marker chain (oracle form
'dense' under orc_set_mt_linear_form(0): per marker one dot product per trait, the t conditionals / the joint state / t single-trait
draws, one axpy per trait -- MTBayesABC.jl:57-127), not against the oracle's lookahead form, which shares the device's block
algebra (block partition, Gram-based corrections across blocks).  The multi-trait counterpart of tests/test_gpu_literal.py; rule:
DESIGN section 6.  The case table, the builder and the bars: tests/mt_literal_cases.py; the same rows on the CPU, lookahead oracle
against literal oracle: tests/test_mt_literal_host.py.

Device: MFMA Grams, n = 5 200 (five full 1024-row slices and a ragged one, several row groups), its default rules (Rule L on, no
section_solve).  Literal oracle: neither rule, no Gram.

Per sweep: state_counts (sampler I / II) or sum_delta (mega-trait), n_events and every trait's delta array equal.  At the end, per
trait: |alpha_hip - alpha_lit|.max() <= 1e-4 max(|alpha_lit|.max(), 1e-3), and the residual within 1e-4 of its own maximum (the
project's stated bars: tests/test_gpu_literal.py).

WHAT THE FLAGS AND COUNTERS PROVE, AND WHAT THEY DO NOT

  * sparse rows (skip and verify, sampler_role_mt).  Counter 31 counts the 64-marker sub-blocks a HELPER wave evaluated instead of
    the serial wave; counter 30 the blocks in which the serial wave took the chain over again because a marker of a skipped
    sub-block moved.  > 20 and (dup rows of sampler I / II: the copies of the causal columns sit in later sub-blocks of the same
    block) > 0 prove that both paths RAN; that their results are the chain's is what the delta / effect comparison proves.
  * mixed rows (256-marker blocks, half the markers changing joint state per sweep).  DENSE_MT set in
    HipEngine.last_sweep_schedule() says that the full 256-marker blocks of that sweep ran the dense-walk-only instantiation,
    whose sampler-I blocks are dense_big_mt (sampler_mt.hpp).  The host sets it from the previous sweep's change count
    (>= 10 % of p) for sampler I only: never in a chain's first sweep, never for sampler II or the mega-trait sampler, whose mixed
    rows run the general instantiation (candidacy front + speculative rounds).  DENSE_MT_SWEEPS is that observation, exact.
    There is NO counter for "the hoisted evaluation ran" (mt1_eval_hoisted inside walk_mixed), and none is added: code that merely
    exists in the sampler's kernel costs time (NOTES R6).  It is shown from the source and the inputs instead.  In dense_big_mt a
    section's walk takes walk_mixed's slow branch for lane l when bit l of
        slow = __ballot(!in_all) & ~skip;   if (popcount(slow) * 4 > 64) slow = ~skip;
    is set: in_all = every trait's delta is 1 at section entry, skip = markers out of the model for every trait (delta and alpha 0)
    that are predicted to stay out.  A marker in the model for some traits but not all is neither in_all nor skippable, so it sets
    its bit.  Sweep 1 starts from delta = 1 everywhere (slow = 0: walk_fast), and every marker that leaves the all-ones state
    fails the verification (`bad`) and is walked again through walk_mixed.  From sweep 2 on the entry state is the previous
    sweep's draw from a Dirichlet(1,..,1) prior over the 2^t states (default_rng(5): the all-ones state has prior mass 0.020 at
    t = 3 and 0.116 at t = 2, the partial states together 0.64 and 0.45), so most markers enter in a partial state; the test ASSERTS from the literal side's delta
    that every full 256-marker block of every sweep after the first is entered with at least one marker in a partial state.
    Together with DENSE_MT this proves that the slow branch ran on those sweeps -- not that it ran for any particular marker.
  * that at least one effect differs IN BITS from the literal oracle's shows that the device did not run the literal
    arithmetic (Rule L's linear form, the block algebra's association): the comparison is between two different computations.
  * levels row: the block size selected for each sweep is the host's; `used` records that all three were.

MEASURED (MI355X; largest relative difference over the traits; counters summed over the chain; every run prints them again):

  row               effects   residual  events  counter 31  counter 30  DENSE_MT sweeps  effects differing in bits
  s1-512-dup        7.0e-07   9.7e-07      707          42           1  none                  98
  s1-1024-dup       5.8e-07   1.0e-06      753          38           1  none                  81
  s1-1024-t4        2.3e-07   1.3e-06      853          23           2  none                 116
  s1-256-mixed-t3   1.9e-07   2.8e-06     4529           0           0  2..8                 433
  s1-256-mixed-t2   1.9e-07   1.4e-06     3366           0           0  2..8                 329
  s2-512-dup        9.4e-08   1.1e-06      697          54           2  none                  63
  s2-256-mixed      1.7e-07   1.3e-06     3500           0           0  none                 284
  mega-512-dup      1.3e-07   6.1e-07      622          52           1  none                  44
  mega-256-mixed    1.1e-07   1.6e-06     6199           0           0  none                1039
  b1-512            1.5e-07   1.1e-06      592          54           2  none                  72
  levels            2.0e-07   6.4e-07      602         126           0  none                  75

Rows s1-512-dup and s1-256-mixed-t3 run again under sweep seeds 29, 31, 37 and 41 (ids ...-seedNN): effects at most 1.0e-06, residual
at most 2.2e-06, counter 31 47..62, counter 30 2 / 1 / 0 / 0 (the take-over condition is asked of the table's rows only), DENSE_MT in
sweeps 2..8 of all four mixed ones.  The last test drives runMCMC itself against the literal chain (its docstring).

The bars are 1e-4: two orders of magnitude above the largest figure.  s1-1024-dup uses dataset seed 1938: with 1937 (and 1941) no
marker of a skipped sub-block moved in twelve sweeps at n = 5 200 (counter 30 = 0), so the take-over path would not have run;
1938 is the next seed, and the first tried, with counter 30 > 0.  No bar was touched; the chain at 1937 passed every comparison.
"""
import numpy as np
import pytest

import mt_literal_cases as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import jwas_jl_amd as J
    e = J.HipEngine(0)
    yield e
    e.close()


# Sweeps (1-based) of the mixed rows in which HipEngine.last_sweep_schedule() shows DENSE_MT.  n_events is asserted equal to the
# literal chain's in every sweep, and the flag is a function of the previous sweep's n_events, so the lists are exact.
DENSE_MT_SWEEPS = {
    "s1-256-mixed-t3": [2, 3, 4, 5, 6, 7, 8],
    "s1-256-mixed-t2": [2, 3, 4, 5, 6, 7, 8],
    "s2-256-mixed": [],
    "mega-256-mixed": [],
}


@pytest.mark.parametrize("case", M.CASES, ids=M.CASE_IDS)
def test_multitrait_device_sweeps_against_the_literal_chain(hip, case):
    t, mega = case.t, case.method == "MegaBayesC"
    inp = M.build_inputs(case)
    lit = M.literal(inp["X"], case.method, t)
    hip.load_dense(inp["X"])
    hip.setup_blocks(case.bs, "mfma")
    if case.levels:
        hip.add_block_size(512, "mfma"); hip.add_block_size(1024, "mfma")
    hip.init_state(case.method, t)
    M.start(lit, inp, t); M.start(hip, inp, t)
    events, helped, taken_over, changed, dense_mt, partial_ok, used = 0, 0, 0, [], [], [], set()
    nfull = case.p // 256
    with M.literal_order():
        for it in range(1, case.sweeps + 1):
            if case.levels:
                hip.select_block_size(M.level_of_sweep(it)); used.add(hip.block_size)
            before = M.joint_state(lit, t)
            part = ((before != 0) & (before != (1 << t) - 1))[:nfull * 256].reshape(nfull, 256)
            partial_ok.append(bool(part.any(axis=1).all()))
            sl = lit.sweep(iteration=it, seed=case.sweep_seed, **inp["kw"])
            sh = hip.sweep(iteration=it, seed=case.sweep_seed, **inp["kw"])
            diff = M.first_difference(lit, hip, t)
            assert diff is None, f"sweep {it}: trait {diff[0]} diverged from the literal chain at markers {diff[1]}"
            key = "sum_delta" if mega else "state_counts"
            assert np.array_equal(sl[key], sh[key]), f"sweep {it}: {key}"
            assert sl["n_events"] == sh["n_events"], f"sweep {it}"
            events += int(sh["n_events"])
            c = hip.last_sweep_counters()
            helped += int(c[31]); taken_over += int(c[30])
            changed.append(float((M.joint_state(lit, t) != before).mean()))
            if hip.last_sweep_schedule(names=True)["DENSE_MT"]:
                dense_mt.append(it)
    gaps = M.relative_gaps(lit, hip, t)
    differ = sum(int((lit.get_state(k)[0] != hip.get_state(k)[0]).sum()) for k in range(t))
    print(f"[mt-literal gpu] {case.id}: effects {max(g[0] for g in gaps):.2e}  residuals {max(g[1] for g in gaps):.2e}  events {events}  "
          f"counter 31 {helped}  counter 30 {taken_over}  DENSE_MT sweeps {dense_mt}  effects differing in bits {differ}  "
          f"joint-state changes per sweep {min(changed[1:]):.3f}..{max(changed[1:]):.3f}")
    for k, (ga, gr) in enumerate(gaps):
        assert ga <= M.REL_BAR, f"trait {k}: effects {ga:.2e} of their scale from the literal chain"
        assert gr <= M.REL_BAR, f"trait {k}: residual {gr:.2e} of its scale from the literal chain"
    if case.prior == "sparse":
        assert helped > 20, f"the helper waves evaluated only {helped} sub-blocks"
        assert events >= 300, f"vacuous: only {events} effect changes"
        if case.dup and case.method in ("MTBayesC", "MTBayesC_II") and M.is_table_row(case):
            assert taken_over > 0, "no skipped marker ever moved: the take-over path did not run"
        assert dense_mt == []
    else:
        assert all(0.30 <= c <= 0.95 for c in changed[1:]), f"joint-state changes per sweep {changed}"
        assert dense_mt == DENSE_MT_SWEEPS[case.id.split("-seed")[0]], f"sweeps that ran the dense-walk-only instantiation: {dense_mt}"
        assert all(partial_ok[1:]), "a full block was entered without a marker in a partial state: walk_mixed's slow branch is not proven"
        assert differ > 0, "every effect equals the literal oracle's bit for bit: the device's own arithmetic did not apply"
    if case.levels:
        assert used == {256, 512, 1024}


API_DATASET_SEED = 1426      # (1425 has a rounding tie in sweep 76: see the docstring below and NOTES)


def test_runmcmc_three_trait_default_prior_chain_against_the_literal_chain(tmp_path):
    """runMCMC as shipped (three traits, the default prior: every marker in the model, Pi estimated; MFMA Grams, the adaptive
    256 -> 512 block policy, Rule T by SectionSolvePolicy on the dense 256-marker sweeps) against the SAME host loop on the literal
    oracle engine -- the harness of tests/test_gpu_e2e.py::test_three_trait_chain_gpu_vs_oracle with OracleEngine(form="dense") in
    place of the lookahead form.  n = 5 200;
    p = 4 * 512 + 100 = 2 148, not 2 * 512 + 100: mcmc's adaptive_mt needs p > 4 * 512, below it the policy never leaves 256.  340
    sweeps: pick_block_size_mt first picks 512 in sweep 270 and both sizes run (asserted on the literal side, whose decisions are
    the device's when the chains are equal).  Bars: posterior-mean effects within 1e-4 of their scale, model frequencies EQUAL.

    Measured: effects 6.2e-7 of their scale; Rule T ran in 52 sweeps (seed 1425), every one of 340 sweeps taken from the device's own
    state made the literal chain's decisions.  Dataset seed: with 1425 the two chains part in sweep 76 at marker 364, trait 1 -- the
    literal oracle's inclusion probability 0.0299548550 against the uniform 0.0299548406, 1.4e-8 apart: a rounding tie (the chains'
    effects were 8.2e-7 of their scale apart entering that sweep; mt_literal_cases.literal_probabilities is the replay that printed
    it); 1426 is the next seed and has none in 340 sweeps."""
    import pandas as pd
    from oracle_engine import OracleEngine
    from conftest import make_dataset
    from jwas_jl_amd import api

    n, p, chain = M.N, 4 * 512 + 100, 340
    d = make_dataset(n=n, p=p, ncausal=24, h2=0.7, seed=API_DATASET_SEED, center=False)      # (the cases' generator settings)
    rng = np.random.default_rng(4)
    ids = [f"i{i}" for i in range(n)]
    gdf = pd.DataFrame(d["raw"], columns=[f"m{j}" for j in range(p)])
    gdf.insert(0, "ID", ids)
    ph = pd.DataFrame({"ID": ids, "y1": d["y"], "y2": (0.7 * d["y"] + 0.5 * rng.standard_normal(n)).astype(np.float32),
                       "y3": (-0.4 * d["y"] + 0.8 * rng.standard_normal(n)).astype(np.float32)})

    class Recording(OracleEngine):
        selected = ()

        def select_block_size(self, bs):
            super().select_block_size(bs)
            self.selected += (int(bs),)

    lit = Recording(form="dense")
    outs = {}
    for tag, eng in (("lit", lit), ("hip", None)):
        geno = api.get_genotypes(gdf, method="BayesC", estimatePi=True)
        model = api.build_model("y1 = intercept + geno\ny2 = intercept + geno\ny3 = intercept + geno")
        kw = dict(chain_length=chain, burnin=chain // 5, seed=11, outputEBV=False, output_folder=str(tmp_path / tag))
        if eng is None:
            outs[tag] = api.runMCMC(model, ph, **kw)
        else:
            with M.literal_order():
                outs[tag] = api.runMCMC(model, ph, _engine=eng, **kw)
    el, eh = outs["lit"]["marker effects geno"], outs["hip"]["marker effects geno"]
    assert len(eh) == 3 * p
    a, b = el["Estimate"].to_numpy(), eh["Estimate"].to_numpy()
    first512 = lit.selected.index(512) + 1 if 512 in lit.selected else None
    print(f"[mt-literal gpu] runMCMC: effects {np.abs(a - b).max() / np.abs(a).max():.2e} of their scale; model frequencies differ at "
          f"{int((el['Model_Frequency'].to_numpy() != eh['Model_Frequency'].to_numpy()).sum())} of {len(a)}; 512 first selected after sweep {first512}, "
          f"in {lit.selected.count(512)} of {len(lit.selected)} sweeps")
    assert 256 in lit.selected and 512 in lit.selected, "pick_block_size_mt never moved from 256 to 512"
    assert np.array_equal(el["Model_Frequency"].to_numpy(), eh["Model_Frequency"].to_numpy()), "model frequencies differ: the chains parted"
    assert np.abs(a - b).max() <= 1e-4 * np.abs(a).max()
