"""The oracle's LOOKAHEAD form -- the restatement every multi-trait GPU parity test trusts: block form on the device's partition,
Float64 Grams, Gram-based corrections across blocks -- against the LITERAL non-block chain (tests/mt_literal_cases.py) on every row
of the case table (and rows 1 and 4 under four more sweep seeds), at the rows' own shapes (n = 5 200).  No GPU.

What this pins: the restatement itself to MTBayesABC.jl:57-127 where no device is present; and that the inputs of
tests/test_gpu_mt_literal.py stay inside its bars on the reference side alone (the printed gaps are the reference-side share of
those bars: measured <= 7.8e-7 of the scale for the effects and <= 2.6e-6 for the residuals, the bars are 1e-4).

Asserted per row: every trait's delta identical after EVERY sweep; effects and residuals within 1e-4 of their scale at the end;
and the non-vacuity conditions that need no device counter -- sparse rows: >= 300 effect changes over the chain; mixed rows:
30 % .. 95 % of the markers change joint state in every sweep after the first.
"""
import numpy as np
import pytest

import mt_literal_cases as M
from oracle_engine import OracleEngine


@pytest.mark.parametrize("case", M.CASES, ids=M.CASE_IDS)
def test_lookahead_oracle_against_the_literal_chain(case):
    t = case.t
    inp = M.build_inputs(case)
    lit = M.literal(inp["X"], case.method, t)
    la = OracleEngine(form="lookahead")
    la.load_dense(inp["X"])
    la.setup_blocks(case.bs)
    if case.levels:
        la.add_block_size(512); la.add_block_size(1024)
    la.init_state(case.method, t)
    M.start(lit, inp, t); M.start(la, inp, t)
    events, changed, used = 0, [], set()
    for it in range(1, case.sweeps + 1):
        if case.levels:
            la.select_block_size(M.level_of_sweep(it)); used.add(la.block_size)
        before = M.joint_state(lit, t)
        with M.literal_order():
            sl = lit.sweep(iteration=it, seed=case.sweep_seed, **inp["kw"])
        so = la.sweep(iteration=it, seed=case.sweep_seed, **inp["kw"])
        diff = M.first_difference(lit, la, t)
        assert diff is None, f"sweep {it}: trait {diff[0]} diverged from the literal chain at markers {diff[1]}"
        assert sl["n_events"] == so["n_events"], f"sweep {it}"
        key = "sum_delta" if case.method == "MegaBayesC" else "state_counts"      # (the mega-trait sampler has no joint states)
        assert np.array_equal(sl[key], so[key]), f"sweep {it}: {key}"
        events += int(sl["n_events"])
        changed.append(float((M.joint_state(lit, t) != before).mean()))
    gaps = M.relative_gaps(lit, la, t)
    print(f"[mt-literal host] {case.id}: effects {max(g[0] for g in gaps):.2e}  residuals {max(g[1] for g in gaps):.2e}  "
          f"events {events} (last sweep {int(sl['n_events'])})  joint-state changes per sweep {min(changed[1:]):.3f}..{max(changed[1:]):.3f}")
    for k, (ga, gr) in enumerate(gaps):
        assert ga <= M.REL_BAR, f"trait {k}: effects {ga:.2e} of their scale from the literal chain"
        assert gr <= M.REL_BAR, f"trait {k}: residual {gr:.2e} of its scale from the literal chain"
    if case.prior == "sparse":
        assert events >= 300, f"vacuous: only {events} effect changes"
    else:
        assert all(0.30 <= c <= 0.95 for c in changed[1:]), f"joint-state changes per sweep {changed}"
    if case.levels:
        assert used == {256, 512, 1024}
