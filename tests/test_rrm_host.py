"""runMCMC(RRM=Phi) on the CPU stand-in (tests/rrm_reference.py): the exact block form against the marker-by-marker chain,
generatefullPhi, the draws against their closed-form posterior, the driver's outputs and every error of the contract."""
import contextlib
import io
import os

import numpy as np
import pytest

import rrm_reference as RR
from rrm_reference import RrmStandInEngine


# ---- 1. the blocked restatement against the marker-by-marker chain ------------------------------------------------------------------
def test_block_form_is_the_marker_by_marker_chain():
    """n = 301, p = 96, T = 5, c = 3, 20 % of the records missing, three sweeps with shared draws: blocks of 1, 40 and p choose the
    states of the plain chain; effects and residual agree within 1e-12 relative."""
    cs = RR.make_case(301, 96, 5, 3, 0.2, 7)
    O = RR.occupancy(cs.Phi, cs.obs)
    M = RR.m_array(cs.X, O)

    def run(bs):
        W, a, b, d = cs.W.copy(), cs.alpha.copy(), cs.beta.copy(), cs.delta.copy()
        grams = None if bs is None else [RR.gram_block(cs.X, O, j0, min(bs, cs.p - j0)) for j0 in range(0, cs.p, bs)]
        out = []
        for it in (1, 2, 3):
            kw = dict(iteration=it, seed=5, vare=cs.vare, G=cs.G, log_pi=cs.log_pi, min_margin=1e-9)
            r = RR.sweep_plain(cs.X, cs.Phi, cs.obs, M, W, a, b, d, **kw) if bs is None else \
                RR.sweep_blocked(cs.X, cs.Phi, cs.obs, M, grams, W, a, b, d, block_size=bs, **kw)
            out.append((r.states.copy(), a.copy(), b.copy(), W.copy(), r))
        return out
    ref = run(None)
    assert len({tuple(o[0]) for o in ref}) == 3 and all(o[4].n_changed > 0 for o in ref)
    for bs in (1, 40, cs.p):
        for (s0, a0, b0, w0, r0), (s1, a1, b1, w1, r1) in zip(ref, run(bs)):
            assert np.array_equal(s0, s1)
            da = np.abs(a0 - a1).max() / np.abs(a0).max()
            db = np.abs(b0 - b1).max() / np.abs(b0).max()
            dw = np.abs(w0 - w1).max() / np.abs(w0).max()
            print(f"blocks of {bs}: alpha {da:.2e}, beta {db:.2e}, residual {dw:.2e} relative")
            assert max(da, db, dw) <= 1e-12
            assert np.all(w1[~cs.obs] == 0.0) and np.array_equal(r0.state_counts, r1.state_counts) and r0.n_changed == r1.n_changed


# ---- 2. generatefullPhi ---------------------------------------------------------------------------------------------------------------
def test_generatefullphi_closed_form():
    from jwas_jl_amd import api
    timevec = [3, 1, 2, 5, 4, 2, 1, 9, 7]                                # unsorted, repeated, unevenly spaced
    Phi = api.generatefullPhi(timevec, 5)
    assert Phi.shape == (7, 5)
    np.testing.assert_allclose(Phi, RR.legendre_phi(timevec, 5), rtol=0, atol=4e-15)
    q = 2.0 * (np.array([1, 2, 3, 4, 5, 7, 9.0]) - 1) / 8 - 1
    np.testing.assert_allclose(Phi[:, 0], np.sqrt(0.5), atol=1e-16)
    np.testing.assert_allclose(Phi[:, 1], np.sqrt(1.5) * q, atol=1e-15)
    np.testing.assert_allclose(Phi[:, 2], np.sqrt(2.5) * 0.5 * (3 * q * q - 1), atol=2e-15)
    assert api.generatefullPhi([0.0, 10.0]).shape == (2, 3)              # ncoeff defaults to 3
    with pytest.raises(ValueError, match="two distinct"):
        api.generatefullPhi([4, 4, 4])
    # the columns are orthonormal on a fine grid: int_-1^1 phi_a phi_b = delta_ab
    grid = np.linspace(0, 1, 20001)
    F = api.generatefullPhi(grid, 4)
    np.testing.assert_allclose(F.T @ F * (2.0 / 20000), np.eye(4), atol=2e-3)


# ---- 3. the draws follow the closed-form posterior -------------------------------------------------------------------------------------
def test_one_marker_draws_follow_the_closed_form_posterior():
    case = RR.conditional_case()
    prob, _ = RR.conditional_posterior(case)
    assert prob.min() > 0.08                                             # every state is visited a few hundred times
    eng = RR.conditional_engine(RrmStandInEngine(64), case)
    rows_state, rows_coef = RR.conditional_check(eng, case)
    for s, zf in rows_state:
        print(f"state {s}: frequency {zf:.2f} se from P = {prob[s]:.4f}")
    for s, q, zm, zv in rows_coef:
        print(f"state {s} coefficient {q}: mean {zm:.2f} se, variance {zv:.2f} se")
    assert len(rows_state) == 4 and max(z for _, z in rows_state) <= 5.0
    assert len(rows_coef) == 8 and max(max(zm, zv) for _, _, zm, zv in rows_coef) <= 5.0


# ---- 4. and 5. the driver ----------------------------------------------------------------------------------------------------------------
def rrm_data(n=60, p=48, T=4, c=3, seed=3):
    """(genotype frame, phenotype frame in shuffled record order, Phi): growth-curve records with ~25 % of them missing."""
    import pandas as pd
    rng = np.random.default_rng(seed)
    ids = [f"i{i}" for i in range(n)]
    raw = rng.binomial(2, rng.uniform(0.15, 0.85, p), size=(n, p)).astype(np.float64)
    gdf = pd.DataFrame(raw, columns=[f"m{j}" for j in range(p)])
    gdf.insert(0, "ID", ids)
    times = np.array([2.0, 5.0, 9.0, 14.0, 20.0, 27.0][:T])
    Phi = RR.legendre_phi(times, c)
    Xc = raw - raw.mean(axis=0)
    a = np.zeros((p, c))
    a[rng.choice(p, 8, replace=False)] = 0.4 * rng.standard_normal((8, c))
    u = Xc @ a @ Phi.T                                                   # n x T
    rows = []
    for i in range(n):
        keep = rng.random(T) >= 0.25
        keep[rng.integers(T)] = True
        for t in np.flatnonzero(keep):
            rows.append((ids[i], times[t], 1.0 + 0.05 * times[t] + u[i, t] + 0.5 * rng.standard_normal(), rng.uniform(1, 3)))
    ph = pd.DataFrame(rows, columns=["ID", "time", "y", "age"]).sample(frac=1.0, random_state=5).reset_index(drop=True)
    return gdf, ph, Phi


def run_rrm(tmp_path, name, *, data=None, engine="standin", double=True, geno_kw=None, model_kw=None, equation="y = intercept + age + geno",
            ph_edit=None, model_edit=None, Phi=None, **kw):
    from jwas_jl_amd import api
    gdf, ph, Phi0 = data if data is not None else rrm_data()
    ph = ph.copy()
    if ph_edit is not None:
        ph = ph_edit(ph) if ph_edit(ph) is not None else ph
    if engine == "standin":
        engine = RrmStandInEngine(64 if double else 32)
    with contextlib.redirect_stdout(io.StringIO()):
        gk = dict(method="BayesC", double_precision=double)
        gk.update(geno_kw or {})
        geno = api.get_genotypes(gdf, **gk)                              # noqa: F841 (build_model finds it)
        model = api.build_model(equation, **(model_kw or {}))
        api.set_covariate(model, "age")
        if model_edit is not None:
            model_edit(model, api)
        args = dict(chain_length=20, burnin=5, seed=17, double_precision=double, RRM=Phi0 if Phi is None else Phi,
                    output_folder=str(tmp_path / name), _engine=engine, block_size=20)
        args.update(kw)
        out = api.runMCMC(model, ph, **args)
    return out


def expected_files(c):
    names = ["residual_variance", "marker_effects_variances_geno", "pi_geno", "genetic_variance"]
    names += [f"marker_effects_geno_{q + 1}" for q in range(c)] + [f"EBV_{q + 1}" for q in range(c)]
    return [f"MCMC_samples_{nm}.txt" for nm in names]


def check_outputs(out, folder, n, p, c, nsaved):
    assert "heritability" not in out and not os.path.exists(os.path.join(folder, "MCMC_samples_heritability.txt"))
    me = out["marker effects geno"]
    assert list(me.columns) == ["Trait", "Marker_ID", "Estimate", "SD", "Model_Frequency"] and len(me) == c * p
    assert list(me["Trait"].unique()) == [str(q + 1) for q in range(c)]
    assert len(out["pi_geno"]) == 1 << c and list(out["pi_geno"]["π"])[1] == "1" + "0" * (c - 1)
    assert list(out["residual variance"]["Covariance"]) == ["1"]
    assert len(out["marker effects variance geno"]) == c * c and len(out["genetic_variance"]) == c * c
    assert list(out["location parameters"]["Effect"]) == ["intercept", "age"]
    for q in range(c):
        assert len(out[f"EBV_{q + 1}"]) == n and list(out[f"EBV_{q + 1}"].columns) == ["ID", "EBV", "PEV"]
    for f in expected_files(c):
        rows = open(os.path.join(folder, f)).read().strip().split("\n")
        assert len(rows) == nsaved + 1, f
    assert len(open(os.path.join(folder, "MCMC_samples_marker_effects_geno_1.txt")).readline().split(",")) == p
    for tab in out.values():
        if hasattr(tab, "select_dtypes"):
            assert np.all(np.isfinite(tab.select_dtypes("number").to_numpy()))
    for key in out:
        if key != "_timing":
            assert os.path.exists(os.path.join(folder, key.replace(" ", "_") + ".txt"))


def test_driver_outputs_and_same_seed_same_files(tmp_path):
    gdf, ph, Phi = data = rrm_data()
    out = run_rrm(tmp_path, "a", data=data)
    p = len(out["marker effects geno"]) // 3
    check_outputs(out, str(tmp_path / "a"), 60, p, 3, 15)
    assert out["_timing"]["nrecords"] == len(ph) and out["_timing"]["ntimes"] == 4
    # EBV_q = X alpha_q over the phenotyped individuals in first-appearance order of the records sorted by time, then ID
    first = ph.sort_values(["time", "ID"], kind="stable")["ID"].drop_duplicates().tolist()
    assert list(out["EBV_1"]["ID"]) == first
    assert out["pi_geno"]["SD"].max() > 0 and out["residual variance"]["SD"][0] > 0
    run_rrm(tmp_path, "b", data=data)
    for f in sorted(os.listdir(tmp_path / "a")):
        assert open(tmp_path / "a" / f).read() == open(tmp_path / "b" / f).read(), f
    other = run_rrm(tmp_path, "c", data=data, seed=18)
    assert not np.array_equal(other["marker effects geno"]["Estimate"], out["marker effects geno"]["Estimate"])
    # estimatePi = false: no pi table, the prior stays on the all-ones state (tools4genotypes.jl:357-373): every marker in the model
    fixed = run_rrm(tmp_path, "d", data=data, geno_kw=dict(estimatePi=False))
    assert "pi_geno" not in fixed and np.all(fixed["marker effects geno"]["Model_Frequency"] == 1.0)
    # Float32 storage
    f32 = run_rrm(tmp_path, "e", data=data, double=False)
    check_outputs(f32, str(tmp_path / "e"), 60, p, 3, 15)


def test_contract_errors(tmp_path):
    from jwas_jl_amd import api
    data = rrm_data()
    Phi = data[2]
    count = [0]

    def fails(exc, match, **kw):
        count[0] += 1
        with pytest.raises(exc, match=match):
            run_rrm(tmp_path, f"e{count[0]}", data=data, **kw)
        assert not os.path.exists(tmp_path / f"e{count[0]}")            # nothing was written

    for method in ("BayesA", "BayesB", "BayesR", "RR-BLUP", "BayesL"):
        fails(NotImplementedError, "BayesC only", geno_kw=dict(method=method))
    fails(NotImplementedError, "fast_blocks as a vector", fast_blocks=[1, 21, 41])
    fails(NotImplementedError, "independent_blocks", fast_blocks=True, independent_blocks=True)
    fails(NotImplementedError, "set_random", equation="y = intercept + age + herd + geno",
          ph_edit=lambda ph: ph.assign(herd=[f"h{i % 3}" for i in range(len(ph))]), model_edit=lambda m, api_: api_.set_random(m, "herd", 0.3))
    fails(NotImplementedError, "categorical or censored", model_kw=dict(categorical_trait=["y"]),
          ph_edit=lambda ph: ph.assign(y=np.digitize(ph["y"], [ph["y"].median()]) + 1.0))
    fails(NotImplementedError, "categorical or censored", model_kw=dict(censored_trait=["y"]),
          ph_edit=lambda ph: ph.assign(y_l=ph["y"] - 0.1, y_u=ph["y"] + 0.1))
    fails(ValueError, "causal_structure", causal_structure=np.zeros((1, 1)))
    fails(NotImplementedError, "annotations", geno_kw=dict(annotations=np.random.default_rng(1).random((48, 2))))
    fails(NotImplementedError, "starting values", geno_kw=dict(starting_value=np.zeros(48)))
    fails(NotImplementedError, "starting values", starting_value=np.zeros(5))

    class Sharded(RrmStandInEngine):
        def comm_info(self):
            return (0, 2)
    fails(NotImplementedError, "shards", engine=Sharded())

    class NoRrm:
        precision, dtype = 64, np.float64
    with pytest.raises(NotImplementedError, match="no CPU fallback") as ei:
        run_rrm(tmp_path, "nofallback", data=data, engine=NoRrm())
    assert "rrm_sweep" in str(ei.value)
    fails(NotImplementedError, "one trait", equation="y = intercept + geno\nz = intercept + geno", ph_edit=lambda ph: ph.assign(z=ph["y"] * 2))
    fails(ValueError, "regression coefficients", Phi=RR.legendre_phi(np.arange(4.0), 5))
    fails(ValueError, "regression coefficients", Phi=Phi[:, :1])
    fails(ValueError, "time points", Phi=np.ones((65, 3)))
    fails(ValueError, "4 distinct time points but Phi has 3 rows", Phi=Phi[:3])
    fails(ValueError, "column named time", ph_edit=lambda ph: ph.rename(columns={"time": "day"}))
    fails(ValueError, "finite", Phi=np.where(np.arange(12).reshape(4, 3) == 5, np.nan, Phi))
    fails(NotImplementedError, 'location_parameters="device"', location_parameters="device")
    fails(NotImplementedError, "heterogeneous_residuals", heterogeneous_residuals=True)
    fails(ValueError, "block_size", block_size=257)
    # storage=:stream: the reference's message (input_data_validation.jl:97-98)
    from jwas_jl_amd import streaming as S
    gdf, ph, _ = data
    prefix = S.prepare_streaming_genotypes(gdf.iloc[:, 1:].to_numpy(dtype=np.float64), tmp_path / "st", obs_ids=list(gdf["ID"]), marker_ids=list(gdf.columns[1:]))
    with contextlib.redirect_stdout(io.StringIO()):
        geno = api.get_genotypes(prefix, method="BayesC", storage="stream")      # noqa: F841
        model = api.build_model("y = intercept + geno")
        with pytest.raises(ValueError, match="storage=:stream MVP does not support random regression model"):
            api.runMCMC(model, ph, RRM=Phi, output_folder=str(tmp_path / "stream"), _engine=RrmStandInEngine(32))
    # any other non-false value keeps today's catch-all
    for bad in (True, "legendre", 3):
        with pytest.raises(NotImplementedError, match=r"runMCMC\(\.\.\.; RRM=\.\.\.\) is outside the device marker path and stays on the reference"):
            run_rrm(tmp_path, "catchall", data=data, RRM=bad)
    # an individual without genotypes, two records at one time point
    with pytest.raises(ValueError, match="is not found"):
        run_rrm(tmp_path, "unknown", data=data, ph_edit=lambda ph: ph.assign(ID=ph["ID"].where(ph.index != 3, "nobody")))
    with pytest.raises(ValueError, match="more than one record"):
        import pandas as pd
        run_rrm(tmp_path, "dup", data=data, ph_edit=lambda ph: pd.concat([ph, ph.iloc[:1]], ignore_index=True))
