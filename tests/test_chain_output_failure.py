"""An exception inside the chain: it propagates unchanged, every file the run opened is closed, and the engine sees the session-end
calls it saw at the parent commit of the output-layer refactor (run_mtjoint and run_chains: at the parent of the commit that gave them
and run_megatrait one copy of their shared steps) -- one run per driver, on the runs of tests/chain_output_cases.py with a stand-in whose
sweep raises at iteration 3.

ENDS is the parent commit's list, recorded there with the same spy: run_chain ends the causal-structure session it opened (the
location-parameter session is ended after the results only); the other five drivers end nothing on the way out, and no driver closes
an engine that was handed to it."""
import builtins
import pathlib

import pytest

import chain_output_cases as C


class SweepFailed(RuntimeError):
    pass


def _engine_classes():
    from chains_reference import ChainsStandInEngine
    from mega_reference import MegaStandInEngine
    from mtj_reference import MtjStandInEngine
    from multigeno_reference import MultiOracleEngine
    from rrm_reference import RrmStandInEngine
    from sem_reference import SemLocparOracleEngine64
    return {"run_chain": ("causal_structure", SemLocparOracleEngine64, "sweep"),
            "run_multigeno": ("multigeno_mixed", MultiOracleEngine, "sweep"),
            "run_megatrait": ("megatrait_f64", MegaStandInEngine, "mega_sweep"),
            "run_rrm": ("rrm_default", RrmStandInEngine, "rrm_sweep"),
            "run_mtjoint": ("mtjoint_f64", MtjStandInEngine, "mtj_sweep"),
            "run_chains": ("chains_bayesc", ChainsStandInEngine, "mega_sweep")}


ENDS = {"run_chain": ["sem_end"], "run_multigeno": [], "run_megatrait": [], "run_rrm": [], "run_mtjoint": [], "run_chains": []}


@pytest.mark.parametrize("driver", sorted(ENDS))
def test_exception_in_the_chain_closes_every_file(driver, tmp_path, monkeypatch):
    case, cls, sweep_name = _engine_classes()[driver]
    sweep = getattr(cls, sweep_name)
    error = SweepFailed("the sweep of iteration 3")
    seen = []

    def failing(self, *args, **kw):
        seen.append(kw["iteration"])
        if kw["iteration"] == 3:
            raise error
        return sweep(self, *args, **kw)
    monkeypatch.setattr(cls, sweep_name, failing)

    ends = []
    for name in [nm for nm in dir(cls) if nm.endswith("_end") or nm == "close"]:
        def spy(self, *args, _name=name, _real=getattr(cls, name), **kw):
            ends.append(_name)
            return _real(self, *args, **kw)
        monkeypatch.setattr(cls, name, spy)

    opened = []
    real_open = builtins.open

    def tracking_open(file, *args, **kw):
        fh = real_open(file, *args, **kw)
        if str(tmp_path) in str(file) and any(c in (args[0] if args else kw.get("mode", "r")) for c in "wa"):
            opened.append((str(file), fh))
        return fh
    monkeypatch.setattr(builtins, "open", tracking_open)

    inputs, run = {**C.CASES, **C.SESSION_DRIVER_CASES}[case](tmp_path)
    with pytest.raises(SweepFailed) as ei:
        run()
    assert ei.value is error                                             # the exception itself, not a wrapped one
    assert seen[-1] == 3 and 1 in seen and 2 in seen
    samples = [path for path, _ in opened if "MCMC_samples" in pathlib.Path(path).name]
    assert len(samples) >= 4, samples                                    # (the run had opened its sample files)
    still_open = [path for path, fh in opened if not fh.closed]
    assert not still_open, still_open
    assert ends == ENDS[driver]
