"""The output layer of the chain drivers (mcmc.run_chain, multigeno.run_multigeno, megatrait.run_megatrait, rrm.run_rrm): the sample
files of a run, the running means, and the result tables of output.jl:108-212 -- the one place where their formats are written down.
A driver keeps its sampler order and hands over values; where the drivers differ in a format, the difference is an argument here
and a commented choice at the call site."""
import contextlib
import os

import numpy as np

from .samples import MarkerSampleWriter


class Running:
    """mean += (x-mean)/k ; mean2 += (x^2-mean2)/k   (output.jl:556-560)"""

    def __init__(self, like):
        self.mean = np.zeros_like(np.asarray(like, dtype=np.float64))
        self.mean2 = np.zeros_like(self.mean)

    def add(self, x, k):
        x = np.asarray(x, dtype=np.float64)
        self.mean += (x - self.mean) / k
        self.mean2 += (x * x - self.mean2) / k

    def sd(self):
        return np.sqrt(np.abs(self.mean2 - self.mean ** 2))          # output.jl:112,133


@contextlib.contextmanager
def host_blas_limit():
    """The host step between two sweeps is a handful of O(n) vector operations.  A threaded BLAS runs them on every core and its
    workers keep spinning afterwards: in a container with a CPU quota that burns the quota and stalls the NEXT device call until the
    scheduler's next 100 ms period (measured: 78-100 ms per iteration instead of 21 at 50k x 600k).  JWAS_HOST_BLAS_THREADS overrides
    (0 = leave the BLAS alone)."""
    limit = None
    try:
        nthr = int(os.environ.get("JWAS_HOST_BLAS_THREADS", "1"))
        if nthr > 0:
            from threadpoolctl import threadpool_limits
            limit = threadpool_limits(limits=nthr, user_api="blas")
    except Exception:                            # threadpoolctl missing: nothing to limit with
        limit = None
    try:
        yield
    finally:                                     # also on an exception inside the chain: give the BLAS its threads back
        if limit is not None:
            limit.restore_original_limits()


def resolve_output_ids(model, obs_ids, record_ids):
    """check_outputID (input_data_validation.jl:143-196): (the individuals EBVs are reported for, whether they are exactly the
    training records in their order) -- all genotyped individuals unless outputEBV(model, IDs) named a list; IDs without genotypes
    are dropped with the reference's note."""
    want = list(obs_ids) if getattr(model, "output_ID", False) is False else list(model.output_ID)
    known = set(obs_ids)
    if not all(i in known for i in want):
        print("Testing individuals are not a subset of genotyped individuals (complete genomic data,non-single-step). "
              "Only output EBV for tesing individuals with genotypes.")
        want = [i for i in want if i in known]
    return want, want == list(record_ids)


def write_id_files(folder, record_ids, obs_ids):
    for name, ids in (("phenotypes", record_ids), ("genotypes", obs_ids)):
        with open(os.path.join(folder, f"IDs_for_individuals_with_{name}.txt"), "w") as fh:
            fh.write("\n".join(ids) + "\n")


class SampleFiles:
    """Every text sample file (MCMC_samples_<key>.txt) and every binary marker-sample writer of one run.  A driver opens them inside
    `with files:`, which closes whatever was opened by then -- at the end of the chain or on an exception."""

    def __init__(self, folder):
        self.folder, self._files, self._writers = folder, {}, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __contains__(self, key):
        return key in self._files

    def open_bare(self, key, filename=None):
        """A file without a header line (liabilities, thresholds: output.jl:367-372)."""
        self._files[key] = open(os.path.join(self.folder, filename or f"MCMC_samples_{key}.txt"), "w")

    def open(self, key, header):
        self.open_bare(key)
        self._files[key].write(",".join(header) + "\n")

    def row(self, key, values):
        self._files[key].write(",".join(repr(float(v)) for v in values) + "\n")

    def effects_row(self, key, array, fmt):
        """One value per marker, text at C speed; "%.9g" round-trips Float32, "%.17g" Float64."""
        array.tofile(self._files[key], sep=",", format=fmt)
        self._files[key].write("\n")

    def sparse_effects_row(self, key, idx, val, p, ftype, fmt):
        a = np.zeros(p, dtype=ftype)
        a[idx] = val
        self.effects_row(key, a, fmt)

    def marker_writer(self, key, marker_ids):
        """Sparse records of the saved marker effects (samples.py): MCMC_samples_<key>.bin."""
        self._writers.append(MarkerSampleWriter(os.path.join(self.folder, f"MCMC_samples_{key}.bin"), marker_ids))
        return self._writers[-1]

    def close(self):
        for fh in self._files.values():
            fh.close()
        for w in self._writers:
            w.close()


def sparse_effects(engine, trait):
    """(idx, val) of the nonzero marker effects of a trait: compacted on the device where the engine can."""
    if hasattr(engine, "alpha_sparse"):
        return engine.alpha_sparse(trait)
    a = engine.get_state(trait)[0]
    idx = np.flatnonzero(a).astype(np.int32)
    return idx, a[idx]


def term_sample_columns(model, labels, off):
    """outputMCMCsamples (output.jl:76-95,443-460): {file key: (columns of sol, header)} of the terms that are in the model."""
    terms = {}
    for tr, trm in getattr(model, "outputSamplesVec", []):
        k = model.lhsVec.index(tr)
        cols = [off[k] + i for i, (_, eff, _) in enumerate(labels[k]) if eff == trm]
        if cols:
            terms[f"{tr}.{trm}"] = (cols, [f"{tr}:{trm}:{labels[k][c - off[k]][2]}" for c in cols])
    return terms


class GeneticVarianceSamples:
    """The genetic (co)variance of every saved sample of the EBVs and the heritabilities from it (output.jl:498-512), their files,
    and the tables of output.jl:196-209.  trait_names=None: no heritability (RRM, output.jl:360-364)."""

    def __init__(self, files, cov_names, trait_names=None):
        self.files, self.names, self.samples = files, {"genetic_variance": cov_names}, {"genetic_variance": []}
        if trait_names is not None:
            self.names["heritability"], self.samples["heritability"] = trait_names, []
        for key, header in self.names.items():
            files.open(key, header)

    def add(self, ebvs, vare_diag=None, diagonal_only=False):
        gv = np.atleast_2d(np.cov(np.stack(ebvs, axis=1).astype(np.float64), rowvar=False))
        if diagonal_only:
            gv = np.diag(np.diag(gv))
        row = {"genetic_variance": gv.ravel()}
        if "heritability" in self.names:
            row["heritability"] = np.diag(gv) / (np.diag(gv) + vare_diag)
        for key, values in row.items():
            self.samples[key].append(values)
            self.files.row(key, values)

    def tables(self):
        """Mean and std of the samples; no table without a saved sample, no SD from one."""
        import pandas as pd
        out = {}
        for key, samples in self.samples.items():
            if samples:
                s = np.array(samples)
                out[key] = pd.DataFrame({"Covariance": self.names[key], "Estimate": s.mean(axis=0),
                                         "SD": s.std(axis=0, ddof=1) if len(s) > 1 else np.full(s.shape[1], np.nan)})
        return out


# ---- result tables (output.jl:108-212) --------------------------------------------------------------------------------------------
def state_labels(t):
    """The joint states of t indicators, state index = sum_k delta_k << k."""
    return ["".join(str((s >> k) & 1) for k in range(t)) for s in range(1 << t)]


def pi_labels(t, method):
    return state_labels(t) if t > 1 else (["class1", "class2", "class3", "class4"] if method == "BayesR" else ["π"])


def location_table(labels, off, mean, sd):
    import pandas as pd
    return pd.DataFrame([(tr, eff, lev, mean[off[k] + i], sd[off[k] + i]) for k, lab in enumerate(labels) for i, (tr, eff, lev) in enumerate(lab)],
                        columns=["Trait", "Effect", "Level", "Estimate", "SD"])


def covariance_table(names, run):
    import pandas as pd
    return pd.DataFrame({"Covariance": names, "Estimate": np.atleast_1d(run.mean).ravel(), "SD": np.atleast_1d(run.sd()).ravel()})


def marker_effects_table(parts, sd_in_double):
    """parts: (trait, marker IDs, mean, mean of squares, model frequency) per trait; sd_in_double: the SD from the moments cast to
    Float64 first (the engines return them in the element type of the run)."""
    import pandas as pd
    frames = []
    for tr, ids, ma, ma2, md in parts:
        sd = np.sqrt(np.abs(ma2.astype(np.float64) - ma.astype(np.float64) ** 2)) if sd_in_double else np.sqrt(np.abs(ma2 - ma ** 2))
        frames.append(pd.DataFrame({"Trait": tr, "Marker_ID": ids, "Estimate": ma, "SD": sd, "Model_Frequency": md}))
    return pd.concat(frames, ignore_index=True)


def pi_table(run, labels):
    import pandas as pd
    return pd.DataFrame({"π": labels, "Estimate": run.mean, "SD": run.sd()})


def ebv_tables(names, out_ids, runs):
    import pandas as pd
    return {f"EBV_{nm}": pd.DataFrame({"ID": out_ids, "EBV": r.mean, "PEV": np.abs(r.mean2 - r.mean ** 2)}) for nm, r in zip(names, runs)}


def write_tables(out, folder):
    for key, tab in out.items():                                         # JWAS.jl:480-482
        tab.to_csv(os.path.join(folder, key.replace(" ", "_") + ".txt"), index=False)


def print_posterior_means(it, residual_variance):
    print(f"\nPosterior means at iteration: {it}")
    print(f"Residual variance: {np.round(residual_variance, 6)}")
