"""The output layer of the chain drivers (mcmc.run_chain, multigeno.run_multigeno, megatrait.run_megatrait, mtjoint.run_mtjoint,
chains.run_chains, rrm.run_rrm): the sample
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


def timing(wall, t_sweep, chain_length, bs, n, p, **more):
    """runMCMC's "_timing" of a driver of a block session."""
    return {"wall_s": wall, "device_sweep_ms_total": t_sweep, "iterations": chain_length, "block_size": bs, "n": n, "p": p, **more}


class MultiTraitOutputs:
    """The outputs of a run with more than 4 traits on one genotype category (run_megatrait, run_mtjoint), as an unconstrained run of
    2 to 4 traits writes them (output.jl:320-437): the running means, the sample files, the tables.  The two variances are handed over
    as t x t matrices; pi=None: it is not estimated; out_ids=None: no EBVs.  diagonal_only (constraint=true): the genetic covariance
    of a sample keeps its diagonal, and the progress lines show the diagonal of the residual variance."""

    def __init__(self, model, folder, labels, off, sol, vare, G, pi, out_ids, *, double_precision, heritability, marker_samples, diagonal_only):
        Mi = model.M[0]
        self.name, self.marker_ids, self.traits, self.folder = Mi.name, Mi.markerID, list(model.lhsVec), folder
        self.labels, self.off, self.out_ids, self.diagonal_only = labels, off, out_ids, diagonal_only
        self.run_sol, self.run_vare, self.run_varg = Running(sol), Running(vare), Running(G)
        self.run_pi = Running(pi) if pi is not None else None
        self.ebv_run = [Running(np.zeros(len(out_ids))) for _ in self.traits] if out_ids is not None else None
        self.rnames = [f"{a}_{b}" for a in self.traits for b in self.traits]
        self.term_cols = term_sample_columns(model, labels, off)
        self.marker_samples, self.heritability = marker_samples, heritability
        self.ftype, self.fmt = (np.float64, "%.17g") if double_precision else (np.float32, "%.9g")      # the marker rows follow the precision of the run
        self.genvar = None
        self.files = SampleFiles(folder)

    def open(self):
        """Every sample file of the run: inside `with outputs.files:`."""
        files, name = self.files, self.name
        files.open("residual_variance", self.rnames)
        files.open(f"marker_effects_variances_{name}", self.rnames)
        if self.run_pi is not None:
            files.open(f"pi_{name}", [f"pi{i + 1}" for i in range(self.run_pi.mean.size)])
        if self.out_ids is not None and self.heritability:               # output.jl:358-362,426-432
            self.genvar = GeneticVarianceSamples(files, self.rnames, self.traits)
        for key, (_, header) in self.term_cols.items():
            files.open(key, header)
        if self.marker_samples:
            for tr in self.traits:
                files.open(f"marker_effects_{name}_{tr}", self.marker_ids)
        self.bin_writers = [files.marker_writer(f"marker_effects_{name}_{tr}", self.marker_ids) for tr in self.traits]

    def save(self, ks, sol, vare, G, pi, alpha, ebvs):
        """Saved sample number ks: alpha [t x p] the marker effects, ebvs (None without EBVs) the t vectors X_out alpha_k."""
        files, name = self.files, self.name
        self.run_sol.add(sol, ks)
        self.run_vare.add(vare, ks)
        self.run_varg.add(G, ks)
        if self.run_pi is not None:
            self.run_pi.add(pi, ks)
            files.row(f"pi_{name}", pi)
        for key, (cols, _) in self.term_cols.items():
            files.row(key, sol[cols])
        files.row("residual_variance", vare.ravel())
        files.row(f"marker_effects_variances_{name}", G.ravel())
        for k, tr in enumerate(self.traits):
            a = alpha[k].astype(self.ftype)
            si = np.flatnonzero(a).astype(np.int32)
            self.bin_writers[k].append(si, a[si])
            if self.marker_samples:
                files.effects_row(f"marker_effects_{name}_{tr}", a, self.fmt)
        if ebvs is not None:                                             # getEBV, output.jl:281-306
            for k, ebv in enumerate(ebvs):
                self.ebv_run[k].add(ebv, ks)
            if self.genvar is not None:                                  # output.jl:498-512
                self.genvar.add(ebvs, np.diag(vare), diagonal_only=self.diagonal_only)

    def print_means(self, it):
        print_posterior_means(it, np.diag(self.run_vare.mean) if self.diagonal_only else self.run_vare.mean)

    def tables(self, posteriors, pi_names):
        """The result tables (output.jl:108-212), written to the folder.  posteriors: a callable that returns (mean, mean of squares,
        model frequency) of trait k as the session holds them (doubles: the SD is formed from them as they are)."""
        name = self.name
        out = {"location parameters": location_table(self.labels, self.off, self.run_sol.mean, self.run_sol.sd()),
               "residual variance": covariance_table(self.rnames, self.run_vare)}
        out[f"marker effects {name}"] = marker_effects_table([(tr, self.marker_ids) + tuple(posteriors(k)) for k, tr in enumerate(self.traits)],
                                                             sd_in_double=False)
        out[f"marker effects variance {name}"] = covariance_table(self.rnames, self.run_varg)
        if self.run_pi is not None:
            out[f"pi_{name}"] = pi_table(self.run_pi, pi_names)
        if self.out_ids is not None:
            out.update(ebv_tables(self.traits, self.out_ids, self.ebv_run))
        if self.genvar is not None:
            out.update(self.genvar.tables())
        write_tables(out, self.folder)
        return out
