"""Convergence diagnostics on sample files: PSRF, the reference's function of that name (misc/convergence_diagnosis.jl:31-57)."""
import re

import numpy as np


def _read_samples(path, header):
    with open(path) as fh:
        lines = [ln for ln in fh.read().splitlines() if ln.strip()]
    if header:
        lines = lines[1:]
    values = [float(v) for ln in lines for v in re.split(r"[,\s]+", ln.strip()) if v]
    if len(values) < 2:
        raise ValueError(f"{path}: at least two sample values are needed")
    return np.array(values, dtype=np.float64)


def PSRF(*files, header=True):
    """The potential scale reduction factor of convergence_diagnosis.jl:31-57, one sample file per chain, as that code evaluates:

      * a file is ONE pooled sample: its mean and variance (n - 1 in the denominator) run over every value of the file, whatever
        its rows and columns; N is the number of values of the LAST file, M the number of files;
      * B = N / (M - 1) sum (mean_i - mean of the means)^2,  W = the mean of the variances;
      * V = (N - 1) / N * W + (M + 1) / N * M * B -- evaluated left to right, that is ((M + 1) / N) M B, where Gelman and Rubin have
        (M + 1) / (M N) B;
      * the result is V / W, with no square root.

    header=True drops the first line of every file.  The reference reads with readdlm's default (white space separates); here commas
    separate as well, so that one column of an MCMC_samples_*.txt file copied to a file of its own, or a one-column file such as
    MCMC_samples_residual_variance.txt of a single-trait run, reads the same.

    How it differs from the statistic runMCMC(chains=K) writes to PSRF.txt: that one is per parameter (every marker effect, pi, the
    variances), sqrt(V / W) with V = (N - 1) / N W + B / N in the form of Gelman and Rubin (1992) without the (M + 1) / M sampling
    correction, and N there is the number of saved samples of a chain.  With M B in place of B / M the value here grows with the
    square of the number of chains where the chains disagree; the two agree only in saying "near 1 is good"."""
    if len(files) < 2:
        raise ValueError("PSRF needs the sample files of at least two chains.")
    means, variances, n = [], [], 0
    for path in files:
        x = _read_samples(path, header)
        means.append(x.mean())
        variances.append(x.std(ddof=1) ** 2)
        n = x.size
    M, N = len(files), n
    means = np.array(means)
    B = N / (M - 1) * np.sum((means - means.mean()) ** 2)
    W = float(np.mean(variances))
    V = (N - 1) / N * W + (M + 1) / N * M * B
    return V / W
