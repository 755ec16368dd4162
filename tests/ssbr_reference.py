"""CPU stand-in for the single-step imputation session (jwas_hip_ss_*, csrc/ssbr.hpp): a numpy restatement of single_step/SSBR.jl:83-159
-- a DENSE Float64 solve of A^nn M_n = -A^ng M_g, the rows [M_n; M_g][prow], the cast to the engine's element type -- on top of the
location-parameter stand-ins with structured random effects (locpar_ped_reference.py).  Also the small pedigrees the single-step
tests share."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import locpar_ped_reference as PR  # noqa: E402
from locpar_ped_reference import PedOracleEngine, PedOracleEngine64  # noqa: E402

CHUNK_GRANULE, MAX_CHUNK = 64, 65536


def estimate_bytes(n_n, g, nnz_l, nnz_u, nnz_a, markers_per_chunk):
    """jwas_hip_ss_estimate_bytes: three row-pointer arrays, (column, value) of every stored entry, two permutations, W, Gt, the staging block."""
    ldc = min(MAX_CHUNK, -(-max(int(markers_per_chunk), 1) // CHUNK_GRANULE) * CHUNK_GRANULE)
    return 24 * (n_n + 1) + 12 * (nnz_l + nnz_u + nnz_a) + 8 * n_n + 8 * ldc * (n_n + 2 * g)


class _SsMixin:
    """ss_begin .. ss_end of HipEngine.  The factors are multiplied back to A^nn (Pr A Pc = L U) and the solve is dense."""

    ss_estimate_bytes = staticmethod(estimate_bytes)

    def ss_begin(self, factors, Ai_ng, budget_bytes=None, markers_per_chunk=None, g=None):
        import scipy.sparse as sp
        L, U, perm_r, perm_c = (factors.L, factors.U, factors.perm_r, factors.perm_c) if hasattr(factors, "perm_r") else factors
        n = L.shape[0]
        Pr = sp.csc_matrix((np.ones(n), (perm_r, np.arange(n))), shape=(n, n))
        Pc = sp.csc_matrix((np.ones(n), (np.arange(n), perm_c)), shape=(n, n))
        self._ss_A = (Pr.T @ (L @ U) @ Pc.T).toarray()
        self._ss_Ang = np.asarray(Ai_ng.todense(), dtype=np.float64)
        self._ss_rows = {}
        chunk = 1000 if markers_per_chunk is None else int(markers_per_chunk)
        self._ss_ldc = min(MAX_CHUNK, -(-chunk // CHUNK_GRANULE) * CHUNK_GRANULE)
        return self._ss_ldc

    def _ss_all(self, Mg):
        Mg = np.asarray(Mg, dtype=np.float64)
        return np.vstack([np.linalg.solve(self._ss_A, -(self._ss_Ang @ Mg)), Mg])

    def ss_set_rows(self, target, prow):
        self._ss_rows[{"sweep": 0, "output": 1}.get(target, target)] = np.asarray(prow, dtype=np.int64)

    def ss_impute(self, j0, Mg):
        Mg = np.asarray(Mg)
        if Mg.shape[1] > self._ss_ldc:
            raise ValueError("count exceeds the session's markers per chunk")
        full = self._ss_all(Mg.astype(self.dtype))               # (the block arrives in the engine's element type)
        for target, prow in self._ss_rows.items():
            mat = self.X if target == 0 else self.X_out
            mat[:, j0:j0 + Mg.shape[1]] = full[prow].astype(mat.dtype)          # data_type.(Mpheno), SSBR.jl:137-138
        self.block_size = 0

    def ss_solve_host(self, Mg, prow):
        Mg = np.asarray(Mg, dtype=np.float64)
        return self._ss_all(Mg.reshape(Mg.shape[0], -1))[np.asarray(prow, dtype=np.int64)]

    def ss_end(self):
        self._ss_A = self._ss_Ang = None
        self._ss_rows = {}


class _Output64:
    """The output rows of a Float64 context (jwas_hip_load_output_dense_f64 / _mul_alpha_output_f64)."""

    def load_output_dense(self, X_out):
        self.X_out = np.asfortranarray(np.asarray(X_out, dtype=np.float64))

    def mul_alpha_output(self, trait=0):
        return self.X_out @ self.alpha[trait]


class SsOracleEngine(_SsMixin, PedOracleEngine):
    dtype = np.float32

    def load_output_dense(self, X_out):
        self.X_out = np.asfortranarray(np.asarray(X_out, dtype=np.float32))          # (writable: the session fills it in place)


class SsOracleEngine64(_SsMixin, _Output64, PedOracleEngine64):
    pass


def ped_for(ids, seed=4):
    """tests/test_gpu_locpar_ped.py::_ped_for: a pedigree over `ids` plus 40 ancestors: 40 founders, then len(ids) offspring in 3
    generations, each by one of 4 sires (animal 0 sires in every generation: its row of A-inverse is long)."""
    from jwas_jl_amd.single_step import Pedigree
    n = len(ids)
    _, sire, dam = PR.generate_pedigree(40, 3, n // 3, 4, 0.1, seed=seed)
    assert len(sire) == 40 + n
    return Pedigree([f"anc{i}" for i in range(40)] + list(ids), sire, dam)


def long_row_pedigree(seed=7):
    """120 members: 12 founders, then 3 generations of 36 by one of 2 sires -- animal 0 sires about half of every generation (>= 40
    offspring), parents are drawn from all earlier animals (inbreeding)."""
    from jwas_jl_amd.single_step import Pedigree
    ids, sire, dam = PR.generate_pedigree(12, 3, 36, 2, 0.1, seed=seed)
    return Pedigree(ids, sire, dam)


def split(ped, n_genotyped=37, seed=1, keep_non=("a0",)):
    """(genotyped IDs, non-genotyped IDs in pedigree order); the IDs of keep_non stay non-genotyped (the long row belongs to A^nn)."""
    rng = np.random.default_rng(seed)
    pool = [v for v in ped.ids if v not in keep_non]
    gen = set(rng.choice(pool, n_genotyped, replace=False).tolist())
    return [v for v in ped.ids if v in gen], [v for v in ped.ids if v not in gen]


def blocks(ped, genotyped):
    """(Ai_nn CSC, Ai_ng CSR, splu(Ai_nn)) the way the driver forms them."""
    from jwas_jl_amd import ssbr
    _, _, Ai_nn, Ai_ng = ssbr.pedigree_blocks(ped, genotyped)
    return Ai_nn, Ai_ng, ssbr.factorize(Ai_nn)


def small_case(seed=5, markers=70, traits=("y",)):
    """The small single-step case of the host and GPU tests: the 120-member long-row pedigree, 37 genotyped individuals x 70 markers,
    65 records in the pedigree (60 distinct IDs, genotyped and non-genotyped mixed, 5 repeated) and 3 records outside it; a0 and 42 of
    its offspring stay non-genotyped (a row of A^nn with more than 40 entries)."""
    import pandas as pd
    ped = long_row_pedigree()
    off0 = [ped.ids[i] for i in range(len(ped.ids)) if ped.sire[i] == 0][:42]
    gen, non = split(ped, 37, keep_non=["a0"] + off0)
    rng = np.random.default_rng(seed)
    G = rng.binomial(2, rng.uniform(0.15, 0.85, markers), size=(len(gen), markers)).astype(np.float64)
    gdf = pd.DataFrame(G, columns=[f"m{j}" for j in range(markers)])
    gdf.insert(0, "ID", gen)
    first = list(rng.choice(ped.ids, 60, replace=False))
    rec = first + list(rng.choice(first, 5, replace=False)) + ["x1", "x2", "x3"]
    ph = pd.DataFrame({"ID": rec, "age": rng.normal(size=len(rec)), "weights": rng.uniform(0.5, 2.0, len(rec))})
    for tr in traits:
        ph[tr] = rng.normal(size=len(rec))
    return dict(ped=ped, gen=gen, non=non, gdf=gdf, ph=ph, G=G)
