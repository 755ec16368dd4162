"""TEST INFRASTRUCTURE for the pedigree random effect (csrc/locpar.hpp, "A STRUCTURED random effect"): the demo pedigree, a seeded
pedigree generator, the numpy restatement of the structured step on the device's Philox counters, and stand-in engines that add
locpar_set_group_structure / locpar_group_colors / locpar_structure_estimate_bytes to the stand-ins of tests/locpar_reference.py.

For level l of a member term of trait k (position pos in its random effect), V = the structure, p_km = vare Gi_km (one trait) or
Gi_km (several):
    S_l    as for any term (locpar_reference.term_draw)
    lhs_l  = d_l c_kk + p_kk V_ll
    mean_l = (S_l + d_l c_kk sol_l - sum_m p_km sum_j V_lj u_m,j) / lhs_l        (the sum over j skips j == l for m == k)
    sol_l' = mean_l + z sqrt(s / lhs_l)
The levels are visited colour by colour; u_k is read in place, so the levels of earlier colours hold their new values.  The prior
sums run in scipy's order (a sparse matrix-vector product per colour), the device's in the order of its layout: tests/
test_gpu_locpar_ped.py bounds the difference.
"""
import copy
import os
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import locpar_reference as LP  # noqa: E402
from locpar_reference import LocparOracleEngine, LocparOracleEngine64  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO_PEDIGREE = os.path.join(ROOT, "tests", "golden", "demo_pedigree", "pedigree.txt")
LONG_ROW = 32                           # jwp::kLongRow: a row of V with more entries than this is summed by a wave
MAX_PAIRS = 10


def generate_pedigree(founders, generations, per_generation, sires, unknown_dam=0.1, seed=1):
    """(ids, sire, dam) with parents before offspring: `founders` animals without parents, then `generations` of `per_generation`
    offspring, each by one of `sires` sires and a dam (unknown with probability unknown_dam) drawn from ALL earlier animals -- so
    parents are often relatives (inbreeding); animal 0 is a sire in every generation, so its row of A-inverse is long."""
    rng = np.random.default_rng(seed)
    sire, dam = [-1] * founders, [-1] * founders
    for _ in range(generations):
        born = len(sire)
        pool = np.concatenate([[0], 1 + rng.choice(born - 1, size=sires - 1, replace=False)])      # animal 0 sires in every generation
        for _ in range(per_generation):
            sire.append(int(rng.choice(pool)))
            dam.append(-1 if rng.random() < unknown_dam else int(rng.integers(0, born)))
    return [f"a{i}" for i in range(len(sire))], np.array(sire), np.array(dam)


def structure_from_pedigree(ped):
    """A-inverse as api.set_random passes it on: rounded through Float32 (random_effects.jl:184), exactly symmetric, CSR."""
    from jwas_jl_amd import api
    return api.pedigree_structure(ped)


def greedy_colors(V):
    """Levels in ascending order, the smallest colour no neighbour holds (what the library does on the host)."""
    V = sp.csr_matrix(V)
    color = np.full(V.shape[0], -1, dtype=np.int32)
    for l in range(V.shape[0]):
        nb = V.indices[V.indptr[l]:V.indptr[l + 1]]
        held = set(color[nb[nb != l]].tolist())
        c = 0
        while c in held:
            c += 1
        color[l] = c
    return color


def prepare_structure(V, colors):
    """What structured_term_draw reads of a structure, formed once: the diagonal, the off-diagonal rows of every colour."""
    V = sp.csr_matrix(V)
    vdiag = V.diagonal()
    Voff = (V - sp.diags(vdiag)).tocsr()
    Voff.eliminate_zeros()
    levels = [np.flatnonzero(colors == c) for c in range(int(colors.max()) + 1)]
    return {"V": V, "Vabs": abs(V).tocsr(), "vdiag": vdiag, "colors": colors, "levels": levels, "nnz_l": np.diff(V.indptr),
            "rows": [Voff[L] for L in levels], "absrows": [abs(Voff[L]) for L in levels]}


def structured_term_draw(T, ordinal, r, sol, partner_offs, p_row, W, *, iteration, seed, vare, Rinv, normals=None):
    """The new values of the structured term T, colour by colour.  W: prepare_structure(V, colours); p_row: row `pos` of Gi, times
    vare in a one-trait model.  Returns (new, detail); detail holds what the parity bound is built from."""
    t = r.shape[0]
    k = T.trait
    # the data part: S, its absolute sum and d c_kk sol exactly as for an unstructured term (the prior is handled here)
    free = copy.copy(T)
    free.group = -1
    _, det = LP.term_draw(free, ordinal, r, sol, (), None, iteration=iteration, seed=seed, vare=vare, Rinv=Rinv, normals=normals)
    ckk = 1.0 if t == 1 else np.asarray(Rinv, dtype=np.float64).reshape(t, t)[k, k]
    s = float(vare) if t == 1 else 1.0
    nl = T.nlevels
    old = sol[T.off:T.off + nl].copy()
    cur = old.copy()
    pkk = p_row[T.pos]
    lhs = T.d * ckk + pkk * W["vdiag"]
    z = det["z"]
    # the partners' sums never change during the term; the own trait's are formed colour by colour from the current values
    fixed, Afix = np.zeros(nl), np.zeros(nl)
    for m, po in enumerate(partner_offs):
        if m != T.pos:
            um = sol[po:po + nl]
            fixed += p_row[m] * (W["V"] @ um)
            Afix += np.abs(p_row[m]) * (W["Vabs"] @ np.abs(um))
    mean, A = np.zeros(nl), np.zeros(nl)
    for L, rows, absrows in zip(W["levels"], W["rows"], W["absrows"]):
        num = det["S"][L] + T.d[L] * ckk * old[L] - fixed[L] - pkk * (rows @ cur)
        A[L] = det["A"][L] + Afix[L] + np.abs(pkk) * (absrows @ np.abs(cur))
        mean[L] = num / lhs[L]
        cur[L] = mean[L] + z[L] * np.sqrt(s / lhs[L])
    return cur, {"S": det["S"], "A": A, "lhs": lhs, "mean": mean, "sd": np.sqrt(s / lhs), "live": np.ones(nl, dtype=bool),
                 "n_l": det["n_l"] + len(partner_offs) * W["nnz_l"], "z": z, "pkk": pkk}


class _PedMixin:
    """locpar_set_group_structure / locpar_group_colors on the stand-ins of tests/locpar_reference.py."""

    @staticmethod
    def locpar_structure_estimate_bytes(nlevels, nnz):
        return 8 * (int(nlevels) + 1) + 12 * int(nnz) + 4 * int(nlevels) + 8 * MAX_PAIRS * (int(nlevels) // 256 + 1)

    def locpar_begin(self, ntraits=None):
        super().locpar_begin(ntraits)
        self._lp_struct = {}

    def locpar_set_group_structure(self, random_group, indptr, indices, values):
        g = int(random_group)
        if not 0 <= g < LP.MAX_GROUPS:
            raise ValueError("random_group outside 0 .. 7")
        if self._lp_final or self._lp_groups.get(g):
            raise RuntimeError("the structure is set before the effect's first member term")
        nl = len(indptr) - 1
        V = sp.csr_matrix((np.asarray(values, dtype=np.float64), np.asarray(indices), np.asarray(indptr)), shape=(nl, nl))
        if not V.has_sorted_indices or not np.all(np.isfinite(V.data)) or (V != V.T).nnz or np.any(V.diagonal() <= 0):
            raise ValueError("the structure must be finite, sorted and exactly symmetric with a positive diagonal")
        self._lp_struct[g] = prepare_structure(V, greedy_colors(V))

    def locpar_group_colors(self, random_group):
        return self._lp_struct[int(random_group)]["colors"].copy()

    def locpar_add_factor(self, trait, level, nlevels, random_group=-1):
        if random_group in self._lp_struct and self._lp_struct[random_group]["V"].shape[0] != nlevels:
            raise ValueError("the member differs from the structure's nlevels")
        super().locpar_add_factor(trait, level, nlevels, random_group)

    def locpar_step(self, *, iteration, seed, vare=None, Rinv=None, Gi=(), first_term=0, last_term=-1, details=None, normals=None):
        """The step of locpar_reference._LocparMixin with structured terms sampled colour by colour and their utu = U V U'.
        normals (tests only): {term ordinal: the normals to use instead of the counter's}."""
        t = self.ntraits
        nterms = len(self._lp_terms)
        last = nterms if last_term < 0 else int(last_term)
        if not self._lp_struct:
            return super().locpar_step(iteration=iteration, seed=seed, vare=vare, Rinv=Rinv, Gi=Gi, first_term=first_term, last_term=last_term,
                                       details=details)
        super().locpar_step(iteration=iteration, seed=seed, vare=vare, Rinv=Rinv, Gi=Gi, first_term=first_term, last_term=first_term)  # the checks
        Gi = [np.atleast_2d(np.asarray(M, dtype=np.float64)) for M in Gi]
        for j in range(first_term, last):
            T = self._lp_terms[j]
            if T.group in self._lp_struct:
                offs = [self._lp_terms[m].off for m in self._lp_groups[T.group]]
                row = Gi[T.group][T.pos] * (float(vare) if t == 1 else 1.0)
                new, det = structured_term_draw(T, j, self.r.astype(np.float64), self._lp_sol, offs, row, self._lp_struct[T.group], iteration=iteration,
                                                seed=seed, vare=vare, Rinv=Rinv, normals=None if normals is None else normals.get(j))
                delta = new - self._lp_sol[T.off:T.off + T.nlevels]
                self._lp_sol[T.off:T.off + T.nlevels] = new
                self.r[T.trait] = LP.term_apply(T, self.r[T.trait], delta, self.r.dtype)
                if details is not None:
                    det["delta"] = delta
                    details.append(det)
            else:
                super().locpar_step(iteration=iteration, seed=seed, vare=vare, Rinv=Rinv, Gi=Gi, first_term=j, last_term=j + 1, details=details)
        utu = []
        for g in sorted(self._lp_groups):
            U = np.stack([self._lp_sol[self._lp_terms[m].off:self._lp_terms[m].off + self._lp_terms[m].nlevels] for m in self._lp_groups[g]])
            utu.append(U @ (self._lp_struct[g]["V"] @ U.T) if g in self._lp_struct else U @ U.T)
        return {"utu": utu, "step_ms": 0.0}


class PedOracleEngine(_PedMixin, LocparOracleEngine):
    pass


class PedOracleEngine64(_PedMixin, LocparOracleEngine64):
    pass


def dense_mme_structured(terms, groups, structs, w, r, sol, *, vare=None, Rinv=None, Gi=()):
    """locpar_reference.dense_mme with kron(Gi, V) instead of kron(Gi, I) for the random effects that have a structure."""
    t = r.shape[0]
    A, b = LP.dense_mme(terms, {g: m for g, m in groups.items() if g not in structs}, w, r, sol, vare=vare, Rinv=Rinv, Gi=Gi)
    for g, members in groups.items():
        if g not in structs:
            continue
        G = np.atleast_2d(np.asarray(Gi[g], dtype=np.float64))
        Vd = np.asarray(sp.csr_matrix(structs[g]).todense())
        for a, ja in enumerate(members):
            for e, je in enumerate(members):
                Ta, Te = terms[ja], terms[je]
                A[Ta.off:Ta.off + Ta.nlevels, Te.off:Te.off + Te.nlevels] += Vd * (G[a, e] * (vare if t == 1 else 1.0))
    return A, b


def reference_scan_in_order(A, x, b, z, order, vare=None):
    """Gibbs(A, x, b[, vare]) of iterative_solver/solver.jl:143-162 with the equations visited in `order`, fed the normals z."""
    x = x.copy()
    for i in order:
        if A[i, i] != 0.0:
            invlhs = 1.0 / A[i, i]
            mu = invlhs * (b[i] - A[:, i] @ x) + x[i]
            x[i] = z[i] * np.sqrt(invlhs * (vare if vare is not None else 1.0)) + mu
    return x


# ---- the exact-posterior case of the issue: intercept + a 200-animal pedigree term, weights, fixed variances ----------------------
POSTERIOR_STEPS, POSTERIOR_BURNIN, POSTERIOR_BATCHES, POSTERIOR_SEED = 4000, 200, 40, 7


def ped200():
    from jwas_jl_amd.single_step import Pedigree
    return Pedigree(*generate_pedigree(20, 3, 60, 3, 0.1, seed=200))


def posterior_case():
    rng = np.random.default_rng(201)
    ped = ped200()
    V = structure_from_pedigree(ped)
    q, n = len(ped.ids), 300
    lev = rng.integers(0, q, n).astype(np.int32)
    u = rng.standard_normal(q) * 0.8
    w = rng.uniform(0.5, 2.0, n)
    y = 1.0 + u[lev] + rng.standard_normal(n) / np.sqrt(w)
    return {"n": n, "q": q, "V": V, "level": lev, "w": w, "y": y, "vare": 1.0, "Gi": [np.array([[1.5]])], "X": rng.standard_normal((n, 8))}


def posterior_setup(engine, case):
    dtype = np.float64
    engine.load_dense(np.asfortranarray(case["X"], dtype=dtype))
    engine.set_weights(case["w"].astype(dtype))
    engine.setup_blocks(8 if not hasattr(engine, "_L") else 64, "f64")
    engine.init_state("BayesC", 1)
    engine.set_residual(case["y"].astype(dtype), 0)
    engine.locpar_begin(1)
    V = case["V"]
    engine.locpar_set_group_structure(0, V.indptr, V.indices, V.data)
    engine.locpar_add_covariate(0, None)
    engine.locpar_add_factor(0, case["level"], case["q"], 0)
    return engine


def posterior_z(engine, case, seed=POSTERIOR_SEED):
    """|chain mean - solve| in batch-means standard errors for every entry of sol: POSTERIOR_STEPS steps after POSTERIOR_BURNIN."""
    q = case["q"]
    terms = [LP.Term(0, None, None, 1, -1, 0, 0, case["w"]), LP.Term(0, None, case["level"], q, 0, 0, 1, case["w"])]
    A, b = dense_mme_structured(terms, {0: [1]}, {0: case["V"]}, case["w"], case["y"][None, :].astype(np.float64), np.zeros(q + 1),
                                vare=case["vare"], Gi=case["Gi"])
    solve = np.linalg.solve(A, b)
    chain = np.empty((POSTERIOR_STEPS, q + 1))
    for it in range(1, POSTERIOR_BURNIN + POSTERIOR_STEPS + 1):
        engine.locpar_step(iteration=it, seed=seed, vare=case["vare"], Gi=case["Gi"])
        if it > POSTERIOR_BURNIN:
            chain[it - POSTERIOR_BURNIN - 1] = engine.locpar_get_sol()
    bm = chain.reshape(POSTERIOR_BATCHES, -1, q + 1).mean(axis=1)
    se = bm.std(axis=0, ddof=1) / np.sqrt(POSTERIOR_BATCHES)
    return np.abs(chain.mean(axis=0) - solve) / se
