"""The relationship matrix of 2-bit packed genotypes on the device (csrc/gblup.hpp k_grm_packed, jwas_hip_grm_packed2bit,
HipEngine.grm_packed) and api.genomic_relationship_matrix on PLINK filesets, .jgb2 backends and resident Genotypes objects.

1. Bit identity: grm_packed of a packed engine equals grm of a dense engine loaded with the columns the packed one decodes
   (get_columns), K == K' bit for bit, and K is within the project's derived bound (gblup_reference.grm_bound: (c + 2) 2^-24
   (sum_k |z_ik z_jk| + 1e-5) / p) of the double restatement on the decoded columns.  n = 7 (one tile), 129 (a ragged second tile),
   301 (six tiles), 258 (n % 4 != 0 across slices); p = c + 13 (a chunk fold and a ragged tail) and 5 (less than one LDS tile); centred
   and uncentred storage; about 3 % missing codes, one byte all missing, one marker missing for a whole 128-row panel.
2. The stray fields of a marker's last byte (n = 301: three of them) set to 1, 2, 3: the same bits.
3. Two calls give equal bits and leave storage_info() and the payload as they were.
4. The codes returned before any launch.
5. The whole path: a 64 x 200 fileset without missing values (every marker mean is k / 64, exact in Float32 on both paths) gives the
   text path's matrix bit for bit from input_format="plink", from plink_genotypes' object and from input_format="stream"; a fileset
   with missing genotypes and a reordered keep subset returns keep's order within the derived bound; the result runs through
   get_genotypes(K, G, method="GBLUP") and runMCMC.
Every test prints what it measured before it asserts."""
import contextlib
import functools
import io

import numpy as np
import pytest

import gblup_reference as GR
import grm_packed_reference as PKR
import plink_reference as PR

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, EUNSUP = -1, -3, -4


def _hip(precision=32):
    import jwas_jl_amd as J
    return J.HipEngine(0, precision=precision)


@functools.lru_cache(maxsize=None)
def _case(n, p, seed=None):
    """(payload p x cld(n,4), means, divisor) of PKR.case_codes; read-only."""
    codes, means = PKR.case_codes(n, p, seed=n + p if seed is None else seed)
    payload, d = PR.pack_codes(codes), PKR.divisor_of(means)
    for a in (payload, means, d):
        a.setflags(write=False)
    return payload, means, d


def _quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


# ---- 1. bit identity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("centered", [True, False])
@pytest.mark.parametrize("p", [GR._GblupMixin.GRM_CHUNK + 13, 5])
@pytest.mark.parametrize("n", [7, 129, 301, 258])
def test_packed_equals_dense_bit_for_bit(n, p, centered):
    import jwas_jl_amd as J
    c = J.HipEngine.GRM_CHUNK
    assert c == GR._GblupMixin.GRM_CHUNK
    payload, means, d = _case(n, p)
    packed, dense = _hip(), _hip()
    try:
        packed.load_packed2bit(payload, n, means, centered=centered)
        X = packed.get_columns(0, p)
        Kp = packed.grm_packed(d)
        dense.load_dense(X)
        Kd = dense.grm(d)
    finally:
        packed.close()
        dense.close()
    want = PKR.decode(PKR.unpack(payload, n), means, centered)
    ref, absZZ = GR.grm_reference(X, d)
    bound = GR.grm_bound(absZZ, p, np.float32, c)
    err = np.abs(Kp.astype(np.float64) - ref)
    print(f"grm_packed n={n} p={p} centered={centered}: equal to dense {np.array_equal(Kp, Kd)} ({int((Kp != Kd).sum())} of {n * n} differ); "
          f"symmetric {np.array_equal(Kp, Kp.T)}; worst error / bound {np.max(err / bound):.3f}; decode equal {np.array_equal(X, want)}")
    assert Kp.dtype == np.float32 and Kp.shape == (n, n)
    assert np.array_equal(X, want)                                  # (the dense engine holds what the storage decodes to)
    assert np.array_equal(Kp, Kd)
    assert np.array_equal(Kp, Kp.T)
    assert np.all(err <= bound)


# ---- 2. stray fields --------------------------------------------------------------------------------------------------------------------
def test_stray_fields_of_the_last_byte_are_not_read():
    n, p = 301, GR._GblupMixin.GRM_CHUNK + 13
    payload, means, d = _case(n, p)
    used = n & 3                                                    # fields of the last byte that are rows
    assert used == 1 and not np.any(payload[:, -1] >> (2 * used))   # three stray fields, clean in the case's payload
    variants = {"1": (1, 1, 1), "2": (2, 2, 2), "3": (3, 3, 3), "1,2,3": (1, 2, 3)}
    hip = _hip()
    try:
        hip.load_packed2bit(payload, n, means)
        clean = hip.grm_packed(d)
        same = {}
        for name, fields in variants.items():
            dirty = payload.copy()
            for k, f in enumerate(fields):
                dirty[:, -1] |= np.uint8(f << (2 * (used + k)))
            hip.load_packed2bit(dirty, n, means)
            assert np.array_equal(hip.get_packed2bit(0, p), dirty)  # (the strays are in the storage)
            same[name] = np.array_equal(hip.grm_packed(d), clean)
    finally:
        hip.close()
    print(f"stray fields n={n} p={p}: K equal to the clean payload's {same}")
    assert all(same.values())


# ---- 3. two calls, and what a call leaves behind ------------------------------------------------------------------------------------------
def test_two_calls_are_equal_and_leave_the_storage_alone():
    n, p = 258, GR._GblupMixin.GRM_CHUNK + 13
    payload, means, d = _case(n, p)
    hip = _hip()
    try:
        hip.load_packed2bit(payload, n, means, centered=False)
        info0, q0, x0 = hip.storage_info(), hip.get_packed2bit(0, p), hip.get_columns(0, p)
        K1 = hip.grm_packed(d)
        K2 = hip.grm_packed(d)
        info1, q1, x1 = hip.storage_info(), hip.get_packed2bit(0, p), hip.get_columns(0, p)
    finally:
        hip.close()
    print(f"two calls n={n} p={p}: equal {np.array_equal(K1, K2)}; storage_info {info0} -> {info1}; payload equal {np.array_equal(q0, q1)}; "
          f"columns equal {np.array_equal(x0, x1)}")
    assert np.array_equal(K1, K2)
    assert info0 == info1 and info0["kind"] == "packed2bit"
    assert np.array_equal(q0, q1) and np.array_equal(q0, payload) and np.array_equal(x0, x1)


# ---- 4. return codes ------------------------------------------------------------------------------------------------------------------------
def test_return_codes():
    import ctypes as C
    from jwas_jl_amd import _lib
    n, p = 129, 40
    payload, means, d = _case(n, p)

    def code(fn, *a, **kw):
        with pytest.raises(_lib.JwasHipError) as ei:
            fn(*a, **kw)
        return ei.value.code

    got = {}
    L = _lib.load()
    K = np.empty((n, n), dtype=np.float32)
    dp, Kp = d.ctypes.data_as(C.c_void_p), K.ctypes.data_as(C.c_void_p)
    hip = _hip()
    try:
        hip.n, hip.p = n, p
        got["empty context"] = code(hip.grm_packed, d)
        hip.load_dense(np.zeros((n, p), dtype=np.float32, order="F"))
        got["dense context"] = code(hip.grm_packed, d)
        hip.load_packed2bit(payload, n, means)
        for bad in (0.0, -1.0, np.inf, np.nan):
            d2 = d.copy()
            d2[17] = bad
            got[f"divisor {bad}"] = code(hip.grm_packed, d2)
        got["NULL context"] = L.jwas_hip_grm_packed2bit(None, dp, Kp)
        got["NULL divisor"] = L.jwas_hip_grm_packed2bit(hip._h, None, Kp)
        got["NULL K"] = L.jwas_hip_grm_packed2bit(hip._h, dp, None)
        hip.comm_init_loopback(0, 0, 1)
        got["loopback shards"] = code(hip.grm_packed, d)
        hip.comm_destroy()
        K_after = hip.grm_packed(d)                                 # the refusals left the context usable
    finally:
        hip.close()
    f64 = _hip(64)
    try:
        f64.n, f64.p = n, p
        got["Float64 engine"] = code(f64.grm_packed, d)
    finally:
        f64.close()
    print(f"jwas_hip_grm_packed2bit codes: {got}")
    want = {"empty context": ESTATE, "dense context": ESTATE, "Float64 engine": EUNSUP, "loopback shards": EUNSUP, "NULL context": EINVAL,
            "NULL divisor": EINVAL, "NULL K": EINVAL, "divisor 0.0": EINVAL, "divisor -1.0": EINVAL, "divisor inf": EINVAL, "divisor nan": EINVAL}
    assert got == want
    assert np.array_equal(K_after, K_after.T)


# ---- 5. the whole path ----------------------------------------------------------------------------------------------------------------------
def _counts(n, p, seed, missing=0.0):
    """n x p copies of A1 (9 = missing); marker 3 is fixed and marker 7 has one copy: quality control drops both."""
    rng = np.random.default_rng(seed)
    G = rng.binomial(2, 0.2 + 0.6 * rng.random(p), size=(n, p)).astype(np.int64)
    G[:, 3] = 0
    G[:, 7] = 0
    G[5, 7] = 1
    if missing:
        G[rng.random((n, p)) < missing] = 9
    return G


def test_fileset_stream_and_resident_object_equal_the_text_path(tmp_path):
    import pandas as pd
    from jwas_jl_amd import api, streaming
    n, p = 64, 200
    G = _counts(n, p, seed=5)
    prefix = str(tmp_path / "geno")
    ids, markers, _, _ = PR.write_fileset(prefix, G)
    table = pd.DataFrame(G.astype(np.float64), columns=markers)
    table.insert(0, "ID", ids)
    text = _quiet(api.genomic_relationship_matrix, table)
    plink = _quiet(api.genomic_relationship_matrix, prefix, input_format="plink")
    geno = _quiet(api.plink_genotypes, prefix)
    try:
        resident = _quiet(api.genomic_relationship_matrix, geno)
        info = geno.device_backend.storage_info()
    finally:
        geno.device_backend.close()
    out = _quiet(streaming.prepare_streaming_genotypes, prefix, str(tmp_path / "backend"), input_format="plink")
    stream = _quiet(api.genomic_relationship_matrix, out, input_format="stream")
    Kt = text.iloc[:, 1:].to_numpy()
    same = {name: (list(f.columns) == list(text.columns) and list(f["ID"]) == list(text["ID"]), np.array_equal(f.iloc[:, 1:].to_numpy(), Kt))
            for name, f in (("plink", plink), ("resident", resident), ("stream", stream))}
    print(f"whole path {n} x {p} ({geno.nMarkers} markers kept): (labels, bits) equal to the text path {same}; resident storage {info}")
    assert Kt.dtype == np.float32 and Kt.shape == (n, n) and geno.nMarkers == p - 2
    assert info["kind"] == "packed2bit"
    assert all(a and b for a, b in same.values())


def test_keep_order_missing_genotypes_and_a_gblup_run(tmp_path):
    import pandas as pd
    import jwas_jl_amd as J
    from jwas_jl_amd import api, plink
    n, p = 80, 200
    G = _counts(n, p, seed=9, missing=0.03)
    prefix = str(tmp_path / "geno")
    ids, _, _, _ = PR.write_fileset(prefix, G)
    rng = np.random.default_rng(1)
    keep = [ids[i] for i in rng.permutation(n)[:64]]
    Kdf = _quiet(api.genomic_relationship_matrix, prefix, input_format="plink", keep=keep)
    hip = _hip()
    try:
        b = _quiet(plink.load_plink, hip, prefix, keep=keep)
        X = hip.get_columns(0, hip.p)
    finally:
        hip.close()
    d = PKR.divisor_of(b["marker_means"])
    K = Kdf.iloc[:, 1:].to_numpy()
    ref, absZZ = GR.grm_reference(X, d)
    bound = GR.grm_bound(absZZ, X.shape[1], np.float32, J.HipEngine.GRM_CHUNK)
    err = np.abs(K.astype(np.float64) - ref)
    print(f"keep subset {len(keep)} of {n}, {X.shape[1]} of {p} markers kept, {int((G == 9).sum())} missing: IDs in keep's order "
          f"{list(Kdf['ID']) == keep}; worst error / bound {np.max(err / bound):.3f}")
    assert list(Kdf["ID"]) == keep and list(Kdf.columns[1:]) == keep
    assert np.array_equal(d, np.sqrt(np.float32(2.0) * b["allele_freq"] * (np.float32(1.0) - b["allele_freq"])))
    assert K.dtype == np.float32 and np.array_equal(K, K.T) and np.all(err <= bound)
    geno = _quiet(api.get_genotypes, Kdf, 1.0, method="GBLUP")
    model = api.build_model("y1 = intercept + geno", genotypes={"geno": geno})
    ph = pd.DataFrame({"ID": keep, "y1": 1.0 + rng.standard_normal(len(keep))})
    out = _quiet(api.runMCMC, model, ph, chain_length=20, seed=3, output_folder=str(tmp_path / "run"))
    ebv = out["EBV_y1"]
    print(f"GBLUP run on it: {len(ebv)} EBVs, finite {np.isfinite(ebv['EBV'].to_numpy(dtype=np.float64)).all()}")
    assert sorted(str(v) for v in ebv["ID"]) == sorted(keep)
    assert np.isfinite(ebv["EBV"].to_numpy(dtype=np.float64)).all()
    for key in ("marker effects geno", "residual variance", "genetic_variance"):
        assert np.isfinite(out[key]["Estimate"].to_numpy(dtype=np.float64)).all(), key
