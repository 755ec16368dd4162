"""HipEngine: numpy-facing wrapper over the C ABI -- the device side of the marker sweep.

The host MCMC loop (jwas.jl_amd/mcmc.py) drives a *sweep engine* through this small protocol:

    load_dense(X) / alloc_dense(n,p) + synth(...)      genotype storage      (Genotypes.genotypes)
    setup_blocks(block_size, gram_mode)                x'x + block Grams     (GibbsMats)
    xpx() / gram(i) / set_gram(i, G)
    init_state(method, ntraits); set_state/get_state   alpha, beta, delta
    set_residual/get_residual(trait)                   ycorr
    sub_xalpha(trait); mul_alpha(trait)
    sweep(**params) -> dict of reductions              BayesABC!/BayesR!/MTBayesABC!
    accumulate(k); posterior(trait)                    running posterior means
    liability_begin / set_categorical / set_censored / set_thresholds / liability_init / liability_sample /
    liability_minmax / liabilities / liability_end     threshold and censored traits (sample_liabilities!)

HipEngine is the only engine the package ships; it raises if libjwas_hip.so or the GPU is missing.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import JwasHipError, SweepParams, SweepStats

METHOD_CODES = {"BayesC": _lib.BAYESC, "BayesB": _lib.BAYESB, "BayesA": _lib.BAYESB,
                "BayesR": _lib.BAYESR, "MTBayesC": _lib.MTBAYESC1, "MTBayesC_II": _lib.MTBAYESC2,
                "MegaBayesC": _lib.MEGABAYESC, "MTBayesB": _lib.MTBAYESB1, "MTBayesB_II": _lib.MTBAYESB2, "MegaBayesB": _lib.MEGABAYESB}
BAYESR_GAMMA = np.array([0.0, 0.01, 0.1, 1.0], dtype=np.float64)   # JWAS.jl:12


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _csr_arrays(M):
    """(indptr int64, indices int32, data float64) of a sparse matrix as CSR with sorted columns; a triple goes through as it is."""
    if isinstance(M, (tuple, list)):
        ptr, col, val = M
    else:
        M = M.tocsr().copy()
        M.sum_duplicates()
        M.sort_indices()
        ptr, col, val = M.indptr, M.indices, M.data
    return np.ascontiguousarray(ptr, dtype=np.int64), np.ascontiguousarray(col, dtype=np.int32), np.ascontiguousarray(val, dtype=np.float64)


class SectionSolvePolicy:
    """When the host sets jwas_sweep_params.section_solve (Rule T) along a chain.  A multi-trait sampler-I chain that starts from
    the reference's default prior (every marker in the model) drifts, with Pi estimated, towards sparser joint states; once
    most 64-marker sections hold more markers outside the model than the rule takes as exceptions, the per-sweep section
    inverses and the lazily fetched Gram tiles are pure overhead.  The rule is therefore switched off for `probe` sweeps when
    the last sweep solved fewer than half of its sections, and tried again afterwards (speed only: on or off, a sweep samples
    the same conditionals)."""

    def __init__(self, enabled, nsections, probe=50, probe_max=800):
        self.enabled, self.nsections, self.probe, self.probe_max = bool(enabled), int(nsections), int(probe), int(probe_max)
        self.probe0 = self.probe
        self.off_until = 0

    def use(self, it):
        return self.enabled and it >= self.off_until

    def observe(self, it, engine, ran=True):
        """After sweep `it`.  ran: the sweep really passed section_solve (a sweep on another block size did not, and its
        counter 16 means something else -- reading it would switch the rule off without evidence)."""
        if not ran or not self.enabled or it < self.off_until or not hasattr(engine, "last_sweep_counters"):
            return
        if engine.last_sweep_counters()[16] * 2 < self.nsections:
            # (a probe sweep that fails costs more than a sweep without the rule: back off -- 50, 100, 200 ... sweeps between tries)
            self.off_until = it + 1 + self.probe
            self.probe = min(2 * self.probe, self.probe_max)
        else:
            self.probe = self.probe0


class HipEngine:
    def __init__(self, device=0, precision=32):
        """precision: 32 (the reference's default Float32 path) or 64 (runMCMC(double_precision=true): a Float64 context --
        genotypes, residual, effects and the samplers' arithmetic all in double; jwas_hip_set_precision)."""
        if precision not in (32, 64):
            raise ValueError("precision must be 32 or 64")
        self._L = _lib.load()
        h = C.c_void_p()
        rc = self._L.jwas_hip_create(int(device), C.byref(h))
        if rc != 0:
            raise JwasHipError(rc, self._L.jwas_hip_last_error(None).decode())
        self._h = h
        self.precision = int(precision)
        self.dtype = np.float64 if precision == 64 else np.float32
        if precision == 64:
            rc = self._L.jwas_hip_set_precision(h, 64)
            if rc != 0:
                raise JwasHipError(rc, self._L.jwas_hip_last_error(h).decode())
        self.device = int(device)
        self.n = self.p = 0
        self.method = None
        self.ntraits = 0
        self.block_size = 0
        self._keep = []   # host arrays referenced by the last sweep call
        self._weighted = False          # non-unit residual weights on the device (set_weights)
        self._explicit_starts = None    # explicit block partition resident (setup_blocks_explicit)
        self._rrm = None                # (T, c, block size) of an open random-regression session
        self._mega = None               # (traits, block size) of an open mega-trait session
        self._mtj = None                # ... of an open joint multi-trait session (mtj_begin)
        self._ss = None                 # (non-genotyped, genotyped, markers per chunk) of an open single-step imputation session

    # -- plumbing --------------------------------------------------------------------------------
    def _chk(self, rc):
        if rc != 0:
            raise JwasHipError(rc, self._L.jwas_hip_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None):
            self._L.jwas_hip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_handle):
        self._chk(self._L.jwas_hip_set_stream(self._h, C.c_void_p(int(stream_handle))))

    def device_info(self):
        ncu, tot, free = C.c_int(), C.c_int64(), C.c_int64()
        self._chk(self._L.jwas_hip_device_info(self._h, C.byref(ncu), C.byref(tot), C.byref(free)))
        return {"n_cu": ncu.value, "hbm_total": tot.value, "hbm_free": free.value}

    @staticmethod
    def estimate_bytes(n, p, ntraits=1, block_size=256, storage="dense"):
        kind = _lib.STORAGE_PACKED2BIT if storage in ("stream", "packed2bit") else _lib.STORAGE_DENSE_F32
        return _lib.load().jwas_hip_estimate_bytes_storage(int(n), int(p), int(ntraits), int(block_size), kind)

    # -- storage ---------------------------------------------------------------------------------
    def load_dense(self, X):
        """X: n x p float32.  Fortran order is uploaded as is (marker-major, zero re-layout)."""
        X = np.asarray(X)
        if X.dtype != self.dtype:
            raise TypeError(f"this engine stores {np.dtype(self.dtype).name} genotypes (double_precision={'true' if self.precision == 64 else 'false'})")
        if X.ndim != 2:
            raise ValueError("genotype matrix must be 2-D")
        if not X.flags.f_contiguous:
            X = np.asfortranarray(X)
        n, p = X.shape
        self._chk((self._L.jwas_hip_load_dense_f64 if self.precision == 64 else self._L.jwas_hip_load_dense_f32)(self._h, _ptr(X), n, p, n))
        self.n, self.p = n, p
        self.method, self.block_size = None, 0

    def alloc_dense(self, n, p):
        self._chk(self._L.jwas_hip_alloc_dense_f32(self._h, int(n), int(p)))
        self.n, self.p = int(n), int(p)
        self.method, self.block_size = None, 0

    # 2-bit packed storage (the reference's Packed2BitBackend kept packed in HBM) ----------------
    def load_packed2bit(self, payload, n, means, centered=True):
        """payload: p x stride uint8 (marker-major rows, stride >= cld(n,4)); means: p float32."""
        payload = np.ascontiguousarray(payload, dtype=np.uint8)
        if payload.ndim != 2:
            raise ValueError("payload must be a p x stride_bytes uint8 array")
        means = np.ascontiguousarray(means, dtype=np.float32)
        p, stride = payload.shape
        if means.shape != (p,):
            raise ValueError("one marker mean per packed marker is required")
        self._chk(self._L.jwas_hip_load_packed2bit(self._h, _ptr(payload), int(n), p, stride, _ptr(means), int(bool(centered))))
        self.n, self.p = int(n), p
        self.method, self.block_size = None, 0

    def load_jgb2(self, path):
        """load_streaming_backend (streaming_genotypes.jl:884-971): prefix, or <prefix>.meta / <prefix>.jgb2."""
        self._chk(self._L.jwas_hip_load_jgb2(self._h, str(path).encode()))
        info = self.storage_info()
        self.n, self.p = info["n"], info["p"]
        self.method, self.block_size = None, 0

    def alloc_packed(self, n, p, centered=True):
        self._chk(self._L.jwas_hip_alloc_packed2bit(self._h, int(n), int(p), int(bool(centered))))
        self.n, self.p = int(n), int(p)
        self.method, self.block_size = None, 0

    # PLINK 1 binary filesets (jwas_hip_plink_*; the host side is plink.load_plink) ----------------
    def plink_scan(self, bed_path, n_file, p_file, rows=None, count_a1=True):
        """Transcodes every marker of a variant-major .bed file into a staging buffer on the device.  rows: the file rows of the
        individuals to keep, in the order wanted (None: all, file order).  Returns p_file x 4 int64: the kept individuals of every
        marker with code 0, 1, 2 (copies of the counted allele) and 3 (missing).  plink_commit / plink_discard end the scan."""
        r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64)
        counts = np.empty((int(p_file), 4), dtype=np.int64)
        self._chk(self._L.jwas_hip_plink_scan(self._h, str(bed_path).encode(), int(n_file), int(p_file), _ptr(r), 0 if r is None else r.size,
                                              int(bool(count_a1)), _ptr(counts)))
        self._scan_rows = int(n_file) if r is None else int(r.size)      # (what plink_commit_output's rows will number)
        return counts

    def plink_commit(self, selected, means, centered=True):
        """The scanned markers `selected` (0-based file indices, strictly ascending) become the context's packed storage."""
        sel = np.ascontiguousarray(selected, dtype=np.int64)
        means = np.ascontiguousarray(means, dtype=np.float32)
        if sel.ndim != 1 or means.shape != sel.shape:
            raise ValueError("one marker mean per selected marker is required")
        self._chk(self._L.jwas_hip_plink_commit(self._h, _ptr(sel), sel.size, _ptr(means), int(bool(centered))))
        info = self.storage_info()
        self.n, self.p = info["n"], info["p"]
        self.method, self.block_size = None, 0

    def plink_discard(self):
        self._chk(self._L.jwas_hip_plink_discard(self._h))

    def get_packed2bit(self, j0, count):
        """The packed rows of markers [j0, j0 + count): count x cld(n,4) uint8, the payload of a .jgb2 file."""
        out = np.empty((int(count), (self.n + 3) // 4), dtype=np.uint8)
        self._chk(self._L.jwas_hip_get_packed2bit(self._h, int(j0), int(count), _ptr(out), out.shape[1]))
        return out

    # Output rows in 2-bit packed storage beside packed training storage (the host side is plink.load_plink_output) ----------------
    def _need_f32_packed(self, what):
        if self.precision != 32:
            raise ValueError(f"{what} needs a Float32 engine (2-bit packed storage has no Float64 path)")

    def load_output_packed2bit(self, payload, n_out):
        """The rows EBVs are reported for as a second packed matrix, decoded with the training storage's means and centring.
        payload: p x stride uint8 in the .jgb2 field layout (stride >= cld(n_out,4))."""
        self._need_f32_packed("load_output_packed2bit")
        payload = np.ascontiguousarray(payload, dtype=np.uint8)
        if payload.ndim != 2:
            raise ValueError("payload must be a p x stride_bytes uint8 array")
        p, stride = payload.shape
        self._chk(self._L.jwas_hip_load_output_packed2bit(self._h, _ptr(payload), int(n_out), p, stride))
        self.n_out = int(n_out)

    def plink_commit_output(self, selected):
        """The individuals of the pending plink_scan become the packed output rows: the scanned markers `selected`, which is the
        training selection (the scan ran with the training's counted allele)."""
        self._need_f32_packed("plink_commit_output")
        sel = np.ascontiguousarray(selected, dtype=np.int64)
        if sel.ndim != 1:
            raise ValueError("selected must be a vector of file marker indices")
        self._chk(self._L.jwas_hip_plink_commit_output(self._h, _ptr(sel), sel.size))
        self.n_out = self._scan_rows

    def get_output_packed2bit(self, j0, count):
        """The packed output rows of markers [j0, j0 + count): count x cld(n_out,4) uint8."""
        self._need_f32_packed("get_output_packed2bit")
        out = np.empty((int(count), (getattr(self, "n_out", 0) + 3) // 4), dtype=np.uint8)
        self._chk(self._L.jwas_hip_get_output_packed2bit(self._h, int(j0), int(count), _ptr(out), out.shape[1]))
        return out

    def ebv_output(self):
        """EBV = output_genotypes * alpha (output.jl:281-306) of every trait in one call: ntraits x n_out, row k = mul_alpha_output(k)."""
        self._need_f32_packed("ebv_output")
        out = np.empty((int(self.ntraits), getattr(self, "n_out", 0)), dtype=np.float32)
        self._chk(self._L.jwas_hip_ebv_output(self._h, _ptr(out)))
        return out

    def storage_info(self):
        k, n, p, b = C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64()
        self._chk(self._L.jwas_hip_storage_info(self._h, C.byref(k), C.byref(n), C.byref(p), C.byref(b)))
        return {"kind": "packed2bit" if k.value == _lib.STORAGE_PACKED2BIT else "dense_f32", "n": n.value, "p": p.value,
                "bytes": b.value}

    def set_xpx(self, xpx):
        x = np.ascontiguousarray(xpx, dtype=np.float32)
        if x.shape != (self.p,):
            raise ValueError(f"x'x must have length {self.p}")
        self._chk(self._L.jwas_hip_set_xpx(self._h, _ptr(x)))

    def set_weights(self, rinv):
        """Residual weights R^-1 = 1 ./ weights (build_MME.jl:305-310); None = unit.  Call before setup_blocks."""
        if rinv is None:
            self._chk(self._L.jwas_hip_set_weights(self._h, None))
        else:
            w = np.ascontiguousarray(rinv, dtype=self.dtype)             # Float64 contexts keep the weights' Float64 values (build_MME.jl:310)
            if w.shape != (self.n,):
                raise ValueError(f"one weight per individual is required ({self.n}), got {w.shape}")
            self._chk((self._L.jwas_hip_set_weights_f64 if self.precision == 64 else self._L.jwas_hip_set_weights)(self._h, _ptr(w)))
        self._weighted = rinv is not None
        self.block_size = 0

    def synth(self, seed, kind=0, center=True, marker_offset=0):
        self._chk(self._L.jwas_hip_synth_genotypes(self._h, int(seed), int(kind), int(bool(center)), int(marker_offset)))

    def synth_single_step(self, seed, n_genotyped, center=True, marker_offset=0):
        """Config-5 shaped input: rows < n_genotyped are 0/1/2 genotypes, the rest real-valued 'imputed' rows."""
        self._chk(self._L.jwas_hip_synth_single_step(self._h, int(seed), int(n_genotyped), int(bool(center)), int(marker_offset)))

    def layout(self):
        n, p, ld, ptr = C.c_int64(), C.c_int64(), C.c_int64(), C.c_void_p()
        self._chk(self._L.jwas_hip_dense_layout(self._h, C.byref(n), C.byref(p), C.byref(ld), C.byref(ptr)))
        return {"n": n.value, "p": p.value, "ld": ld.value, "ptr": ptr.value}

    def get_columns(self, j0, count):
        out = np.empty((self.n, int(count)), dtype=np.float32, order="F")
        self._chk(self._L.jwas_hip_get_columns(self._h, int(j0), int(count), _ptr(out)))
        return out

    def set_columns(self, j0, cols):
        """Overwrite columns [j0, j0 + cols.shape[1]) of an allocated dense matrix (n x count float32, any order)."""
        cols = np.asfortranarray(cols, dtype=np.float32)
        if cols.ndim != 2 or cols.shape[0] != self.n:
            raise ValueError(f"column chunk must be {self.n} x count")
        self._chk(self._L.jwas_hip_set_columns(self._h, int(j0), int(cols.shape[1]), _ptr(cols), self.n))
        self.block_size = 0

    # -- precompute ------------------------------------------------------------------------------
    def setup_blocks(self, block_size=256, gram_mode="mfma"):
        mode = {"f64": _lib.GRAM_F64, "mfma": _lib.GRAM_MFMA}[gram_mode]
        self._chk(self._L.jwas_hip_setup_blocks(self._h, int(block_size), mode))
        self.block_size = int(block_size)
        self._resident = [int(block_size)]
        self._groups = {}
        self._explicit_starts = None

    def setup_blocks_explicit(self, starts, gram_mode="mfma"):
        """Explicit, possibly non-uniform block partition (fast_blocks = a vector of block starts, JWAS.jl:298-304):
        `starts` = 0-based first marker of every block, starts[0] = 0, strictly increasing, blocks of <= 1024 markers."""
        mode = {"f64": _lib.GRAM_F64, "mfma": _lib.GRAM_MFMA}[gram_mode]
        st = np.ascontiguousarray(starts, dtype=np.int64)
        self._chk(self._L.jwas_hip_setup_blocks_explicit(self._h, st.ctypes.data_as(C.POINTER(C.c_int64)), len(st), mode))
        nb, bs = C.c_int64(0), C.c_int32(0)
        self._chk(self._L.jwas_hip_num_blocks(self._h, C.byref(nb), C.byref(bs)))
        self.block_size = int(bs.value)
        self._resident = [self.block_size]
        self._groups = {}
        self._explicit_starts = st.copy()

    def add_block_size(self, block_size, gram_mode="mfma"):
        """Make a second block size resident (see jwas_hip_add_block_size); select_block_size switches between sweeps."""
        mode = {"f64": _lib.GRAM_F64, "mfma": _lib.GRAM_MFMA}[gram_mode]
        self._chk(self._L.jwas_hip_add_block_size(self._h, int(block_size), mode))
        self._resident.append(int(block_size))

    def setup_groups(self, blocks_per_launch, gram_mode="mfma"):
        """Grouped launches for the selected block size (jwas_hip_setup_groups): 2 or 4 consecutive blocks per launch of the step
        kernel, used by the sweeps that pass group_launch=True; 0 frees the buffers."""
        mode = {"f64": _lib.GRAM_F64, "mfma": _lib.GRAM_MFMA}[gram_mode]
        self._chk(self._L.jwas_hip_setup_groups(self._h, int(blocks_per_launch), mode))
        self._groups = dict(getattr(self, "_groups", {}))
        self._groups[self.block_size] = int(blocks_per_launch)

    def blocks_per_launch(self, block_size=None):
        """Blocks per grouped launch set up for a block size (0: none)."""
        return getattr(self, "_groups", {}).get(self.block_size if block_size is None else int(block_size), 0)

    def resident_block_sizes(self):
        """Block sizes whose Grams are resident (setup_blocks / add_block_size)."""
        return list(getattr(self, "_resident", [])) if self.block_size else []

    def select_block_size(self, block_size):
        self._chk(self._L.jwas_hip_select_block_size(self._h, int(block_size)))
        self.block_size = int(block_size)

    @property
    def nblocks(self):
        nb, bs = C.c_int64(), C.c_int32()
        self._chk(self._L.jwas_hip_num_blocks(self._h, C.byref(nb), C.byref(bs)))
        return nb.value

    def block_starts(self):
        if getattr(self, "_explicit_starts", None) is not None:
            return self._explicit_starts.copy()
        return np.arange(0, self.p, self.block_size, dtype=np.int64)

    def _bsize(self, i):
        if getattr(self, "_explicit_starts", None) is not None:
            st = self._explicit_starts
            return int((st[i + 1] if i + 1 < len(st) else self.p) - st[i])
        j0 = i * self.block_size
        return min(self.block_size, self.p - j0)

    def xpx(self):
        out = np.empty(self.p, dtype=self.dtype)
        self._chk((self._L.jwas_hip_get_xpx_f64 if self.precision == 64 else self._L.jwas_hip_get_xpx)(self._h, _ptr(out)))
        return out

    def gram(self, i):
        b = self._bsize(i)
        out = np.empty((b, b), dtype=np.float32)
        self._chk(self._L.jwas_hip_get_gram(self._h, int(i), _ptr(out)))
        return out

    def set_gram(self, i, G):
        b = self._bsize(i)
        G = np.ascontiguousarray(G, dtype=np.float32)
        if G.shape != (b, b):
            raise ValueError(f"Gram block {i} must be {b} x {b}")
        self._chk(self._L.jwas_hip_set_gram(self._h, int(i), _ptr(G)))

    def set_cross_gram(self, i, C_):
        """Overwrite X_{i-1}' X_i (rows = markers of block i-1), i >= 1."""
        Cc = np.ascontiguousarray(C_, dtype=np.float32)
        if Cc.shape != (self._bsize(i - 1), self._bsize(i)):
            raise ValueError(f"cross-Gram of block {i} must be {self._bsize(i - 1)} x {self._bsize(i)}")
        self._chk(self._L.jwas_hip_set_cross_gram(self._h, int(i), _ptr(Cc)))

    def cross_gram(self, i):
        """X_{i-1}' X_i of the selected block size as the device holds it (rows = markers of block i-1), i >= 1."""
        buf = np.empty(max(1, self.block_size) ** 2, dtype=np.float32)
        self._chk(self._L.jwas_hip_get_cross_gram(self._h, 0, int(i), _ptr(buf)))
        bp, b = self._bsize(i - 1), self._bsize(i)
        return buf[:bp * b].reshape(bp, b).copy()

    def group_cross_gram(self, level, i):
        """The cross-Gram of grouped launches between group i-1 (rows) and group i (columns), i >= 1: level 1 = pairs of blocks,
        level 2 = fours.  At 4 blocks per launch only the odd pairs exist (jwas_hip_get_cross_gram)."""
        gb = (2 if int(level) == 1 else 4) * self.block_size
        out = np.empty((max(gb, 1), max(1, min(gb, self.p - int(i) * gb))), dtype=np.float32)
        self._chk(self._L.jwas_hip_get_cross_gram(self._h, int(level), int(i), _ptr(out)))
        return out

    def update_geometry(self):
        """(slices per row group, row groups, column groups) of the streaming role for this matrix."""
        a, b, c_ = C.c_int32(), C.c_int32(), C.c_int32()
        self._chk(self._L.jwas_hip_update_geometry(self._h, C.byref(a), C.byref(b), C.byref(c_)))
        return a.value, b.value, c_.value

    def set_grams_packed(self, grams):
        """grams: concatenated row-major b_i x b_i blocks (the oracle's packing)."""
        off = 0
        g = np.ascontiguousarray(grams, dtype=np.float32)
        for i in range(self.nblocks):
            b = self._bsize(i)
            self.set_gram(i, g[off:off + b * b].reshape(b, b))
            off += b * b

    # -- state -----------------------------------------------------------------------------------
    def init_state(self, method, ntraits=1):
        code = METHOD_CODES[method] if isinstance(method, str) else int(method)
        self._chk(self._L.jwas_hip_init_state(self._h, code, int(ntraits)))
        self.method, self.ntraits = code, int(ntraits)

    def _delta_dtype(self):
        return np.int32 if self.method == _lib.BAYESR else self.dtype

    def _f(self, name):
        """The entry point `name`, or its _f64 namesake in a Float64 context."""
        return getattr(self._L, name + "_f64" if self.precision == 64 else name)

    def set_state(self, trait=0, alpha=None, beta=None, delta=None):
        a = None if alpha is None else np.ascontiguousarray(alpha, dtype=self.dtype)
        b = None if beta is None else np.ascontiguousarray(beta, dtype=self.dtype)
        d = None if delta is None else np.ascontiguousarray(delta, dtype=self._delta_dtype())
        for v in (a, b, d):
            if v is not None and v.shape != (self.p,):
                raise ValueError(f"state vectors must have length {self.p}")
        self._chk(self._f("jwas_hip_set_state")(self._h, int(trait), _ptr(a), _ptr(b), _ptr(d)))

    def get_state(self, trait=0):
        a = np.empty(self.p, dtype=self.dtype)
        b = np.empty(self.p, dtype=self.dtype)
        d = np.empty(self.p, dtype=self._delta_dtype())
        self._chk(self._f("jwas_hip_get_state")(self._h, int(trait), _ptr(a), _ptr(b), _ptr(d)))
        return a, b, d

    def set_residual(self, r, trait=0):
        r = np.ascontiguousarray(r, dtype=self.dtype)
        if r.shape != (self.n,):
            raise ValueError(f"residual must have length {self.n}")
        self._chk(self._f("jwas_hip_set_residual")(self._h, int(trait), _ptr(r)))

    def get_residual(self, trait=0):
        r = np.empty(self.n, dtype=self.dtype)
        self._chk(self._f("jwas_hip_get_residual")(self._h, int(trait), _ptr(r)))
        return r

    def residual_dev(self):
        ptr, ld = C.c_void_p(), C.c_int64()
        self._chk(self._L.jwas_hip_residual_dev(self._h, C.byref(ptr), C.byref(ld)))
        return ptr.value, ld.value

    def residual_to_dev(self, dst_ptr, trait=0):
        self._chk(self._L.jwas_hip_residual_to_dev(self._h, int(trait), C.c_void_p(int(dst_ptr))))

    def residual_from_dev(self, src_ptr, trait=0):
        self._chk(self._L.jwas_hip_residual_from_dev(self._h, int(trait), C.c_void_p(int(src_ptr))))

    def residual_handover(self, src_engine):
        """This engine's resident residual := src_engine's (all traits, device to device, ordered by events on the two streams:
        jwas_hip_residual_handover) -- the one residual of a model with several genotype categories moving to the next category."""
        self._chk(self._L.jwas_hip_residual_handover(self._h, src_engine._h))

    def residual_add_scalar(self, shift, trait=0):
        """r_trait += shift on the device (the intercept's residual correction; no host copy of the residual)."""
        self._chk(self._L.jwas_hip_residual_add_scalar(self._h, int(trait), float(shift)))

    def last_sweep_counters(self):
        """The sampler's diagnostics counters of the last sweep (jwas_hip_last_sweep_counters)."""
        out = (C.c_uint64 * 32)()
        self._chk(self._L.jwas_hip_last_sweep_counters(self._h, out, 32))
        return [int(v) for v in out]

    def last_sweep_schedule(self, names=False):
        """Which schedule variant the last sweep ran (jwas_hip_last_sweep_schedule): the JWAS_HIP_SCHED_* mask, or with names=True
        a dict {name: bool} of _lib.SCHEDULE_FLAGS plus "COMPACT_OFF" (0..3)."""
        out = C.c_uint32(0)
        self._chk(self._L.jwas_hip_last_sweep_schedule(self._h, C.byref(out)))
        mask = int(out.value)
        if not names:
            return mask
        d = {k: bool(mask & bit) for k, bit in _lib.SCHEDULE_FLAGS.items()}
        d["COMPACT_OFF"] = (mask & _lib.SCHEDULE_COMPACT_OFF_MASK) >> _lib.SCHEDULE_COMPACT_OFF_SHIFT
        return d

    def set_kernel_timing(self, stride):
        self._chk(self._L.jwas_hip_set_kernel_timing(self._h, int(stride)))

    def sub_xalpha(self, trait=0):
        self._chk(self._L.jwas_hip_residual_sub_xalpha(self._h, int(trait)))

    def mul_alpha(self, trait=0):
        out = np.empty(self.n, dtype=self.dtype)
        self._chk(self._f("jwas_hip_mul_alpha")(self._h, int(trait), _ptr(out)))
        return out

    def alpha_sparse(self, trait=0):
        """(idx int32, val float32 | float64): the nonzero effects of a trait in marker order, compacted on the device."""
        cap = getattr(self, "_sparse_cap", 4096)
        while True:
            idx = np.empty(cap, dtype=np.int32)
            val = np.empty(cap, dtype=self.dtype)
            nnz = C.c_int64(0)
            rc = self._f("jwas_hip_get_alpha_sparse")(self._h, int(trait), cap, _ptr(idx), _ptr(val), C.byref(nnz))
            if rc == 0:
                return idx[:nnz.value].copy(), val[:nnz.value].copy()
            if nnz.value > cap:                      # grow and retry
                cap = self._sparse_cap = int(min(self.p, max(2 * cap, nnz.value)))
                continue
            self._chk(rc)

    def load_output_dense(self, X_out):
        """Rows EBVs are reported for when they differ from the training rows (Mi.output_genotypes,
        tools4genotypes.jl:290-296).  X_out: n_out x p float32 (float64 in a Float64 context)."""
        X_out = np.asarray(X_out)
        if X_out.dtype != self.dtype:
            raise TypeError(f"this engine stores {np.dtype(self.dtype).name} genotypes (double_precision={'true' if self.precision == 64 else 'false'})")
        if X_out.ndim != 2:
            raise ValueError("genotype matrix must be 2-D")
        if not X_out.flags.f_contiguous:
            X_out = np.asfortranarray(X_out)
        n_out, p = X_out.shape
        self._chk((self._L.jwas_hip_load_output_dense_f64 if self.precision == 64 else self._L.jwas_hip_load_output_dense_f32)(self._h, _ptr(X_out), n_out, p, n_out))
        self.n_out = n_out

    def window_sums(self, wptr, idx, val, use_output_rows=False):
        """(sum_i BV_w[i], sum_i BV_w[i]^2) for every window of one marker-effect sample (GWAS.jl:152-165); CSR-like
        description of the nonzero effects: window w = idx/val[wptr[w]:wptr[w+1]]."""
        wptr = np.ascontiguousarray(wptr, dtype=np.int32)
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        val = np.ascontiguousarray(val, dtype=self.dtype)
        nwin = wptr.size - 1
        s, q = np.empty(nwin), np.empty(nwin)
        self._chk(self._f("jwas_hip_window_sums")(self._h, 1 if use_output_rows else 0, nwin, _ptr(wptr), _ptr(idx), _ptr(val), _ptr(s), _ptr(q)))
        return s, q

    def window_sums2(self, wptr, idx, val1, val2, use_output_rows=False):
        """Two effect vectors over the same markers: (sum1, ss1, sum2, ss2, cross) per window (GWAS.jl:199-217)."""
        wptr = np.ascontiguousarray(wptr, dtype=np.int32)
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        v1 = np.ascontiguousarray(val1, dtype=self.dtype)
        v2 = np.ascontiguousarray(val2, dtype=self.dtype)
        nwin = wptr.size - 1
        outs = [np.empty(nwin) for _ in range(5)]
        self._chk(self._f("jwas_hip_window_sums2")(self._h, 1 if use_output_rows else 0, nwin, _ptr(wptr), _ptr(idx), _ptr(v1), _ptr(v2),
                                                *[_ptr(o) for o in outs]))
        return tuple(outs)

    # -- GWAS session (jwas_hip_gwas_*; GWAS.jl:149-173) -------------------------------------------
    @staticmethod
    def gwas_estimate_bytes(n_rows, nwin, max_nnz, local_ebv=False):
        """Device bytes of a session: rows padded to 256; local_ebv adds 8 * padded_rows * nwin."""
        return _lib.load().jwas_hip_gwas_estimate_bytes(int(n_rows), int(nwin), int(max_nnz), 1 if local_ebv else 0)

    def gwas_begin(self, col_start, col_end, local_ebv=False, use_output_rows=False):
        """Open a session over the windows [col_start[w], col_end[w]) (gwas.build_windows); everything stays resident until
        gwas_end.  local_ebv: keep the n_rows x nwin accumulator of the windows' genomic values (GWAS.jl:159-164)."""
        cs = np.ascontiguousarray(col_start, dtype=np.int32)
        ce = np.ascontiguousarray(col_end, dtype=np.int32)
        if cs.shape != ce.shape or cs.ndim != 1:
            raise ValueError("col_start and col_end must be vectors of one length")
        self._chk(self._L.jwas_hip_gwas_begin(self._h, 1 if use_output_rows else 0, cs.size, _ptr(cs), _ptr(ce), 1 if local_ebv else 0))
        self._gwas_nwin = cs.size
        self._gwas_rows = getattr(self, "n_out", 0) if use_output_rows else self.n

    def gwas_sample(self, idx, val):
        """One saved sample as the ascending (idx, val) list of its nonzero effects -> (sum, ss), nwin + 1 entries each:
        entry 0 = all markers, entry 1 + w = window w (the bits of window_sums)."""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        val = np.ascontiguousarray(val, dtype=self.dtype)
        if idx.shape != val.shape or idx.ndim != 1:
            raise ValueError("idx and val must be vectors of one length")
        nent = getattr(self, "_gwas_nwin", 0) + 1
        s, q = np.empty(nent), np.empty(nent)
        self._chk(self._f("jwas_hip_gwas_sample")(self._h, idx.size, _ptr(idx), _ptr(val), _ptr(s), _ptr(q)))
        return s, q

    def gwas_local_ebv(self):
        """(n_rows x nwin Float64 mean of the windows' genomic values over the samples folded so far, number of samples)."""
        nwin, rows = getattr(self, "_gwas_nwin", 0), getattr(self, "_gwas_rows", 0)
        out = np.empty((max(nwin, 1), max(rows, 1)))
        ns = C.c_int64(0)
        self._chk(self._L.jwas_hip_gwas_local_ebv(self._h, _ptr(out), C.byref(ns)))
        return out[:nwin, :rows].T, ns.value

    def gwas_geometry(self):
        """Launch geometry of the session's partial kernel: grid = nslices x nchunks, windows_per_chunk windows per chunk."""
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        self._chk(self._L.jwas_hip_gwas_geometry(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"nslices": a.value, "windows_per_chunk": b.value, "nchunks": c.value}

    def gwas_end(self):
        self._chk(self._L.jwas_hip_gwas_end(self._h))
        self._gwas_nwin = self._gwas_rows = 0

    # -- threshold / censored traits (jwas_hip_liability_*; categorical_and_censored_trait.jl) -----------
    def liability_begin(self, ntraits=None):
        """Start the liability state for the traits of init_state: every trait continuous until set_categorical / set_censored."""
        nt = self.ntraits if ntraits is None else int(ntraits)
        self._chk(self._L.jwas_hip_liability_begin(self._h, nt))
        self._liab_nthr = {}

    def set_categorical(self, trait, codes, thresholds):
        """codes: category per record, 1..ncat (0 = missing); thresholds: [-Inf, t1, ..., +Inf].  The liabilities become the
        codes (the placeholder phenotype)."""
        cd = np.ascontiguousarray(codes, dtype=np.int32)
        th = np.ascontiguousarray(thresholds, dtype=np.float64)
        if cd.ndim != 1 or th.ndim != 1:
            raise ValueError("codes and thresholds must be vectors")
        self._chk(self._L.jwas_hip_liability_set_categorical(self._h, int(trait), cd.size, _ptr(cd), th.size, _ptr(th)))
        self._liab_nthr[int(trait)] = th.size

    def set_censored(self, trait, lower, upper):
        """Bounds per record (+-Inf allowed; lower == upper: an exact record)."""
        lo = np.ascontiguousarray(lower, dtype=np.float64)
        up = np.ascontiguousarray(upper, dtype=np.float64)
        if lo.shape != up.shape or lo.ndim != 1:
            raise ValueError("lower and upper must be vectors of one length")
        self._chk(self._L.jwas_hip_liability_set_censored(self._h, int(trait), lo.size, _ptr(lo), _ptr(up)))

    def set_thresholds(self, trait, thresholds):
        th = np.ascontiguousarray(thresholds, dtype=np.float64)
        self._chk(self._L.jwas_hip_liability_set_thresholds(self._h, int(trait), th.size, _ptr(th)))

    @staticmethod
    def _liability_params(iteration, seed, ngibbs, R):
        P = _lib.LiabilityParams()
        P.iteration, P.ngibbs, P.seed = int(iteration), int(ngibbs), int(seed)
        Rm = np.atleast_2d(np.asarray(R, dtype=np.float64))
        if Rm.shape[0] != Rm.shape[1] or Rm.shape[0] > _lib.MAX_TRAITS:
            raise ValueError("R must be a t x t matrix, t <= 4")
        for i, v in enumerate(Rm.ravel()):
            P.R[i] = float(v)
        return P

    def liability_init(self, *, seed, R):
        """The set-up draw (iteration 0): liability ~ N(cmean, R_kk) truncated to the record's bounds, cmean = liability - residual."""
        P = self._liability_params(0, seed, 1, R)
        self._chk(self._L.jwas_hip_liability_init(self._h, C.byref(P)))

    def liability_sample(self, *, iteration, seed, ngibbs, R):
        """sample_liabilities!: redraw liabilities and residuals of the categorical / censored traits on the device."""
        P = self._liability_params(iteration, seed, ngibbs, R)
        self._chk(self._L.jwas_hip_liability_sample(self._h, C.byref(P)))

    def liability_minmax(self, trait):
        """(max_below, min_above) per threshold of a categorical trait: the support of the threshold draw."""
        nthr = getattr(self, "_liab_nthr", {}).get(int(trait), _lib.MAX_THRESHOLDS)
        a, b = np.empty(_lib.MAX_THRESHOLDS), np.empty(_lib.MAX_THRESHOLDS)
        self._chk(self._L.jwas_hip_liability_minmax(self._h, int(trait), _ptr(a), _ptr(b)))
        return a[:nthr].copy(), b[:nthr].copy()

    def liabilities(self, trait):
        out = np.empty(self.n, dtype=np.float64)
        self._chk(self._L.jwas_hip_get_liabilities(self._h, int(trait), _ptr(out)))
        return out

    def liability_end(self):
        self._chk(self._L.jwas_hip_liability_end(self._h))
        self._liab_nthr = {}

    # -- location parameters (jwas_hip_locpar_*; MCMC_BayesianAlphabet.jl:193-220, solver.jl:143-162) ------
    @staticmethod
    def locpar_estimate_bytes(n, nterms, total_levels):
        return _lib.load().jwas_hip_locpar_estimate_bytes(int(n), int(nterms), int(total_levels))

    def locpar_begin(self, ntraits=None):
        """Start the location-parameter state for the traits of init_state: no terms.  The residual weights are those in force now."""
        nt = self.ntraits if ntraits is None else int(ntraits)
        self._chk(self._L.jwas_hip_locpar_begin(self._h, nt))
        self._locpar_groups = {}
        self._locpar_struct_levels = {}

    def locpar_add_covariate(self, trait, x=None):
        """A one-entry term of `trait`: the covariate x, or the intercept (x = None).  Terms are sampled in the order added."""
        if x is None:
            self._chk(self._L.jwas_hip_locpar_add_covariate(self._h, int(trait), self.n, None))
            return
        xv = np.ascontiguousarray(x, dtype=np.float64)
        if xv.ndim != 1:
            raise ValueError("x must be a vector")
        self._chk(self._L.jwas_hip_locpar_add_covariate(self._h, int(trait), xv.size, _ptr(xv)))

    def locpar_add_factor(self, trait, level, nlevels, random_group=-1):
        """A class factor: level[i] in 0..nlevels-1 or -1 (in no level); random_group -1 = fixed, g >= 0 = member of random effect g."""
        lv = np.ascontiguousarray(level, dtype=np.int32)
        if lv.ndim != 1:
            raise ValueError("level must be a vector")
        self._chk(self._L.jwas_hip_locpar_add_factor(self._h, int(trait), lv.size, _ptr(lv), int(nlevels), int(random_group)))
        if random_group >= 0:
            self._locpar_groups[int(random_group)] = self._locpar_groups.get(int(random_group), 0) + 1

    @staticmethod
    def locpar_structure_estimate_bytes(nlevels, nnz):
        return _lib.load().jwas_hip_lp_structure_estimate_bytes(int(nlevels), int(nnz))

    def locpar_set_group_structure(self, random_group, indptr, indices, values):
        """Give random effect `random_group` the inverse covariance among its levels: a full symmetric CSR matrix (len(indptr) - 1
        levels, ascending columns).  After locpar_begin, before the effect's first member term.  The library colours its graph and
        samples a member term colour by colour (csrc/locpar.hpp); locpar_step's utu of the effect is then U' V U."""
        ip = np.ascontiguousarray(indptr, dtype=np.int64)
        ix = np.ascontiguousarray(indices, dtype=np.int32)
        vv = np.ascontiguousarray(values, dtype=np.float64)
        if ip.ndim != 1 or ip.size < 1 or ix.ndim != 1 or vv.shape != ix.shape or (ip.size and ip[-1] != ix.size):
            raise ValueError("indptr, indices and values must describe one CSR matrix")
        self._chk(self._L.jwas_hip_lp_set_group_structure(self._h, int(random_group), ip.size - 1, _ptr(ip), _ptr(ix), _ptr(vv)))
        if not hasattr(self, "_locpar_struct_levels"):
            self._locpar_struct_levels = {}
        self._locpar_struct_levels[int(random_group)] = ip.size - 1

    def locpar_group_colors(self, random_group):
        """The colour of every level of the structure of `random_group`: the order the device visits them in."""
        nlev = getattr(self, "_locpar_struct_levels", {}).get(int(random_group), 0)
        out, nc = np.empty(max(nlev, 1), dtype=np.int32), C.c_int32()
        self._chk(self._L.jwas_hip_lp_get_group_colors(self._h, int(random_group), nlev, _ptr(out), C.byref(nc)))
        return out[:nlev].copy()

    def locpar_size(self):
        q = C.c_int64()
        self._chk(self._L.jwas_hip_locpar_size(self._h, C.byref(q)))
        return q.value

    def locpar_set_sol(self, sol):
        sv = np.ascontiguousarray(sol, dtype=np.float64)
        self._chk(self._L.jwas_hip_locpar_set_sol(self._h, sv.size, _ptr(sv)))

    def locpar_get_sol(self):
        out = np.empty(self.locpar_size(), dtype=np.float64)
        self._chk(self._L.jwas_hip_locpar_get_sol(self._h, out.size, _ptr(out)))
        return out

    def locpar_step(self, *, iteration, seed, vare=None, Rinv=None, Gi=(), first_term=0, last_term=-1):
        """One scan over the terms first_term .. last_term - 1.  vare: the residual variance (one trait); Rinv: inv(R) (several
        traits); Gi: inv(G) of every random effect, in group order.  Returns {"utu": [U'U per random effect], "step_ms"}."""
        P, S = _lib.LocparParams(), _lib.LocparStats()
        P.iteration, P.seed, P.first_term, P.last_term = int(iteration), int(seed), int(first_term), int(last_term)
        P.vare = 0.0 if vare is None else float(vare)
        if Rinv is not None:
            for i, v in enumerate(np.atleast_2d(np.asarray(Rinv, dtype=np.float64)).ravel()):
                P.Rinv[i] = float(v)
        groups = getattr(self, "_locpar_groups", {})
        if len(Gi) != len(groups):
            raise ValueError(f"Gi must hold one matrix per random effect ({len(groups)}, got {len(Gi)})")
        for g, M in enumerate(Gi):
            M = np.atleast_2d(np.asarray(M, dtype=np.float64))
            if M.shape != (groups.get(g, 0),) * 2:
                raise ValueError(f"Gi[{g}] must be {groups.get(g, 0)} x {groups.get(g, 0)}")
            for i, v in enumerate(M.ravel()):
                P.Gi[16 * g + i] = float(v)
        self._chk(self._L.jwas_hip_locpar_step(self._h, C.byref(P), C.byref(S)))
        utu = [np.array(S.utu[16 * g:16 * g + k * k]).reshape(k, k) for g, k in sorted(groups.items())]
        return {"utu": utu, "step_ms": S.step_ms}

    def locpar_accumulate(self, nsamples):
        self._chk(self._L.jwas_hip_locpar_accumulate(self._h, float(nsamples)))

    def locpar_get_means(self):
        """(mean, mean of squares) of sol over the accumulated samples."""
        m, m2 = np.empty(self.locpar_size(), dtype=np.float64), np.empty(self.locpar_size(), dtype=np.float64)
        self._chk(self._L.jwas_hip_locpar_get_means(self._h, m.size, _ptr(m), _ptr(m2)))
        return m, m2

    def locpar_end(self):
        self._chk(self._L.jwas_hip_locpar_end(self._h))
        self._locpar_groups = {}

    # -- multi-trait records that miss some traits (jwas_hip_mtmiss_*; residual.jl:2-73) ----------------------
    @staticmethod
    def mtmiss_estimate_bytes(n):
        return _lib.load().jwas_hip_mtmiss_estimate_bytes(int(n))

    def _mtmiss_table(self, tab, what):
        t = self.ntraits
        tv = np.ascontiguousarray(tab, dtype=np.float64)
        if tv.shape != (1 << t, t, t):
            raise ValueError(f"{what} must be a [2^t][t][t] table ({(1 << t, t, t)}, got {tv.shape})")
        return tv

    def mtmiss_begin(self, observed):
        """observed: the code of every record (bit k set = trait k observed, 1 .. 2^t - 1), or an n x t boolean matrix.  After
        init_state."""
        ob = np.asarray(observed)
        if ob.ndim == 2:
            ob = ob.astype(np.int64) @ (1 << np.arange(ob.shape[1]))
        cd = np.ascontiguousarray(ob, dtype=np.int32)
        if cd.ndim != 1:
            raise ValueError("observed must be a vector of codes or an n x t matrix")
        self._chk(self._L.jwas_hip_mtmiss_begin(self._h, cd.size, _ptr(cd)))

    def mtmiss_impute(self, *, iteration, seed, B, U):
        """sampleMissingResiduals on the device: the residuals of the missing cells are redrawn from their conditional given the
        observed ones.  B, U: the per-code tables [2^t][t][t] of the current R (csrc/mtmiss.hpp)."""
        Bv, Uv = self._mtmiss_table(B, "B"), self._mtmiss_table(U, "U")
        P = _lib.MtmissParams()
        P.iteration, P.seed, P.B, P.U = int(iteration), int(seed), Bv.ctypes.data, Uv.ctypes.data
        self._chk(self._L.jwas_hip_mtmiss_impute(self._h, C.byref(P)))

    def mtmiss_set_record_weights(self, Ctab):
        """Ctab [2^t][t][t]: every later locpar_step weights record i with Ctab[code_i] (its Rinv is ignored); None: back to
        kron(inv(R), diag(w))."""
        if Ctab is None:
            self._chk(self._L.jwas_hip_mtmiss_set_record_weights(self._h, None))
            return
        Cv = self._mtmiss_table(Ctab, "C")
        self._chk(self._L.jwas_hip_mtmiss_set_record_weights(self._h, _ptr(Cv)))

    def mtmiss_end(self):
        self._chk(self._L.jwas_hip_mtmiss_end(self._h))

    # -- marker-annotation priors (jwas_hip_annot_*; MCMC/annotation_updates.jl, csrc/annot.hpp) ----------------
    ANNOT_KINDS = {"BayesC": _lib.ANNOT_BAYESC, "BayesR": _lib.ANNOT_BAYESR, "tree": _lib.ANNOT_TREE}

    @staticmethod
    def annot_estimate_bytes(p, ncols, kind):
        return _lib.load().jwas_hip_annot_estimate_bytes(int(p), int(ncols), HipEngine.ANNOT_KINDS[kind])

    def annot_begin(self, kind, design_matrix, coefficients, variance, start_prior):
        """Open an annotation session.  kind: "BayesC" (1 step), "BayesR" or "tree" (3 steps; the 2-trait model).  design_matrix:
        p x ncols with the intercept's ones in column 0; coefficients: ncols, or ncols x 3 (the layout of MarkerAnnotations);
        variance: scalar or 3; start_prior: the table the first sweep reads (p, p x 4, or the p x 4 logs of the tree)."""
        code = self.ANNOT_KINDS[kind]
        ns = 1 if code == _lib.ANNOT_BAYESC else 3
        Dm = np.ascontiguousarray(design_matrix, dtype=np.float64)
        if Dm.ndim != 2:
            raise ValueError("design_matrix must be p x ncols")
        cf = np.asarray(coefficients, dtype=np.float64)
        cf = np.ascontiguousarray(cf.reshape(Dm.shape[1], ns).T)      # -> [nsteps][ncols]
        vr = np.ascontiguousarray(np.broadcast_to(np.asarray(variance, dtype=np.float64), (ns,)))
        sp = np.ascontiguousarray(start_prior, dtype=np.float64)
        if sp.size != Dm.shape[0] * (1 if ns == 1 else 4):
            raise ValueError("start_prior must hold one row of the prior table per marker")
        self._chk(self._L.jwas_hip_annot_begin(self._h, code, Dm.shape[0], Dm.shape[1], _ptr(Dm), _ptr(cf), _ptr(vr), _ptr(sp)))
        self._annot = (code, ns, Dm.shape[1])

    def annot_step(self, *, iteration, seed, variance):
        """One probit update from the resident delta; the prior table is left where the next sweep(resident_priors=True) reads it.
        Returns {"coefficients": ncols (BayesC) or ncols x 3, "n_active": per step, "means": column means of the table (BayesC: one
        value), "step_ms"}."""
        code, ns, K = self._annot
        P, S = _lib.AnnotParams(), _lib.AnnotStats()
        P.iteration, P.seed = int(iteration), int(seed)
        for s, v in enumerate(np.broadcast_to(np.asarray(variance, dtype=np.float64), (ns,))):
            P.variance[s] = float(v)
        self._chk(self._L.jwas_hip_annot_step(self._h, C.byref(P), C.byref(S)))
        cf = np.array(S.coef[:ns * K]).reshape(ns, K)
        return {"coefficients": cf[0].copy() if ns == 1 else np.ascontiguousarray(cf.T), "n_active": np.array(S.n_active[:ns]),
                "means": np.array(S.means[:1 if ns == 1 else 4]), "step_ms": S.step_ms}

    def annot_accumulate(self, nsamples):
        self._chk(self._L.jwas_hip_annot_accumulate(self._h, float(nsamples)))

    def _annot_table_shape(self):
        return (self.p,) if self._annot[1] == 1 else (self.p, 4)

    def annot_prior(self):
        """The resident prior table as the sweep reads it: p (BayesC), p x 4 (BayesR), the p x 4 logs (tree)."""
        out = np.empty(self._annot_table_shape(), dtype=np.float64)
        self._chk(self._L.jwas_hip_annot_get_prior(self._h, out.size, _ptr(out)))
        return out

    def annot_means(self):
        """(mean, mean of squares) of the per-marker prior probabilities over the accumulated samples."""
        m, m2 = np.empty(self._annot_table_shape(), dtype=np.float64), np.empty(self._annot_table_shape(), dtype=np.float64)
        self._chk(self._L.jwas_hip_annot_get_means(self._h, m.size, _ptr(m), _ptr(m2)))
        return m, m2

    def _annot_steps(self, fn):
        out = np.empty((self._annot[1], self.p), dtype=np.float64)
        self._chk(fn(self._h, out.size, _ptr(out)))
        return out[0].copy() if self._annot[1] == 1 else np.ascontiguousarray(out.T)

    def annot_liability(self):
        """The liabilities: p (BayesC) or p x 3."""
        return self._annot_steps(self._L.jwas_hip_annot_get_liability)

    def annot_mu(self):
        return self._annot_steps(self._L.jwas_hip_annot_get_mu)

    def annot_end(self):
        self._chk(self._L.jwas_hip_annot_end(self._h))
        self._annot = None

    # -- structural equation models (jwas_hip_sem_*; structure_equation_model/SEM.jl, csrc/sem.hpp) ----------------
    @staticmethod
    def sem_estimate_bytes(n, p, ntraits):
        return _lib.load().jwas_hip_sem_estimate_bytes(int(n), int(p), int(ntraits))

    def sem_begin(self, y, structure):
        """Open a session.  y: the t x n phenotypes (constant); structure: the t x t strictly lower 0/1 causal structure
        (structure[i, j] = 1: trait j acts on trait i).  After init_state and set_residual; the coefficients start at 0."""
        yv = np.ascontiguousarray(y, dtype=np.float64)
        cs = np.asarray(structure)
        if yv.ndim != 2 or cs.shape != (yv.shape[0], yv.shape[0]):
            raise ValueError("y must be t x n and structure t x t")
        if not np.all(np.isfinite(cs) & (cs == np.round(cs))):
            raise ValueError("structure must hold 0 / 1")
        cv = np.ascontiguousarray(cs, dtype=np.int32)
        self._chk(self._L.jwas_hip_sem_begin(self._h, yv.shape[0], yv.shape[1], _ptr(yv), _ptr(cv)))
        self._sem_t = yv.shape[0]

    def sem_step(self, *, iteration, seed, R_diag):
        """One draw of every structural coefficient from the resident residual, which is updated in place.  Returns {"lambda",
        "mean" (of the full conditional), "ypr" ([i, j] = y_j'r_i before the step): t x t, "step_ms"}."""
        t = self._sem_t
        P, S = _lib.SemParams(), _lib.SemStats()
        P.iteration, P.seed = int(iteration), int(seed)
        rd = np.asarray(R_diag, dtype=np.float64).reshape(-1)
        if rd.size != t:
            raise ValueError(f"R_diag must hold one value per trait ({t})")
        for k in range(t):
            P.R_diag[k] = float(rd[k])
        self._chk(self._L.jwas_hip_sem_step(self._h, C.byref(P), C.byref(S)))
        return {"lambda": np.array(S.lambda_[:t * t]).reshape(t, t), "mean": np.array(S.mean[:t * t]).reshape(t, t),
                "ypr": np.array(S.ypr[:t * t]).reshape(t, t), "step_ms": S.step_ms}

    def _sem_matrix(self, fn):
        out = np.empty((self._sem_t, self._sem_t), dtype=np.float64)
        self._chk(fn(self._h, _ptr(out)))
        return out

    def sem_get_lambda(self):
        return self._sem_matrix(self._L.jwas_hip_sem_get_lambda)

    def sem_set_lambda(self, lam):
        """The state only: the residual is not touched."""
        lv = np.ascontiguousarray(lam, dtype=np.float64)
        if lv.shape != (self._sem_t, self._sem_t):
            raise ValueError("lambda must be t x t")
        self._chk(self._L.jwas_hip_sem_set_lambda(self._h, _ptr(lv)))

    def sem_get_gram(self):
        """S = y y' as the step reads it."""
        return self._sem_matrix(self._L.jwas_hip_sem_get_gram)

    def sem_accumulate(self, K, nsamples):
        """Running means of the indirect (K alpha) and overall (alpha + K alpha) marker effects; K = sum_m Lambda^m, t x t."""
        Kv = np.ascontiguousarray(K, dtype=np.float64)
        if Kv.shape != (self._sem_t, self._sem_t):
            raise ValueError("K must be t x t")
        self._chk(self._L.jwas_hip_sem_accumulate(self._h, _ptr(Kv), float(nsamples)))

    def sem_get_effects(self, kind, trait):
        """(mean, mean of squares, frequency of non-zero) per marker; kind: "indirect" or "overall"."""
        code = {"indirect": 0, "overall": 1}[kind]
        out = [np.empty(self.p, dtype=np.float64) for _ in range(3)]
        self._chk(self._L.jwas_hip_sem_get_effects(self._h, code, int(trait), _ptr(out[0]), _ptr(out[1]), _ptr(out[2])))
        return tuple(out)

    def sem_end(self):
        self._chk(self._L.jwas_hip_sem_end(self._h))
        self._sem_t = None

    # -- random regression models (jwas_hip_rrm_*; RRM/RRM.jl, RRM/MCMC_BayesianAlphabet_RRM.jl, csrc/rrm.hpp) ----------------
    @staticmethod
    def rrm_estimate_bytes(n, p, ntimes, ncoeff, block_size=64):
        return _lib.load().jwas_hip_rrm_estimate_bytes(int(n), int(p), int(ntimes), int(ncoeff), int(block_size))

    def rrm_begin(self, Phi, observed, block_size=64):
        """Open a session on the loaded genotypes.  Phi: T x c; observed: T x n booleans (True: the individual has a record at that
        time point).  Builds M_j and the block Gram tensor; the residual starts at 0, alpha and beta at 0, delta at 1."""
        ph = np.ascontiguousarray(Phi, dtype=np.float64)
        ob = np.asarray(observed)
        if ph.ndim != 2 or ob.ndim != 2 or ob.shape[0] != ph.shape[0]:
            raise ValueError("Phi must be T x c and observed T x n")
        T, c = ph.shape
        mask = np.zeros(ob.shape[1], dtype=np.uint64)
        for t in range(min(T, 64)):
            mask |= ob[t].astype(bool).astype(np.uint64) << np.uint64(t)
        self._chk(self._L.jwas_hip_rrm_begin(self._h, T, c, ob.shape[1], _ptr(ph), _ptr(mask), int(block_size)))
        self._rrm = (T, c, int(block_size) if block_size else 64)

    def rrm_set_residual(self, W):
        """W: T x n doubles; the cells without a record are forced to 0."""
        T, c, _ = self._rrm
        Wv = np.ascontiguousarray(W, dtype=np.float64)
        if Wv.shape != (T, self.n):
            raise ValueError(f"the residual must be {T} x {self.n}")
        self._chk(self._L.jwas_hip_rrm_set_residual(self._h, Wv.size, _ptr(Wv)))

    def rrm_get_residual(self):
        T, c, _ = self._rrm
        out = np.empty((T, self.n), dtype=np.float64)
        self._chk(self._L.jwas_hip_rrm_get_residual(self._h, out.size, _ptr(out)))
        return out

    def rrm_set_state(self, alpha=None, beta=None, delta=None):
        """alpha, beta, delta: c x p doubles each, any may be None.  The state only: the residual is not touched."""
        T, c, _ = self._rrm
        arrs = []
        for a in (alpha, beta, delta):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.float64)
                if a.shape != (c, self.p):
                    raise ValueError(f"state arrays must be {c} x {self.p}")
            arrs.append(a)
        self._chk(self._L.jwas_hip_rrm_set_state(self._h, _ptr(arrs[0]), _ptr(arrs[1]), _ptr(arrs[2])))

    def rrm_get_state(self):
        T, c, _ = self._rrm
        out = [np.empty((c, self.p), dtype=np.float64) for _ in range(3)]
        self._chk(self._L.jwas_hip_rrm_get_state(self._h, _ptr(out[0]), _ptr(out[1]), _ptr(out[2])))
        return tuple(out)

    def rrm_sweep(self, *, iteration, seed, vare, G, log_pi):
        """One sweep over all markers.  G: c x c; log_pi: 2^c values, state index bit q = coefficient q.  Returns {"state_counts",
        "beta_ss" (c x c), "alpha_ss", "resid_ss", "n_changed", "step_ms"}."""
        T, c, _ = self._rrm
        P, S = _lib.RrmParams(), _lib.RrmStats()
        P.iteration, P.seed, P.vare = int(iteration), int(seed), float(vare)
        Gv = np.asarray(G, dtype=np.float64)
        lp = np.asarray(log_pi, dtype=np.float64).reshape(-1)
        if Gv.shape != (c, c) or lp.size != 1 << c:
            raise ValueError(f"G must be {c} x {c} and log_pi hold {1 << c} values")
        for i, v in enumerate(Gv.ravel()):
            P.G[i] = float(v)
        for i, v in enumerate(lp):
            P.log_pi[i] = float(v)
        self._chk(self._L.jwas_hip_rrm_sweep(self._h, C.byref(P), C.byref(S)))
        return {"state_counts": np.array(S.state_counts[:1 << c]), "beta_ss": np.array(S.beta_ss[:c * c]).reshape(c, c), "alpha_ss": S.alpha_ss,
                "resid_ss": S.resid_ss, "n_changed": S.n_changed, "step_ms": S.step_ms}

    def rrm_accumulate(self, nsamples):
        self._chk(self._L.jwas_hip_rrm_accumulate(self._h, float(nsamples)))

    def rrm_posterior(self, q):
        """(mean, mean of squares, model frequency) of coefficient q, p values each."""
        out = [np.empty(self.p, dtype=np.float64) for _ in range(3)]
        self._chk(self._L.jwas_hip_rrm_get_posterior(self._h, int(q), _ptr(out[0]), _ptr(out[1]), _ptr(out[2])))
        return tuple(out)

    def rrm_mul_alpha(self, q):
        out = np.empty(self.n, dtype=np.float64)
        self._chk(self._L.jwas_hip_rrm_mul_alpha(self._h, int(q), _ptr(out)))
        return out

    @staticmethod
    def _rrm_full(cells, c):
        """lower cells (a (a + 1) / 2 + b) on the last axis -> symmetric c x c"""
        out = np.empty(cells.shape[:-1] + (c, c), dtype=np.float64)
        for a in range(c):
            for b in range(a + 1):
                out[..., a, b] = out[..., b, a] = cells[..., a * (a + 1) // 2 + b]
        return out

    def rrm_m(self):
        """M_j as p x c x c."""
        T, c, _ = self._rrm
        out = np.empty((self.p, c * (c + 1) // 2), dtype=np.float64)
        self._chk(self._L.jwas_hip_rrm_get_m(self._h, out.size, _ptr(out)))
        return self._rrm_full(out, c)

    def rrm_gram(self, block):
        """The Gram tensor of one block as b x b x c x c: [j, k] = sum_i x_ij x_ik O_i."""
        T, c, bs = self._rrm
        b = min(bs, self.p - int(block) * bs)
        out = np.empty((max(b, 0), max(b, 0), c * (c + 1) // 2), dtype=np.float64)
        self._chk(self._L.jwas_hip_rrm_get_gram(self._h, int(block), out.size, _ptr(out)))
        return self._rrm_full(out, c)

    def rrm_end(self):
        self._chk(self._L.jwas_hip_rrm_end(self._h))
        self._rrm = None

    # -- what the mega-trait and the joint multi-trait session share: one body per twin entry point.  kind: "mega" or "mtj" -- the
    # symbol is jwas_hip_<kind>_<name>, and self._mega or self._mtj holds (T, block size) --------------------------------------------
    def _blk(self, kind, name):
        return (getattr(self._L, f"jwas_hip_{kind}_{name}"),) + getattr(self, "_" + kind)

    def _blk_set_residual(self, kind, R, trait=None, one_trait=""):
        fn, T, _ = self._blk(kind, "set_residual")
        Rv = np.ascontiguousarray(R, dtype=np.float64)
        if Rv.shape != ((T, self.n) if trait is None else (self.n,)):
            raise ValueError(f"the residual must be {T} x {self.n}{one_trait}")
        for k in (range(T) if trait is None else [int(trait)]):
            self._chk(fn(self._h, k, _ptr(Rv[k] if trait is None else Rv)))

    def _blk_get_residual(self, kind, trait=None):
        fn, T, _ = self._blk(kind, "get_residual")
        out = np.empty((T, self.n) if trait is None else (1, self.n), dtype=np.float64)
        for i, k in enumerate(range(T) if trait is None else [int(trait)]):
            self._chk(fn(self._h, k, _ptr(out[i])))
        return out if trait is None else out[0]

    def _blk_set_state(self, kind, alpha, beta, delta):
        fn, T, _ = self._blk(kind, "set_state")
        arrs = []
        for a in (alpha, beta, delta):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.float64)
                if a.shape != (T, self.p):
                    raise ValueError(f"state arrays must be {T} x {self.p}")
            arrs.append(a)
        for k in range(T):
            self._chk(fn(self._h, k, *[_ptr(a[k]) if a is not None else None for a in arrs]))

    def _blk_get_state(self, kind, trait=None):
        fn, T, _ = self._blk(kind, "get_state")
        ks = range(T) if trait is None else [int(trait)]
        out = [np.empty((len(ks), self.p), dtype=np.float64) for _ in range(3)]
        for i, k in enumerate(ks):
            self._chk(fn(self._h, k, _ptr(out[0][i]), _ptr(out[1][i]), _ptr(out[2][i])))
        return tuple(out) if trait is None else tuple(o[0] for o in out)

    def _blk_gram(self, kind, name, block):
        fn, T, bs = self._blk(kind, name)
        b = max(min(bs, self.p - int(block) * bs), 0)
        G, xpx = np.empty((b, b), dtype=np.float64), np.empty(b, dtype=np.float64)
        self._chk(fn(self._h, int(block), G.size, _ptr(G), _ptr(xpx)))
        return G, xpx

    def _blk_posterior(self, fn, trait):
        out = [np.empty(self.p, dtype=np.float64) for _ in range(3)]
        self._chk(fn(self._h, int(trait), _ptr(out[0]), _ptr(out[1]), _ptr(out[2])))
        return tuple(out)

    def _blk_mul_alpha(self, fn, trait, output_rows):
        out = np.empty(getattr(self, "n_out", 0) if output_rows else self.n, dtype=np.float64)
        self._chk(fn(self._h, int(trait), 1 if output_rows else 0, _ptr(out)))
        return out

    def _blk_end(self, kind):
        self._chk(getattr(self._L, f"jwas_hip_{kind}_end")(self._h))
        setattr(self, "_" + kind, None)

    # -- mega-trait models (jwas_hip_mega_*; markers/BayesianAlphabet/BayesABC.jl:1-58, csrc/mega.hpp) ------------------------
    @staticmethod
    def mega_estimate_bytes(n, p, ntraits, block_size=64):
        return _lib.load().jwas_hip_mega_estimate_bytes(int(n), int(p), int(ntraits), int(block_size))

    def mega_begin(self, ntraits, block_size=64, first_trait=0):
        """Open a session of `ntraits` independent single-trait chains on the loaded genotypes: x'x and the block Grams; the
        residuals, alpha and beta start at 0, delta at 1.  first_trait: the RNG trait id of trait 0."""
        self._chk(self._L.jwas_hip_mega_begin(self._h, int(ntraits), int(block_size), int(first_trait)))
        self._mega = (int(ntraits), int(block_size) if block_size else 64)

    def mega_set_missing(self, missing):
        """missing: T x n booleans, True where the record misses the trait (None: complete records)."""
        T, _ = self._mega
        if missing is None:
            self._chk(self._L.jwas_hip_mega_set_missing(self._h, 0, None))
            return
        m = np.ascontiguousarray(np.asarray(missing).astype(bool), dtype=np.uint8)
        if m.shape != (T, self.n):
            raise ValueError(f"the missing pattern must be {T} x {self.n}")
        self._chk(self._L.jwas_hip_mega_set_missing(self._h, m.size, _ptr(m)))

    def mega_set_residual(self, R, trait=None):
        """R: T x n doubles (trait=None), or the n values of one trait."""
        self._blk_set_residual("mega", R, trait, f", or {self.n} values for one trait")

    def mega_get_residual(self, trait=None):
        return self._blk_get_residual("mega", trait)

    def mega_set_state(self, alpha=None, beta=None, delta=None):
        """alpha, beta, delta: T x p doubles each, any may be None.  The state only: the residuals are not touched."""
        self._blk_set_state("mega", alpha, beta, delta)

    def mega_get_state(self, trait=None):
        return self._blk_get_state("mega", trait)

    def _mega_params(self, iteration, seed, vare, var_effect=None, pi=None):
        T, _ = self._mega
        P = _lib.MegaParams()
        P.iteration, P.seed = int(iteration), int(seed)
        keep = []
        for name, v in (("vare", vare), ("var_effect", var_effect), ("pi", pi)):
            if v is None:
                continue
            a = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
            if a.size != T:
                raise ValueError(f"{name} must hold one value per trait ({T})")
            keep.append(a)
            setattr(P, name, a.ctypes.data)
        return P, keep

    def mega_impute(self, *, iteration, seed, vare):
        """Every missing cell redrawn from N(0, vare_k)."""
        P, keep = self._mega_params(iteration, seed, vare)
        self._chk(self._L.jwas_hip_mega_impute(self._h, C.byref(P)))

    def mega_sweep(self, *, iteration, seed, vare, var_effect, pi):
        """One sweep over all markers of all traits.  vare, var_effect, pi: one value per trait.  Returns {"sum_delta", "beta_ss",
        "alpha_ss", "resid_ss", "resid_sum", "n_changed"} (T values each) and "step_ms"."""
        T, _ = self._mega
        P, keep = self._mega_params(iteration, seed, vare, var_effect, pi)
        S = _lib.MegaStats()
        out = {k: np.zeros(T) for k in ("sum_delta", "beta_ss", "alpha_ss", "resid_ss", "resid_sum", "n_changed")}
        for k, a in out.items():
            setattr(S, k, a.ctypes.data)
        self._chk(self._L.jwas_hip_mega_sweep(self._h, C.byref(P), C.byref(S)))
        out["step_ms"] = S.step_ms
        return out

    def mega_accumulate(self, nsamples):
        self._chk(self._L.jwas_hip_mega_accumulate(self._h, float(nsamples)))

    def mega_sweep_r(self, *, iteration, seed, vare, var_effect, gamma, pi):
        """One BayesR sweep over all markers of all chains of the session (BayesR.jl:56-96 in double).  vare, var_effect (sigma2):
        one value per chain; gamma, pi: 4 x T (a vector of 4 serves every chain).  Returns {"class_counts" (4 x T), "ssq", "nnz",
        "alpha_ss", "resid_ss", "resid_sum", "n_changed"} (T values each) and "step_ms"."""
        T, _ = self._mega
        P = _lib.MegaRParams()
        P.iteration, P.seed = int(iteration), int(seed)
        keep = []
        for name, v in (("vare", vare), ("var_effect", var_effect)):
            a = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
            if a.size != T:
                raise ValueError(f"{name} must hold one value per chain ({T})")
            keep.append(a)
            setattr(P, name, a.ctypes.data)
        for name, v in (("gamma", gamma), ("pi", pi)):
            a = np.asarray(v, dtype=np.float64)
            if a.shape == (4,):
                a = np.repeat(a[:, None], T, axis=1)
            if a.shape != (4, T):
                raise ValueError(f"{name} must be 4 values or 4 x {T}")
            a = np.ascontiguousarray(a)
            keep.append(a)
            setattr(P, name, a.ctypes.data)
        S = _lib.MegaRStats()
        out = {k: np.zeros(T) for k in ("ssq", "nnz", "alpha_ss", "resid_ss", "resid_sum", "n_changed")}
        out["class_counts"] = np.zeros((4, T))
        for k, a in out.items():
            setattr(S, k, a.ctypes.data)
        self._chk(self._L.jwas_hip_mega_sweep_r(self._h, C.byref(P), C.byref(S)))
        out["step_ms"] = S.step_ms
        return out

    def mega_accumulate_r(self, nsamples):
        """mega_accumulate for BayesR chains: the model frequency is that of class > 1."""
        self._chk(self._L.jwas_hip_mega_accumulate_r(self._h, float(nsamples)))

    def mega_psrf(self, nsamples):
        """The potential scale reduction factor of every marker effect over the session's chains after `nsamples` accumulated
        samples (p values; NaN where no chain ever had the marker in the model)."""
        out = np.empty(self.p, dtype=np.float64)
        self._chk(self._L.jwas_hip_mega_psrf(self._h, float(nsamples), _ptr(out)))
        return out

    def mega_posterior(self, trait):
        """(mean, mean of squares, model frequency) of one trait's effects, p values each."""
        return self._blk_posterior(self._L.jwas_hip_mega_get_posterior, trait)

    def mega_mul_alpha(self, trait, output_rows=False):
        """X alpha_k over the training rows, or over the rows of load_output_dense."""
        return self._blk_mul_alpha(self._L.jwas_hip_mega_mul_alpha, trait, output_rows)

    def mega_gram(self, block):
        """(G, x'x) of one block: b x b and b doubles."""
        return self._blk_gram("mega", "get_gram", block)

    def mega_end(self):
        self._blk_end("mega")

    # -- unconstrained multi-trait BayesC with 5 to 8 traits (jwas_hip_mtj_*; MTBayesABC.jl:57-127, csrc/mtjoint.hpp) ------------
    def mtj_begin(self, ntraits, block_size=64):
        """Open a session of Gibbs sampler I with a full G, a full R and Pi over the 2^t joint states on the loaded genotypes: x'x
        and the block Grams; the residuals, alpha and beta start at 0, delta at 1."""
        self._chk(self._L.jwas_hip_mtj_begin(self._h, int(ntraits), int(block_size)))
        self._mtj = (int(ntraits), int(block_size) if block_size else 64)

    def mtj_set_residual(self, R):
        """R: T x n doubles."""
        self._blk_set_residual("mtj", R)

    def mtj_get_residual(self):
        return self._blk_get_residual("mtj")

    def mtj_set_state(self, alpha=None, beta=None, delta=None):
        """alpha, beta, delta: T x p doubles each, any may be None.  The state only: the residuals are not touched."""
        self._blk_set_state("mtj", alpha, beta, delta)

    def mtj_get_state(self):
        return self._blk_get_state("mtj")

    def mtj_gram(self, block):
        """(G, x'x) of one block: b x b and b doubles."""
        return self._blk_gram("mtj", "gram", block)

    def mtj_sweep(self, *, iteration, seed, rinv, ginv, log_pi):
        """One sweep of sampler I over all markers.  rinv = inv(vare), ginv = inv(G): T x T; log_pi: the 2^T log probabilities of the
        joint states (state = sum_k delta_k 2^k; -inf: never entered).  Returns {"state_counts" (2^T), "beta_ss" (T x T), "alpha_ss"
        (T), "resid_cp" (T x T), "resid_sum" (T), "n_changed", "step_ms"}."""
        T, _ = self._mtj
        P = _lib.MtjParams()
        P.iteration, P.seed = int(iteration), int(seed)
        keep = []
        for name, v in (("rinv", rinv), ("ginv", ginv)):
            a = np.ascontiguousarray(v, dtype=np.float64)
            if a.shape != (T, T):
                raise ValueError(f"{name} must be {T} x {T}")
            keep.append(a)
            setattr(P, name, a.ctypes.data)
        lp = np.ascontiguousarray(log_pi, dtype=np.float64).reshape(-1)
        keep.append(lp)
        P.log_pi, P.npi = lp.ctypes.data, lp.size
        S = _lib.MtjStats()
        out = {"state_counts": np.zeros(1 << T), "beta_ss": np.zeros((T, T)), "alpha_ss": np.zeros(T), "resid_cp": np.zeros((T, T)),
               "resid_sum": np.zeros(T)}
        for k, a in out.items():
            setattr(S, k, a.ctypes.data)
        self._chk(self._L.jwas_hip_mtj_sweep(self._h, C.byref(P), C.byref(S)))
        out["n_changed"], out["step_ms"] = S.n_changed, S.step_ms
        return out

    def mtj_accumulate(self, nsamples):
        self._chk(self._L.jwas_hip_mtj_accumulate(self._h, float(nsamples)))

    def mtj_posterior(self, trait):
        """(mean, mean of squares, model frequency) of one trait's effects, p values each."""
        return self._blk_posterior(self._L.jwas_hip_mtj_posterior, trait)

    def mtj_mul_alpha(self, trait, output_rows=False):
        """X alpha_k over the training rows, or over the rows of load_output_dense."""
        return self._blk_mul_alpha(self._L.jwas_hip_mtj_mul_alpha, trait, output_rows)

    def mtj_end(self):
        self._blk_end("mtj")

    # -- single-step analysis: the imputation solve (SSBR.jl:83-159; csrc/ssbr.hpp) -----------------
    @staticmethod
    def ss_estimate_bytes(n_n, g, nnz_l, nnz_u, nnz_a, markers_per_chunk):
        return _lib.load().jwas_hip_ss_estimate_bytes(int(n_n), int(g), int(nnz_l), int(nnz_u), int(nnz_a), int(markers_per_chunk))

    def ss_begin(self, factors, Ai_ng, budget_bytes=None, markers_per_chunk=None, g=None):
        """factors: scipy's SuperLU object of Ai_nn (splu), or (L, U, perm_r, perm_c); Ai_ng: n_n x g sparse.  A scipy matrix goes as CSR
        with sorted columns; an (indptr, indices, data) triple goes as it is.  The markers per chunk come from budget_bytes, or from
        markers_per_chunk (the budget of exactly that chunk); returned.  g: the number of genotyped individuals when Ai_ng is a triple."""
        L, U, perm_r, perm_c = (factors.L, factors.U, factors.perm_r, factors.perm_c) if hasattr(factors, "perm_r") else factors
        (lp, lc, lv), (up, uc, uv), (ap, ac, av) = (_csr_arrays(M) for M in (L, U, Ai_ng))
        perm_r, perm_c = (np.ascontiguousarray(v, dtype=np.int32) for v in (perm_r, perm_c))
        n_n = len(lp) - 1
        if len(up) - 1 != n_n or len(ap) - 1 != n_n or perm_r.shape != (n_n,) or perm_c.shape != (n_n,):
            raise ValueError(f"L, U, Ai_ng and the permutations must all have {n_n} rows")
        if g is None:
            g = int(Ai_ng.shape[1]) if hasattr(Ai_ng, "shape") else int(ac.max(initial=-1)) + 1
        if budget_bytes is None:
            budget_bytes = self.ss_estimate_bytes(n_n, g, len(lc), len(uc), len(ac), 1000 if markers_per_chunk is None else markers_per_chunk)
        ldc = C.c_int64(0)
        self._chk(self._L.jwas_hip_ss_begin(self._h, n_n, g, _ptr(lp), _ptr(lc), _ptr(lv), _ptr(up), _ptr(uc), _ptr(uv), _ptr(perm_r), _ptr(perm_c),
                                            _ptr(ap), _ptr(ac), _ptr(av), int(budget_bytes), C.byref(ldc)))
        self._ss = (n_n, g, ldc.value)
        return ldc.value

    def ss_set_rows(self, target, prow):
        """target "sweep" / 0: the dense sweep matrix; "output" / 1: the matrix of load_output_dense.  prow: rows of [M_n; M_g]."""
        prow = np.ascontiguousarray(prow, dtype=np.int32)
        self._chk(self._L.jwas_hip_ss_set_rows(self._h, {"sweep": 0, "output": 1}.get(target, target), prow.size, _ptr(prow)))

    def ss_impute(self, j0, Mg):
        """Mg: g x count, the genotyped individuals' block of markers [j0, j0 + count) in pedigree order, the engine's dtype."""
        Mg = np.asfortranarray(Mg, dtype=self.dtype)
        ss = getattr(self, "_ss", None)
        if Mg.ndim != 2 or (ss and Mg.shape[0] != ss[1]):
            raise ValueError("the genotyped block must be g x count")
        self._chk(self._L.jwas_hip_ss_impute(self._h, int(j0), Mg.shape[1], _ptr(Mg), Mg.shape[0]))
        self.block_size = 0

    def ss_get_columns(self, target, j0, count):
        """Columns [j0, j0 + count) of a target with ALL rows of its leading dimension (the n rows, then the pad rows): ld x count."""
        tg = {"sweep": 0, "output": 1}.get(target, target)
        ld = -(-(self.n if tg == 0 else getattr(self, "n_out", 0)) // 256) * 256
        out = np.empty((ld, int(count)), dtype=self.dtype, order="F")
        self._chk(self._L.jwas_hip_ss_get_columns(self._h, tg, int(j0), int(count), ld, _ptr(out)))
        return out

    def ss_solve_host(self, Mg, prow):
        """Rows prow of [Ai_nn \\ (-Ai_ng Mg); Mg] in Float64: len(prow) x count."""
        Mg = np.asfortranarray(Mg, dtype=np.float64)
        if Mg.ndim == 1:
            Mg = Mg.reshape(-1, 1, order="F")
        ss = getattr(self, "_ss", None)
        if Mg.ndim != 2 or (ss and Mg.shape[0] != ss[1]):
            raise ValueError("the genotyped block must be g x count")
        prow = np.ascontiguousarray(prow, dtype=np.int32)
        out = np.empty((prow.size, Mg.shape[1]), dtype=np.float64, order="F")
        self._chk(self._L.jwas_hip_ss_solve_host(self._h, Mg.shape[1], _ptr(Mg), Mg.shape[0], prow.size, _ptr(prow), _ptr(out)))
        return out

    def ss_end(self):
        self._chk(self._L.jwas_hip_ss_end(self._h))
        self._ss = None

    # -- GBLUP: the relationship matrix and the sampler on pseudo-markers (jwas_hip_grm, jwas_hip_gblup_*; csrc/gblup.hpp) --------
    GRM_CHUNK = _lib.GRM_CHUNK          # markers per fp32 accumulation chunk of grm() in a Float32 context

    @staticmethod
    def grm_estimate_bytes(n, p, precision=32):
        return _lib.load().jwas_hip_grm_estimate_bytes(int(n), int(p), int(precision))

    def grm(self, divisor):
        """K = (Z Z' + 1e-5 I) / p with Z = X ./ divisor of the loaded dense matrix (readgenotypes.jl:406-407): n x n in the engine's
        dtype, symmetric bit for bit.  divisor: p values, sqrt(2 p_j (1 - p_j)) in the engine's dtype."""
        d = np.ascontiguousarray(divisor, dtype=self.dtype)
        if d.shape != (self.p,):
            raise ValueError(f"divisor must have length {self.p}")
        K = np.empty((self.n, self.n), dtype=self.dtype)
        self._chk(self._L.jwas_hip_grm(self._h, _ptr(d), _ptr(K)))
        return K

    def grm_packed(self, divisor):
        """grm() of the 2-bit packed genotypes the engine holds (load_packed2bit, load_jgb2, plink_commit; readgenotypes.jl:403-408):
        n x n Float32, symmetric bit for bit, and bit for bit grm() of the dense matrix get_columns decodes.  divisor: p Float32
        values.  The storage, the state and an open session stay as they are."""
        d = np.ascontiguousarray(divisor, dtype=np.float32)
        if d.shape != (self.p,):
            raise ValueError(f"divisor must have length {self.p}")
        K = np.empty((self.n, self.n), dtype=np.float32)
        self._chk(self._L.jwas_hip_grm_packed2bit(self._h, _ptr(d), _ptr(K)))
        return K

    @staticmethod
    def gblup_estimate_bytes(n, ntraits=1, precision=32):
        return _lib.load().jwas_hip_gblup_estimate_bytes(int(n), int(ntraits), int(precision))

    def gblup_begin(self, D):
        """Open a GBLUP session on the loaded n x n matrix of eigenvectors (column i the i-th) with the eigenvalues D > 0; the
        residual and the effects are the context's (init_state first)."""
        D = np.ascontiguousarray(D, dtype=np.float64)
        if D.shape != (self.p,):
            raise ValueError(f"D must have length {self.p}")
        self._chk(self._L.jwas_hip_gblup_begin(self._h, _ptr(D)))

    def gblup_step(self, *, iteration, seed, vare, G, diagonal=False, first_trait=0):
        """One step of GBLUP! / megaGBLUP! (diagonal) / MTGBLUP! on the resident residual and effects.  vare, G: T x T (scalars for one
        trait); trait k draws the normals of coefficient first_trait + k.  Returns {"alpha_ss": sum_i alpha_i alpha_i' / D_i, "resid_ss", "resid_sum", "step_ms"}."""
        T = self.ntraits
        P, S = _lib.GblupParams(), _lib.GblupStats()
        P.iteration, P.seed, P.diagonal, P.first_trait = int(iteration), int(seed), int(bool(diagonal) or T == 1), int(first_trait)
        for name, v in (("vare", vare), ("G", G)):
            a = np.asarray(v, dtype=np.float64).reshape(-1)
            if a.size != T * T:
                raise ValueError(f"{name} must be {T} x {T}")
            getattr(P, name)[:T * T] = a.tolist()
        self._chk(self._L.jwas_hip_gblup_step(self._h, C.byref(P), C.byref(S)))
        return {"alpha_ss": np.array(S.alpha_ss[:T * T]).reshape(T, T), "resid_ss": np.array(S.resid_ss[:T * T]).reshape(T, T),
                "resid_sum": np.array(S.resid_sum[:T]), "step_ms": S.step_ms}

    def gblup_rhs(self):
        """The right-hand sides s_ik = l_i'(r_k + L alpha_k) of the last step: n x T doubles."""
        out = np.empty((self.n, self.ntraits), dtype=np.float64)
        self._chk(self._L.jwas_hip_gblup_get_rhs(self._h, out.size, _ptr(out)))
        return out

    def gblup_end(self):
        self._chk(self._L.jwas_hip_gblup_end(self._h))

    def mul_alpha_output(self, trait=0):
        """EBV = output_genotypes * alpha (output.jl:281-306)."""
        out = np.empty(getattr(self, "n_out", 0), dtype=self.dtype)
        self._chk(self._f("jwas_hip_mul_alpha_output")(self._h, int(trait), _ptr(out)))
        return out

    # -- the sweep -------------------------------------------------------------------------------
    # -- marker shards over GPUs (jwas_hip_comm_* / jwas_hip_sweep_sharded) ------------------------------
    @staticmethod
    def comm_unique_id():
        """128 bytes identifying a new RCCL communicator (rank 0 creates it, every rank passes it to comm_init)."""
        buf = (C.c_char * 128)()
        L = _lib.load()
        rc = L.jwas_hip_comm_unique_id(C.cast(buf, C.c_void_p))
        if rc != 0:
            raise JwasHipError(rc, L.jwas_hip_last_error(None).decode())
        return bytes(buf)

    def comm_init(self, unique_id, rank, world):
        buf = C.create_string_buffer(bytes(unique_id), 128)
        self._chk(self._L.jwas_hip_comm_init(self._h, C.cast(buf, C.c_void_p), int(rank), int(world)))
        self._comm = True

    def comm_info(self):
        """(rank, world) of the attached communicator as RCCL reports them (ncclCommUserRank / ncclCommCount)."""
        r, w = C.c_int32(0), C.c_int32(1)
        self._chk(self._L.jwas_hip_comm_info(self._h, C.byref(r), C.byref(w)))
        return r.value, w.value

    def comm_row_shards(self, enable=True):
        """Exact ROW shards (jwas_hip_comm_row_shards): this rank holds a slice of the individuals and all markers; call
        after comm_init (or comm_init_loopback) and before setup_blocks.  sweep() is then the exact chain of the pooled data."""
        self._chk(self._L.jwas_hip_comm_row_shards(self._h, 1 if enable else 0))

    def comm_init_loopback(self, slot, rank, world):
        """Test transport: the ranks are engines of ONE process driven by different host threads (exchange through host memory)."""
        self._chk(self._L.jwas_hip_comm_init_loopback(self._h, int(slot), int(rank), int(world)))

    def comm_destroy(self):
        self._chk(self._L.jwas_hip_comm_destroy(self._h))
        self._comm = False

    def sweep_sharded(self, **params):
        """sweep() on this rank's markers + the on-device reconcile (one RCCL all-reduce of delta r and the packed
        statistics); the returned statistics are the all-rank sums, the residual (get_residual) is the reconciled one."""
        return self.sweep(_sharded=True, **params)

    def sweep(self, *, iteration, seed, vare, var_effect, pi=0.0, pi_classes=None, gamma=BAYESR_GAMMA,
              log_prior_states=None, var_effect_vec=None, var_effect_matrix=None, pi_vec=None, pi_matrix=None, nreps=1,
              marker_offset=0, independent_blocks=False, section_solve=False, group_launch=False, resident_priors=False,
              _sharded=False):
        """One marker sweep.  Argument meaning follows BayesABC!/BayesR!/MTBayesABC!:
        vare: residual variance (scalar or t x t); var_effect: marker effect variance (BayesC scalar,
        BayesR sigmaSq, MT t x t); pi: Pr(effect = 0) scalar, or pi_vec per marker (length p, else the
        reference's length error); pi_classes / pi_matrix: BayesR class priors (4 or p x 4).  resident_priors: the per-marker
        prior table is the one an open annotation session keeps on the device (annot_begin / annot_step): no prior pointer
        and no pi_classes are passed."""
        t = self.ntraits
        if resident_priors:
            if pi_vec is not None or pi_matrix is not None or np.ndim(pi) == 1 or np.ndim(pi_classes) == 2 or np.ndim(log_prior_states) == 2:
                raise ValueError("resident_priors=True takes no per-marker prior: the annotation session holds it")
        P = SweepParams()
        P.method, P.ntraits, P.nreps = self.method, t, int(nreps)
        P.iteration, P.seed, P.marker_offset = int(iteration), int(seed), int(marker_offset)
        P.independent_blocks = 1 if independent_blocks else 0          # BayesABC_block_independent! (BayesABC.jl:190-255)
        P.section_solve = 1 if section_solve else 0                    # Rule T: dense chains as triangular solves (jwas_hip.h)
        P.group_launch = 1 if group_launch else 0                      # grouped launches (setup_groups; jwas_hip.h)
        ve = np.asarray(vare, dtype=np.float32).reshape(-1)
        vg = np.asarray(var_effect, dtype=np.float32).reshape(-1)
        if ve.size != t * t or vg.size != t * t:
            raise ValueError(f"vare / var_effect must have {t}x{t} entries")
        ve64 = np.asarray(vare, dtype=np.float64).reshape(-1)
        vg64 = np.asarray(var_effect, dtype=np.float64).reshape(-1)
        for i in range(t * t):
            P.vare[i] = float(ve[i])
            P.var_effect[i] = float(vg[i])
            P.vare_f64[i] = float(ve64[i])              # (read by Float64 contexts: the variances as the reference holds them there)
            P.var_effect_f64[i] = float(vg64[i])
        P.pi = float(pi) if np.ndim(pi) == 0 else 0.0      # (vector pi: per marker, or per trait for megaBayesABC)
        keep = []
        if self.method in (_lib.MTBAYESB1, _lib.MTBAYESB2, _lib.MEGABAYESB):     # multi-trait BayesA/B: one t x t effect covariance per marker
            if var_effect_matrix is not None:     # (None: the covariances resident on the device -- sample_marker_covariances)
                vm = np.ascontiguousarray(var_effect_matrix, dtype=self.dtype)
                if vm.shape != (self.p, t, t):
                    raise ValueError(f"var_effect_matrix must be {self.p} x {t} x {t}")
                if self.precision == 64:          # (a Float64 context keeps them in double: uploaded here, the sweep reads them in place)
                    self._chk(self._L.jwas_hip_set_marker_covariances_f64(self._h, _ptr(vm)))
                else:
                    keep.append(vm)
                    P.var_effect_matrix = vm.ctypes.data_as(C.POINTER(C.c_float))
        if self.method in (_lib.BAYESC, _lib.BAYESB):
            if np.ndim(pi) == 1:
                pi_vec = pi
            if pi_vec is not None:
                pv = np.ascontiguousarray(pi_vec, dtype=np.float64)
                if pv.shape != (self.p,):
                    # bayesabc_pi_vector (BayesABC.jl:16-22)
                    raise ValueError(f"BayesABC pi vector length {pv.size} must match the number of markers ({self.p}).")
                P.pi_vec = pv.ctypes.data_as(C.POINTER(C.c_double))
                keep.append(pv)
            if self.method == _lib.BAYESB:
                if var_effect_vec is None:
                    raise ValueError("BayesB needs per-marker effect variances")
                vv = np.ascontiguousarray(var_effect_vec, dtype=self.dtype)
                if vv.shape != (self.p,):
                    raise ValueError(f"BayesB variance vector must have length {self.p}")
                if self.precision == 64:
                    P.var_effect_vec_f64 = vv.ctypes.data_as(C.POINTER(C.c_double))
                else:
                    P.var_effect_vec = vv.ctypes.data_as(C.POINTER(C.c_float))
                keep.append(vv)
        elif self.method == _lib.BAYESR:
            g = np.asarray(gamma, dtype=np.float64)
            for k in range(4):
                P.gamma[k] = float(g[k])
            pc = pi_classes
            if pc is not None and np.ndim(pc) == 2:
                pi_matrix, pc = pc, None
            if pi_matrix is not None:
                pm = np.ascontiguousarray(pi_matrix, dtype=np.float64)
                # bayesr_validate_priors (BayesR.jl:16-20)
                if pm.shape[0] != self.p:
                    raise ValueError("BayesR per-marker pi must have one row per marker.")
                if pm.shape[1] != 4:
                    raise ValueError("BayesR per-marker pi must have 4 columns.")
                P.pi_matrix = pm.ctypes.data_as(C.POINTER(C.c_double))
                keep.append(pm)
            elif not resident_priors:
                pc = np.asarray(pc, dtype=np.float64)
                if pc.shape != (4,):
                    raise ValueError(f"BayesR pi vector length {pc.size} must match the number of mixture classes (4).")
                for k in range(4):
                    P.pi_classes[k] = float(pc[k])
        elif self.method in (_lib.MEGABAYESC, _lib.MEGABAYESB):
            # megaBayesABC! (BayesABC.jl:1-8): one pi per trait (genotypes.pi[i])
            pt = np.asarray(pi, dtype=np.float64).reshape(-1)
            if pt.shape != (t,):
                raise ValueError(f"megaBayesABC needs one pi per trait ({t}), got {pt.size}")
            for k in range(t):
                P.pi_classes[k] = float(pt[k])
        elif not resident_priors:
            lp = np.asarray(log_prior_states, dtype=np.float64)
            if lp.ndim == 2:                      # marker-specific joint priors (MarkerSpecificPiPrior, MTBayesABC.jl:22-47)
                if lp.shape != (self.p, 1 << t):
                    raise ValueError(f"marker-specific log_prior_states must be {self.p} x {1 << t}")
                lpm = np.ascontiguousarray(lp)
                keep.append(lpm)
                P.log_prior_states_matrix = lpm.ctypes.data_as(C.POINTER(C.c_double))
            else:
                if lp.shape != (1 << t,):
                    raise ValueError(f"log_prior_states must have {1 << t} entries")
                for k in range(1 << t):
                    P.log_prior_states[k] = float(lp[k])
        self._keep = keep
        S = SweepStats()
        self._chk((self._L.jwas_hip_sweep_sharded if _sharded else self._L.jwas_hip_sweep)(self._h, C.byref(P), C.byref(S)))
        return {
            "sum_delta": np.array(S.sum_delta[:t]),
            "alpha_ss": np.array(S.alpha_ss[:t * t]).reshape(t, t),
            "beta_ss": np.array(S.beta_ss[:t * t]).reshape(t, t),
            "resid_ss": np.array(S.resid_ss[:t * t]).reshape(t, t),
            "resid_sum": np.array(S.resid_sum[:t]),
            "class_counts": np.array(S.class_counts[:4]),
            "bayesr_ssq": S.bayesr_ssq, "bayesr_nnz": S.bayesr_nnz,
            "state_counts": np.array(S.state_counts[:1 << t]),
            "n_events": S.n_events, "sweep_ms": S.sweep_ms,
            "update_kernel_ms": S.update_kernel_ms, "update_kernel_samples": S.update_kernel_samples,
            "update_kernel_bytes": S.update_kernel_bytes, "event_overhead_ms": S.event_overhead_ms,
        }

    # -- multi-trait BayesA/B: per-marker effect covariances drawn on the device --------------------
    def sample_marker_covariances(self, df, scale, *, seed, iteration, marker_offset=0):
        """G_j ~ InverseWishart(df, scale + b_j b_j') for every marker from the current beta (variance_components.jl:181-186,
        df = the reference's df + 1); the next sweep(var_effect_matrix=None) uses them in place."""
        sc = np.ascontiguousarray(scale, dtype=np.float64).reshape(-1)
        if sc.size != self.ntraits * self.ntraits:
            raise ValueError(f"scale must be {self.ntraits} x {self.ntraits}")
        self._chk(self._L.jwas_hip_sample_marker_covariances(self._h, float(df), sc.ctypes.data_as(C.POINTER(C.c_double)), int(seed),
                                                             int(iteration), int(marker_offset)))

    def marker_covariances(self):
        """The resident p x t x t per-marker covariances (float32; float64 in a Float64 context)."""
        out = np.empty((self.p, self.ntraits, self.ntraits), dtype=self.dtype)
        self._chk(self._f("jwas_hip_get_marker_covariances")(self._h, _ptr(out)))
        return out

    # -- posterior accumulators --------------------------------------------------------------------
    def accumulate(self, nsamples):
        self._chk(self._L.jwas_hip_accumulate(self._h, float(nsamples)))

    def posterior(self, trait=0):
        ma = np.empty(self.p, dtype=self.dtype)
        ma2 = np.empty(self.p, dtype=self.dtype)
        md = np.empty(self.p, dtype=self.dtype)
        self._chk(self._f("jwas_hip_get_posterior")(self._h, int(trait), _ptr(ma), _ptr(ma2), _ptr(md)))
        return ma, ma2, md
