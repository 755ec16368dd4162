"""A plain float64 reference of every inner product the setup kernels precompute (k_xpx, k_gram_f64, k_cross_f64, k_gram_mfma,
k_cross_mfma128): x'R^-1 x, the block Grams, the cross-Grams of consecutive blocks and the pair / four cross-Grams of grouped
launches -- from the decoded matrix X (float32 values), the weights w and a partition.

    S[a, c] = sum_k x_ak * fl32(x_ck * w_k)          T[a, c] = sum_k |x_ak * fl32(x_ck * w_k)|

The float32 rounding of the WEIGHTED operand is the one piece of the device's arithmetic the definition carries (the weight rides
on the column operand, rounded once, before both operands widen); everything else is numpy float64 matrix products.  With unit
weights (w = None) fl32(x * 1) = x and S is the plain X'X.

The error bounds the GPU tests assert are derived, not tuned:

  * "f64" mode -- the device sums the same float64 products and rounds the total to float32 once:
        |G - S| <= 2^-24 |S| + ld 2^-52 T
    (one float32 rounding of a float64 sum, plus the summation error of two float64 sums of at most ld terms each, the device's
    and this module's, ld 2^-53 T apiece; ld = the row count padded to 256, the padding rows are zeros);
  * "mfma" mode -- float32 products accumulated in float32 over chunks of 64 rows, the chunks folded into float64:
        |G - S| <= 65 2^-23 T + 2^-24 |S|
    (gamma_64 = 64 u / (1 - 64 u) <= 65 u for 64 products and their sums in any order, with u taken as 2^-23 -- twice the unit
    roundoff -- so that the bound does not lean on how the matrix instruction rounds internally; the float64 fold and this module's
    own sums are orders below that; the last term is the final rounding to float32).
"""
import numpy as np

from conftest import make_dataset

U24 = 2.0 ** -24


def padded_rows(n):
    """The device's leading dimension: rows padded to a multiple of 256."""
    return (int(n) + 255) // 256 * 256


def operands(X, w=None):
    """(A, B) in float64: A = X, B = fl32(X .* w) -- the row and the column operand of every product."""
    X = np.asarray(X, dtype=np.float32)
    A = X.astype(np.float64)
    if w is None:
        return A, A
    B = (X * np.asarray(w, dtype=np.float32)[:, None]).astype(np.float32).astype(np.float64)
    return A, B


def products(X, w, rows, cols):
    """S and T between the markers `rows` (a slice: the row operand) and `cols` (the weighted column operand)."""
    A, B = operands(X, w)
    A, B = A[:, rows], B[:, cols]
    return A.T @ B, np.abs(A).T @ np.abs(B)


def xpx(X, w=None):
    A, B = operands(X, w)
    return (A * B).sum(axis=0), np.abs(A * B).sum(axis=0)


def gram(X, w, j0, b):
    return products(X, w, slice(j0, j0 + b), slice(j0, j0 + b))


def cross(X, w, jp, bp, j0, b):
    """X_prev' R^-1 X_this: rows = the bp markers from jp, columns = the b markers from j0."""
    return products(X, w, slice(jp, jp + bp), slice(j0, j0 + b))


def partition(p, block_size=None, starts=None):
    """[(j0, b)] of uniform blocks, or of explicit 0-based block starts."""
    st = list(range(0, p, block_size)) if starts is None else [int(s) for s in starts]
    return [(s, (st[k + 1] if k + 1 < len(st) else p) - s) for k, s in enumerate(st)]


def group_cross(X, w, block_size, level, index):
    """The cross-Gram of grouped launches between group index - 1 (rows) and group index (columns): groups of 2^level blocks."""
    gb = (1 << level) * block_size
    p = np.asarray(X).shape[1]
    return cross(X, w, (index - 1) * gb, gb, index * gb, min(gb, p - index * gb))


def mirrored(M, keep=None):
    """A Gram as the device DEFINES it: the entries a >= c as computed, the rest their mirror image; `keep` (boolean b x b): the
    entries the device computes on their own in both triangles."""
    a, c = np.indices(M.shape)
    own = a >= c if keep is None else (a >= c) | keep
    return np.where(own, M, M.T)


def bound_f64(S, T, ld):
    return U24 * np.abs(S) + ld * 2.0 ** -52 * T


def bound_mfma(S, T):
    return 65 * 2.0 ** -23 * T + U24 * np.abs(S)


# ---- the datasets of tests/test_gpu_precompute.py (tests/test_precompute_host.py checks what the bounds can see on them) --------
def integer_genotypes(n, p, seed):
    """Uncentred 0/1/2 genotypes, no missing codes: every product and partial sum is a small integer."""
    rng = np.random.default_rng(seed)
    return np.asfortranarray(rng.integers(0, 3, size=(n, p)).astype(np.float32))


def integer_weights(n, seed):
    return np.random.default_rng(1000 + seed).integers(1, 5, size=n).astype(np.float32)


def centred_genotypes(n, p, seed):
    return make_dataset(n=n, p=p, ncausal=min(4, p), seed=seed)["X"]


def positive_weights(n, seed):
    return np.random.default_rng(2000 + seed).uniform(0.3, 3.0, n).astype(np.float32)


def packed_genotypes(n, p, seed, centered):
    """(codes n x p uint8 with missing fields (3), means, the decoded matrix) of a 2-bit packed matrix: a missing field decodes to
    the marker's mean (0 when centred)."""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.1, 0.4, size=p)
    codes = ((rng.random((n, p)) < f).astype(np.uint8) + (rng.random((n, p)) < f).astype(np.uint8))
    miss = rng.random((n, p)) < 0.03
    miss[0, :] = False                                                    # (every marker keeps an observed field)
    codes[miss] = 3
    raw = codes.astype(np.float32)
    means = np.array([raw[~miss[:, j], j].mean(dtype=np.float32) for j in range(p)], dtype=np.float32)
    v = np.where(miss, means[None, :], raw).astype(np.float32)
    X = np.asfortranarray((v - means[None, :]).astype(np.float32) if centered else v)
    return codes, means, X


# (block size, markers, rows) of the uniform partitions: a ragged last block below / above a 64-marker tile edge, an exact multiple
# of the block size, a single block shorter than the block size; rows that are no multiple of 4 or 32, padded to 256 and to 512
UNIFORM_SHAPES = [(64, 2 * 64 + 37, 300), (128, 2 * 128 + 65, 257), (256, 256 + 130, 300), (1024, 1024 + 70, 65), (64, 3 * 64, 65),
                  (128, 50, 257)]
EXPLICIT_STARTS = [0, 1, 64, 129, 130, 300]           # p = 470: blocks of 1, 63, 65, 1, 170, 170 markers
EXPLICIT_P, EXPLICIT_N = 470, 300
# (block size, markers, rows, blocks per launch) of the grouped launches (the comment in tests/test_gpu_precompute.py says why)
GROUP_SHAPES = [(64, p, n, m) for p, n in ((100, 257), (128 + 50, 300), (2 * 128 + 30, 65), (4 * 128 + 64, 300)) for m in (2, 4)]
GROUP_SHAPES.append((128, 2 * 512 + 300, 257, 4))
SECOND_SIZE_P, SECOND_SIZE_N = 2 * 128 + 65, 257      # two resident block sizes (64 and 128)
