"""Generators and references for the direct tests of the fp64 dense layer (csrc/dla.h: dgemm.hip,
chol.hip), shared by test_dla_ref_cpu.py (checks these helpers, no GPU) and test_gpu_dla.py.

GEMM and dot data are exact by construction: integer-valued operands small enough that every partial
sum, in any order and with or without FMA, is an integer below 2^52, so the float64 result has one
correct value and numpy's float64 product on the same data is that value.

Cholesky data are well-conditioned SPD matrices with a np.longdouble reference for n <= 257.
"""
import functools

import numpy as np

# ---------------------------------------------------------------- shapes (M, N, K) per kernel path
# dgemm.hip launch(): dot_kernel when M*N <= 64 and K >= 256; gemv_rows / gemv_cols when N <= 8 and
# K >= 256 (rows: A stored along k, trans_a = 0; cols: trans_a = 1); split-K when fewer than 256 64x64
# tiles and K >= 1024; the tiled kernel otherwise.
DOT_SHAPES = [(1, 1, 256), (3, 5, 257), (8, 8, 1000), (64, 1, 300), (1, 64, 4096)]
GEMV_SHAPES = [(65, 1, 256), (9, 8, 256), (67, 3, 300), (130, 8, 515), (257, 2, 777), (300, 8, 1024)]
# (1, 1, 255) sits just below the dot / gemv boundary K = 256, (300, 9, 1024) just above N = 8 (and, with
# K = 1024, in split-K: listed there)
TILED_SHAPES = [(1, 1, 255), (1, 9, 1), (16, 16, 4), (63, 65, 15), (64, 64, 16), (65, 63, 17), (129, 130, 33),
                (200, 70, 255), (70, 200, 1023)]
SPLITK_SHAPES = [(64, 64, 1024), (65, 9, 1025), (300, 9, 1024), (130, 70, 2050), (100, 100, 4096)]
SPLITK_BIG = (960, 960, 1030)  # 15 x 15 = 225 tiles < 256: 768 // 225 = 3 splits
# int8 operands: one shape of each group and the two caller shapes (epi_plan.hip) scaled down
INT8_SHAPES = [(3, 5, 257), (130, 8, 515), (65, 63, 17), (130, 70, 2050), (128, 192, 192), (128, 64, 192)]
MASK_SIZES = (64, 65, 130, 200, 1100)
ALPHA_BETA = [(1.0, 0.0), (-1.0, 1.0), (0.5, -1.0), (2.0, 1.0)]
TRANS = [(0, 0), (0, 1), (1, 0), (1, 1)]
K_MAX = 4096
PAD = 3  # lda, ldb, ldc are each this much above the dense extent

DOT_ROWS_SHAPES = [(1, 1), (3, 63), (4, 64), (5, 65), (130, 1000)]

CHOL_SMALL_N = (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200, 257)
CHOL_SPLIT_N = 3530  # 56 blocks of 64, the last of 10 rows
CHOL_PAD = 5

C_SENTINEL = -123456789.0  # the value of C's padding columns (an integer no product here yields by chance)


def dgemm_path(M, N, K, trans_a, mask=0):
    """The kernel dgemm.hip launch() picks (a copy of its conditions: see launch() in dgemm.hip)."""
    if mask == 0 and K >= 256 and M * N <= 64:
        return "dot"
    if mask == 0 and K >= 256 and N <= 8:
        return "gemv_cols" if trans_a else "gemv_rows"
    tiles = -(-N // 64) * -(-M // 64)
    if mask == 0 and tiles < 256 and K >= 1024:
        return "splitk"
    return "tiled"


def splitk_splits(M, N):
    tiles = -(-N // 64) * -(-M // 64)
    return min(8, max(2, 768 // tiles))


# ---------------------------------------------------------------- exact GEMM data


def _ints(rng, shape, bound):
    return rng.integers(-bound, bound, size=shape, endpoint=True).astype(np.float64)


def store(mat, trans, pad, fill):
    """The storage of a logical matrix: row-major, or its transpose when trans, with `pad` extra columns
    of `fill`."""
    m = np.ascontiguousarray(mat.T if trans else mat)
    buf = np.full((m.shape[0], m.shape[1] + pad), fill, dtype=m.dtype)
    buf[:, :m.shape[1]] = m
    return buf


def gemm_case(seed, M, N, K, alpha=1.0, beta=0.0, trans_a=0, trans_b=0, a_i8=False, b_i8=False, pad=PAD):
    """One exact product: logical a (M x K), b (K x N), c0 (M x N), their padded storage (NaN in the
    double operands' padding, -128 in an int8 operand's, C_SENTINEL in C's; the live part of C is NaN
    when beta == 0) and the float64 reference alpha a b + beta c0 with its exact sum s = a b."""
    assert not (a_i8 and b_i8)
    rng = np.random.default_rng(seed)
    wide = 2 ** 30 if (a_i8 or b_i8) else 2 ** 19
    a = _ints(rng, (M, K), 128).clip(-128, 127) if a_i8 else _ints(rng, (M, K), wide)
    b = _ints(rng, (K, N), 128).clip(-128, 127) if b_i8 else _ints(rng, (K, N), wide)
    if a_i8:  # the whole range, both ends present whatever the draw
        a.flat[0], a.flat[-1] = -128, 127
    if b_i8:
        b.flat[0], b.flat[-1] = -128, 127
    c0 = _ints(rng, (M, N), 2 ** 40)
    amax, bmax = np.abs(a).max(), np.abs(b).max()
    # every partial sum is an integer below 2^52, and so is the epilogue's result (times 2 for alpha = 0.5)
    assert K <= K_MAX and K * amax * bmax * max(1.0, abs(alpha)) + abs(beta) * np.abs(c0).max() < 2.0 ** 52, \
        "gemm_case: magnitude bound exceeded (K = %d)" % K
    s = a @ b
    ref = alpha * s + (beta * c0 if beta != 0.0 else 0.0)
    a_st = store(a.astype(np.int8) if a_i8 else a, trans_a, pad, -128 if a_i8 else np.nan)
    b_st = store(b.astype(np.int8) if b_i8 else b, trans_b, pad, -128 if b_i8 else np.nan)
    c_st = np.full((M, N + pad), C_SENTINEL)
    c_st[:, :N] = c0 if beta != 0.0 else np.nan
    return dict(M=M, N=N, K=K, alpha=alpha, beta=beta, trans_a=trans_a, trans_b=trans_b, a_i8=a_i8, b_i8=b_i8,
                a=a, b=b, c0=c0, s=s, ref=ref, a_st=a_st, b_st=b_st, c_st=c_st)


def exact_entries(case, idx):
    """alpha-free exact sums s[i, j] for the (i, j) in idx, in Python integers."""
    a, b = case["a"], case["b"]
    out = []
    for i, j in idx:
        out.append(sum(int(x) * int(y) for x, y in zip(a[i], b[:, j])))
    return out


def lower_int_matrix(seed, n):
    """Integer-valued lower-triangular X (entries within 2^19), for the mask = 2 product X'X."""
    return np.tril(_ints(np.random.default_rng(seed), (n, n), 2 ** 19))


def tile_lower_mask(n, tile=64):
    """True where the 64 x 64 tile has tile_row >= tile_col: the part a masked product defines."""
    t = np.arange(n) // tile
    return t[:, None] >= t[None, :]


def dot_rows_case(seed, rows, n, pad=0):
    rng = np.random.default_rng(seed)
    a = _ints(rng, (rows, n), 2 ** 19)
    b = _ints(rng, (rows, n), 2 ** 19)
    assert n <= K_MAX and n * 2.0 ** 38 < 2.0 ** 52
    return dict(a=a, b=b, a_st=store(a, 0, pad, np.nan), b_st=store(b, 0, pad, np.nan))


# ---------------------------------------------------------------- real-valued epilogue


def longdouble_ok():
    return np.finfo(np.longdouble).eps < 2e-19


def epilogue_bound(case):
    """(ref, bound): alpha s + beta c0 in np.longdouble and 2 ulp(|alpha s| + |c0|).  s is exact; the
    kernel forms alpha s (one rounding, at most half an ulp of |alpha s|) and adds beta c0 (exact for
    beta = -1; one more rounding of at most half an ulp of the sum's magnitude), or fuses the two."""
    al = np.longdouble(case["alpha"])
    s = case["s"].astype(np.longdouble)
    c0 = case["c0"].astype(np.longdouble)
    ref = al * s + np.longdouble(case["beta"]) * c0
    mag = (np.abs(al * s) + np.abs(c0)).astype(np.float64)
    return ref, 2.0 * np.spacing(mag)


# ---------------------------------------------------------------- Cholesky data and references


@functools.lru_cache(maxsize=None)
def spd_matrix(n):
    """A = G G' / c + I, G n x (n + 5) standard normal, c = n + 5: 2-norm condition number about 6."""
    g = np.random.default_rng(1000 + n).standard_normal((n, n + CHOL_PAD))
    a = g @ g.T / (n + CHOL_PAD) + np.eye(n)
    a = 0.5 * (a + a.T)
    a.setflags(write=False)
    return a


def chol_ld(a):
    """Lower Cholesky factor in np.longdouble, column by column."""
    a = np.asarray(a, dtype=np.longdouble)
    n = a.shape[0]
    L = np.zeros((n, n), dtype=np.longdouble)
    for j in range(n):
        v = a[j:, j] - L[j:, :j] @ L[j, :j]
        L[j, j] = np.sqrt(v[0])
        L[j + 1:, j] = v[1:] / L[j, j]
    return L


def lower_inverse_ld(L):
    """inv(L) of a lower-triangular L by forward substitution, in np.longdouble."""
    L = np.asarray(L, dtype=np.longdouble)
    n = L.shape[0]
    X = np.zeros((n, n), dtype=np.longdouble)
    for i in range(n):
        row = -(L[i, :i] @ X[:i, :])
        row[i] += 1.0
        X[i] = row / L[i, i]
    return X


@functools.lru_cache(maxsize=None)
def chol_reference(n):
    """The np.longdouble reference of spd_matrix(n): L, L^-1, A^-1 = L^-T L^-1, logdet = 2 sum log L_jj,
    and the residuals of numpy's float64 LAPACK results on the same matrix."""
    a = spd_matrix(n)
    L = chol_ld(a)
    X = lower_inverse_ld(L)
    ainv = X.T @ X
    logdet = 2.0 * np.sum(np.log(np.diag(L)))
    Lf = np.linalg.cholesky(a)
    Xf = np.linalg.inv(Lf)
    Af = np.linalg.inv(a)
    lapack = dict(L=resid_llt(Lf, a), linv=resid_inverse(Xf, L), ainv=resid_inverse(Af, a))
    for v in (L, X, ainv):
        v.setflags(write=False)
    return dict(a=a, L=L, linv=X, ainv=ainv, logdet=logdet, lapack=lapack)


def resid_llt(L, a):
    """max |L L' - A| in np.longdouble (L's lower triangle)."""
    L = np.tril(np.asarray(L, dtype=np.longdouble))
    return float(np.abs(L @ L.T - np.asarray(a, dtype=np.longdouble)).max())


def resid_inverse(x, m):
    """max |X M - I| in np.longdouble."""
    x = np.asarray(x, dtype=np.longdouble)
    m = np.asarray(m, dtype=np.longdouble)
    return float(np.abs(x @ m - np.eye(m.shape[0], dtype=np.longdouble)).max())


def resid_floor(n, a):
    """n 2^-52 max|A|: the residual that rounding the result itself accounts for."""
    return n * 2.0 ** -52 * float(np.abs(a).max())


# ---------------------------------------------------------------- chol.hip cholesky_steps task counts

CHOL_SPLIT = 1536  # chol.hip: constexpr int CHOL_SPLIT


def chol_step_plan(n, linv, keep_l, vinv):
    """A copy of the per-step task counts of cholesky_steps (chol.hip): [(k, has_d, tasks, split)] for
    every step that launches anything."""
    K = -(-n // 64)
    out = []
    for k in range(-1, K + (1 if vinv else 0) + 1):
        r = K - 1 - k
        nt1 = nt3 = 0
        if 0 <= k < K:
            nt1 = r * (r + 1) // 2 - 1 if r >= 1 else 0
            nt3 = r * (k + 1) if linv else 0
        nd = 1 if k + 1 < K else 0
        nwl = K - k if (1 <= k <= K and keep_l) else 0
        nwx = k if (1 <= k <= K and linv) else 0
        q = k - 2
        nt5 = (q + 1) * (q + 2) // 2 if (vinv and 0 <= q < K) else 0
        grid = nt1 + nt3 + nwl + nwx + nt5
        if nd + grid > 0:
            out.append((k, bool(nd), grid, bool(nd and grid >= CHOL_SPLIT)))
    return out
