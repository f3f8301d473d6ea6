"""Direct tests of the fp64 dense layer (csrc/dla.h: dgemm.hip, chol.hip) through the gmat_probe_dgemm /
gmat_probe_cholesky / gmat_probe_dot_rows entry points, against the references of tests/dla_ref.py.

GEMM and dot_rows data are exact by construction (integer-valued, every partial sum below 2^52), so the
device result must equal the reference bit for bit whatever kernel, summation order or FMA contraction
produced it.  The Cholesky outputs are held against an np.longdouble reference (n <= 257) or numpy's
float64 LAPACK (n = 3530).

Kernel paths and the shapes that reach them (dla_ref.dgemm_path copies launch()'s conditions and
test_dla_ref_cpu.py pins the table to it): dot_kernel (1,1,256)...(1,64,4096); gemv_rows / gemv_cols
(65,1,256)...(300,8,1024) with trans_a = 0 / 1; tiled (1,1,255)...(70,200,1023) and every masked product;
split-K (64,64,1024)...(960,960,1030) (3 splits); the int8 loaders on one shape of each.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dla_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _lib():
    from gmat_amd import _native as N
    return N, N.ensure_device()


def run_dgemm(case, mask=0):
    """The probe on a case of dla_ref.gemm_case; returns the whole M x ldc buffer."""
    N, lib = _lib()
    a, b, c = case["a_st"], case["b_st"], case["c_st"].copy()
    N.check(lib.gmat_probe_dgemm(case["M"], case["N"], case["K"], case["alpha"], case["beta"], mask,
                                 N.ptr(a), int(case["a_i8"]), case["trans_a"], a.shape[1],
                                 N.ptr(b), int(case["b_i8"]), case["trans_b"], b.shape[1],
                                 N.ptr(c), c.shape[1]), "gmat_probe_dgemm")
    return c


def check_exact(case, what):
    got = run_dgemm(case)
    n = case["N"]
    assert not np.isnan(got).any(), what
    np.testing.assert_array_equal(got[:, n:], R.C_SENTINEL, err_msg="%s: C's padding written" % (what,))
    np.testing.assert_array_equal(got[:, :n], case["ref"], err_msg=str(what))


def sweep(shapes, path, trans=R.TRANS, alpha_beta=R.ALPHA_BETA, **kw):
    seed = 0
    for (M, N, K) in shapes:
        for ta, tb in trans:
            if path is not None:
                want = path if path != "gemv" else ("gemv_cols" if ta else "gemv_rows")
                assert R.dgemm_path(M, N, K, ta) == want
            for alpha, beta in alpha_beta:
                seed += 1
                case = R.gemm_case(seed, M, N, K, alpha, beta, ta, tb, **kw)
                check_exact(case, (path, M, N, K, ta, tb, alpha, beta, kw))


# ---------------------------------------------------------------- dgemm, exact


def test_dgemm_tiled_exact():
    sweep(R.TILED_SHAPES, "tiled")


def test_dgemm_dot_exact():
    sweep(R.DOT_SHAPES, "dot")


def test_dgemm_gemv_exact():
    sweep(R.GEMV_SHAPES, "gemv")


def test_dgemm_splitk_exact():
    """ldc = N + 3 while the partial products have pitch N; beta != 0 goes through splitk_sum_kernel."""
    sweep(R.SPLITK_SHAPES, "splitk")


def test_dgemm_splitk_three_splits_exact():
    """225 tiles, 3 splits of 352 (K = 1030: the last split is short and ends inside a K-step)."""
    sweep([R.SPLITK_BIG], "splitk", trans=[(0, 0), (1, 1)], alpha_beta=[(0.5, -1.0)])


def test_dgemm_int8_a_exact():
    """dgemm_i8a: the gemv / dot kernels index the int8 pointer themselves."""
    sweep(R.INT8_SHAPES, None, trans=[(0, 0), (1, 1)], a_i8=True)
    sweep(R.INT8_SHAPES, None, trans=[(0, 1), (1, 0)], alpha_beta=[(-1.0, 1.0)], a_i8=True)


def test_dgemm_int8_b_exact():
    sweep(R.INT8_SHAPES, None, trans=[(0, 0), (1, 1)], b_i8=True)
    sweep(R.INT8_SHAPES, None, trans=[(0, 1), (1, 0)], alpha_beta=[(-1.0, 1.0)], b_i8=True)


def test_dgemm_both_int8_is_an_argument_error():
    N, lib = _lib()
    a = np.zeros((4, 4), dtype=np.int8)
    c = np.zeros((4, 4))
    assert lib.gmat_probe_dgemm(4, 4, 4, 1.0, 0.0, 0, N.ptr(a), 1, 0, 4, N.ptr(a), 1, 0, 4, N.ptr(c), 4) != 0


@pytest.mark.parametrize("n", R.MASK_SIZES)
def test_dgemm_masks_exact(n):
    """mask = 1 (general operands) and mask = 2 (X'X for a lower-triangular X, the L^-T L^-1 use): the
    64 x 64 tiles with tile_row >= tile_col equal the reference.  The other tiles are unspecified (the
    kernel skips them) and are not asserted on.  n = 1100 has K >= 1024 and fewer than 256 tiles: a
    masked product must not be split (the split-K sum would write every tile)."""
    low = R.tile_lower_mask(n)
    for alpha, beta in ((1.0, 0.0), (-1.0, 1.0)):
        for ta, tb in ((0, 0), (1, 0)):
            case = R.gemm_case(n + ta, n, n, n, alpha, beta, ta, tb)
            got = run_dgemm(case, mask=1)
            np.testing.assert_array_equal(got[:, n:], R.C_SENTINEL)
            np.testing.assert_array_equal(got[:, :n][low], case["ref"][low])
            if beta != 0.0:  # a skipped tile keeps C as it was
                np.testing.assert_array_equal(got[:, :n][~low], case["c0"][~low])
        x = R.lower_int_matrix(n, n)
        c0 = R.gemm_case(n, n, n, 1, beta=1.0)["c0"]
        c_st = np.full((n, n + R.PAD), R.C_SENTINEL)
        c_st[:, :n] = c0 if beta != 0.0 else np.nan
        case = dict(M=n, N=n, K=n, alpha=alpha, beta=beta, trans_a=1, trans_b=0, a_i8=False, b_i8=False,
                    a_st=R.store(x, 0, R.PAD, np.nan), b_st=R.store(x, 0, R.PAD, np.nan), c_st=c_st)
        assert n * 2.0 ** 38 + 2.0 ** 40 < 2.0 ** 52
        ref = alpha * (x.T @ x) + (beta * c0 if beta != 0.0 else 0.0)
        got = run_dgemm(case, mask=2)
        np.testing.assert_array_equal(got[:, n:], R.C_SENTINEL)
        np.testing.assert_array_equal(got[:, :n][low], ref[low])


EPILOGUE_SHAPES = [("dot", (3, 5, 257), 0), ("gemv_rows", (130, 8, 515), 0), ("gemv_cols", (130, 8, 515), 1),
                   ("tiled", (65, 63, 17), 0), ("splitk", (130, 70, 2050), 0)]


@pytest.mark.parametrize("path,shape,ta", EPILOGUE_SHAPES, ids=[e[0] for e in EPILOGUE_SHAPES])
def test_dgemm_real_epilogue(path, shape, ta):
    """alpha = 1/3 (the eigensolver passes 1.0 / e), beta = -1: |got - ref| <= 2 ulp(|alpha s| + |c0|), ref
    in np.longdouble (dla_ref.epilogue_bound derives the bound)."""
    if not R.longdouble_ok():
        pytest.skip("np.longdouble is no wider than float64 here")
    assert R.dgemm_path(*shape, ta) == path
    case = R.gemm_case(77, *shape, alpha=1.0 / 3.0, beta=-1.0, trans_a=ta, trans_b=0)
    got = run_dgemm(case)
    n = case["N"]
    np.testing.assert_array_equal(got[:, n:], R.C_SENTINEL)
    ref, bound = R.epilogue_bound(case)
    err = np.abs(got[:, :n].astype(np.longdouble) - ref).astype(np.float64)
    print("real epilogue %s: max err / bound = %.3f" % (path, float((err / bound).max())))
    assert (err <= bound).all()


# ---------------------------------------------------------------- dot_rows, exact


@pytest.mark.parametrize("rows,n", R.DOT_ROWS_SHAPES)
def test_dot_rows_exact(rows, n):
    N, lib = _lib()

    def run(a_st, b_st, ldb):
        out = np.full(rows, np.nan)
        N.check(lib.gmat_probe_dot_rows(rows, n, N.ptr(a_st), a_st.shape[1], N.ptr(b_st), ldb, N.ptr(out)),
                "gmat_probe_dot_rows")
        return out

    for pad in (0, 3):
        case = R.dot_rows_case(rows * 1000 + n, rows, n, pad)
        a, b = case["a"], case["b"]
        np.testing.assert_array_equal(run(case["a_st"], case["b_st"], n + pad), (a * b).sum(axis=1))
        np.testing.assert_array_equal(run(case["a_st"], None, 0), a.sum(axis=1))
        b0 = np.ascontiguousarray(b[0])
        np.testing.assert_array_equal(run(case["a_st"], b0, 0), a @ b0)


# ---------------------------------------------------------------- cholesky


def run_chol(a_st, n, mode):
    N, lib = _lib()
    a_st = np.ascontiguousarray(a_st)
    out = dict(a_out=np.empty_like(a_st), dinv=np.empty((n, 64)),
               linv=np.empty((n, n)) if mode >= 1 else None, vinv=np.empty((n, n)) if mode >= 2 else None)
    logdet, info = ctypes.c_double(), ctypes.c_int(-1)
    N.check(lib.gmat_probe_cholesky(n, N.ptr(a_st), a_st.shape[1], mode, N.ptr(out["a_out"]), N.ptr(out["dinv"]),
                                    N.ptr(out["linv"]), N.ptr(out["vinv"]), ctypes.byref(logdet), ctypes.byref(info)),
            "gmat_probe_cholesky")
    out["logdet"], out["info"] = logdet.value, info.value
    return out


def padded(a, pad):
    return R.store(np.asarray(a), 0, pad, np.nan)


def check_dinv(dinv, L, n, rtol, atol):
    """Every 64-block: dinv[block rows, :nd] = inv(L_dd); the columns past nd of a partial block exactly 0."""
    for d0 in range(0, n, 64):
        nd = min(64, n - d0)
        blk = np.asarray(L[d0:d0 + nd, d0:d0 + nd])
        want = R.lower_inverse_ld(blk).astype(np.float64)
        np.testing.assert_allclose(dinv[d0:d0 + nd, :nd], want, rtol=rtol, atol=atol)
        np.testing.assert_array_equal(dinv[d0:d0 + nd, nd:], 0.0)
        np.testing.assert_array_equal(np.triu(dinv[d0:d0 + nd, :nd], 1), 0.0)


RTOL, ATOL = 1e-9, 1e-12  # the project's own element tolerances (test_spd_inverse_random)
_mode2 = {}                # n -> mode 2's vinv, for the mode 2 / mode 3 comparison


def _resid_ok(name, n, mode, got, ref):
    lap, floor = ref["lapack"][name], R.resid_floor(n, ref["a"])
    print("chol n=%d mode=%d %s residual: gpu %.3e lapack %.3e ratio %.2f floor %.3e"
          % (n, mode, name, got, lap, got / lap if lap > 0 else 0.0, floor))
    assert got <= max(4.0 * lap, floor), (name, n, mode, got, lap, floor)


@pytest.mark.parametrize("mode,pad", [(0, 0), (0, R.CHOL_PAD), (1, 0), (2, 0), (3, 0), (3, R.CHOL_PAD)])
@pytest.mark.parametrize("n", R.CHOL_SMALL_N)
def test_cholesky_small(n, mode, pad):
    """Every output of cholesky() (mode 0), cholesky_inverse() (1: L^-1; 2: and A^-1) and the dgemm-built
    inverse of the eigensolver (3: chol_lower_inverse, spd_inverse_from_chol) against np.longdouble.

    logdet at rtol 1e-10: rounding gives below 1e-12 (each log L_jj carries about n u cond, n terms), a
    structural slip (a pivot dropped, a padded row counted) at least about 1 / (n max|log L_jj|) ~ 1e-4.

    Residuals max|L L' - A|, max|L^-1 L - I|, max|A^-1 A - I| in np.longdouble: at most 4 x those of
    numpy's float64 LAPACK on the same matrix, or n 2^-52 max|A| if larger (the device multiplies by
    explicit 64 x 64 block inverses where LAPACK solves triangular systems: up to cond(L_kk) <=
    sqrt(cond(A)) <= ~3).  Measured GPU / LAPACK ratios on the MI355X (worst over the modes):
        n      1     2     15    16    17    63    64    65    127   128   129   200   257
        L      1.00  1.00  1.47  1.47  1.80  1.29  1.89  1.73  1.55  1.27  0.98  1.80  1.53
        L^-1   4.28  1.00  1.97  1.67  1.47  1.06  1.73  1.38  1.37  1.73  1.42  2.18  1.64
        A^-1   8.31  1.67  1.03  0.95  1.24  2.19  1.52  2.07  2.31  1.56  1.83  2.22  2.57
    The two n = 1 ratios above 4 are quotients of sub-ulp numbers (1.3e-16 and 2.0e-16 against LAPACK's
    3.0e-17 and 2.4e-17: 1 / L_00 from the reciprocal square root's Newton steps against a correctly
    rounded division) and sit below the floor 2^-52 max|A| = 4.4e-16.  Before the pivot's residual
    correction in factor_invert_block the n = 1 factor missed the bound (L: 7.6e-16, ratio 5.62).
    """
    if not R.longdouble_ok():
        pytest.skip("np.longdouble is no wider than float64 here")
    ref = R.chol_reference(n)
    a = ref["a"]
    got = run_chol(padded(a, pad), n, mode)
    assert got["info"] == 0
    ld = float(ref["logdet"])
    assert abs(got["logdet"] - ld) <= 1e-10 * abs(ld), (got["logdet"], ld)
    check_dinv(got["dinv"], ref["L"], n, RTOL, ATOL)
    if pad:  # the padding is neither read (the outputs are finite) nor written
        assert np.isnan(got["a_out"][:, n:]).all()
    if mode in (0, 3):
        Lg = np.tril(got["a_out"][:, :n])
        np.testing.assert_allclose(Lg, ref["L"].astype(np.float64), rtol=RTOL, atol=ATOL)
        _resid_ok("L", n, mode, R.resid_llt(Lg, a), ref)
    if mode >= 1:
        linv = got["linv"]
        np.testing.assert_array_equal(np.triu(linv, 1), 0.0)  # exactly zero above the diagonal
        np.testing.assert_allclose(linv, ref["linv"].astype(np.float64), rtol=RTOL, atol=ATOL)
        _resid_ok("linv", n, mode, R.resid_inverse(linv, ref["L"]), ref)
    if mode >= 2:
        vinv = got["vinv"]
        np.testing.assert_array_equal(vinv, vinv.T)  # mirrored, so exactly symmetric
        np.testing.assert_allclose(vinv, ref["ainv"].astype(np.float64), rtol=RTOL, atol=ATOL)
        _resid_ok("ainv", n, mode, R.resid_inverse(vinv, a), ref)
        if mode == 2:
            _mode2[n] = vinv
        elif n in _mode2:  # the two inverses agree with each other as well
            np.testing.assert_allclose(vinv, _mode2[n], rtol=RTOL, atol=ATOL)


def _not_pd(p):
    a = R.spd_matrix(200).copy()
    if p is None:
        a[0, 0] = np.nan
    else:
        a[p, p] -= 2.0 * a[p, p]
    return a


@pytest.mark.parametrize("p", [0, 70, 199, None], ids=["p0", "p70", "p199", "nan"])
def test_cholesky_not_positive_definite(p):
    """One failing pivot at n = 200: p = 0 in the block-0 launch (k = -1), p = 70 in a later D task,
    p = 199 in the partial last block; and A[0, 0] = NaN.  info = 1 + the first row of the failing 64-block,
    the call returns, and no output holds an Inf.

    NaN: none may appear.  The failing pivot (non-positive or NaN) is replaced by 1 before the reciprocal
    square root, the column is scaled by that 1, and the stored L_pp is the replaced pivot, exactly 1; so
    the kept factor, dinv, L^-1, A^-1 and logdet are all finite.
    """
    a = _not_pd(p)
    want = 1 if p is None else 64 * (p // 64) + 1
    for mode in (0, 2):
        got = run_chol(a, 200, mode)
        assert got["info"] == want, (mode, got["info"])
        outs = [got["dinv"], np.array(got["logdet"])]
        if mode == 0:  # the kept factor (in mode 2 a is scratch)
            low = np.tril(got["a_out"])
            outs.append(low)
            assert low[p or 0, p or 0] == 1.0
        else:
            outs += [got["linv"], got["vinv"]]
        for o in outs:
            assert not np.isinf(o).any()
            assert not np.isnan(o).any()


def test_spd_inverse_reports_not_positive_definite_and_recovers():
    from gmat_amd import _native as N
    from gmat_amd.gmatrix import spd_inverse
    for p in (0, 70, 199, None):
        with pytest.raises(N.GmatNativeError, match="not positive definite"):
            spd_inverse(_not_pd(p))
    a = R.spd_matrix(200)
    np.testing.assert_allclose(spd_inverse(a), np.linalg.inv(a), rtol=RTOL, atol=ATOL)


@pytest.fixture(scope="module")
def split_ref():
    n = R.CHOL_SPLIT_N
    a = R.spd_matrix(n)
    L = np.linalg.cholesky(a)
    sign, logdet = np.linalg.slogdet(a)
    assert sign == 1.0
    ref = dict(a=a, L=L, linv=np.linalg.inv(L), ainv=np.linalg.inv(a), logdet=logdet)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_cholesky_split_steps(split_ref, mode):
    """n = 3530: 56 blocks, the last of 10 rows -- the smallest block count at which cholesky() without L^-1
    has a two-stream split step (CHOL_SPLIT = 1536 product tasks; chol.hip cholesky_steps, whose task
    counts dla_ref.chol_step_plan copies).  Split steps at this n: mode 0 k = 0, 1; mode 1 k = 0..10;
    mode 2 k = 0..54 (every step with a D task but the block-0 launch).  Against numpy's float64 LAPACK at
    the tolerances test_grm_and_inverse_at_cfg5_n uses for this size class.
    """
    n = R.CHOL_SPLIT_N
    plan = R.chol_step_plan(n, linv=mode >= 1, keep_l=mode == 0, vinv=mode == 2)
    assert any(split for _, _, _, split in plan), "no split step left: CHOL_SPLIT changed?"
    assert any(has_d and not split for _, has_d, _, split in plan)
    ref = split_ref
    got = run_chol(ref["a"], n, mode)
    assert got["info"] == 0
    assert abs(got["logdet"] - ref["logdet"]) <= 1e-10 * abs(ref["logdet"])
    rtol, atol = 1e-8, 1e-10
    for d0 in range(0, n, 64):
        nd = min(64, n - d0)
        np.testing.assert_allclose(got["dinv"][d0:d0 + nd, :nd], np.linalg.inv(ref["L"][d0:d0 + nd, d0:d0 + nd]),
                                   rtol=rtol, atol=atol)
        np.testing.assert_array_equal(got["dinv"][d0:d0 + nd, nd:], 0.0)
    if mode == 0:
        np.testing.assert_allclose(np.tril(got["a_out"]), ref["L"], rtol=rtol, atol=atol)
    else:
        linv = got["linv"]
        assert not np.triu(linv, 1).any()
        np.testing.assert_allclose(linv, ref["linv"], rtol=rtol, atol=atol)
    if mode == 2:
        vinv = got["vinv"]
        np.testing.assert_array_equal(vinv, vinv.T)
        np.testing.assert_allclose(vinv, ref["ainv"], rtol=rtol, atol=atol)
