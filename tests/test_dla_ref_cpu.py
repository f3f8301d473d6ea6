"""CPU checks of tests/dla_ref.py: the generators and references that test_gpu_dla.py holds the fp64
GEMM / Cholesky kernels against are themselves right (no GPU, no library)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dla_ref as R  # noqa: E402


def test_float64_product_is_exact_on_the_largest_shapes():
    """numpy's float64 a @ b equals the Python-integer evaluation on 200 sampled entries of the three
    largest shapes (double x double, and each int8 side), so it can serve as the exact reference."""
    rng = np.random.default_rng(5)
    for (M, N, K), kw in ((R.SPLITK_BIG, {}), ((100, 100, 4096), {}), ((130, 70, 2050), {}),
                          ((130, 70, 2050), {"a_i8": True}), ((130, 70, 2050), {"b_i8": True})):
        case = R.gemm_case(11, M, N, K, alpha=2.0, beta=1.0, **kw)
        idx = list(zip(rng.integers(0, M, 200).tolist(), rng.integers(0, N, 200).tolist()))
        exact = R.exact_entries(case, idx)
        for (i, j), e in zip(idx, exact):
            assert abs(e) < 2 ** 52
            assert int(case["s"][i, j]) == e and case["s"][i, j] == float(e)
            full = 2 * e + int(case["c0"][i, j])
            assert abs(full) < 2 ** 52 and int(case["ref"][i, j]) == full


def test_products_exceed_single_precision():
    case = R.gemm_case(3, 16, 16, 4)
    assert np.abs(case["a"]).max() * np.abs(case["b"]).max() > 2.0 ** 36  # a float slip cannot hide
    case = R.gemm_case(3, 16, 16, 64, a_i8=True)
    assert case["a_st"].dtype == np.int8 and case["a_st"].min() == -128 and case["a"].max() == 127


def test_magnitude_bound_fires():
    with pytest.raises(AssertionError, match="magnitude bound"):
        R.gemm_case(1, 4, 4, 8192)
    R.gemm_case(1, 4, 4, R.K_MAX, alpha=2.0, beta=-1.0)  # the largest allowed case passes it


def test_storage_layout_and_padding():
    case = R.gemm_case(2, 5, 7, 9, beta=1.0, trans_a=1, trans_b=0)
    assert case["a_st"].shape == (9, 5 + R.PAD) and case["b_st"].shape == (9, 7 + R.PAD)
    np.testing.assert_array_equal(case["a_st"][:, :5], case["a"].T)
    assert np.isnan(case["a_st"][:, 5:]).all() and np.isnan(case["b_st"][:, 7:]).all()
    np.testing.assert_array_equal(case["c_st"][:, 7:], R.C_SENTINEL)
    np.testing.assert_array_equal(case["c_st"][:, :7], case["c0"])
    case = R.gemm_case(2, 5, 7, 9, beta=0.0, trans_a=0, trans_b=1)
    assert case["a_st"].shape == (5, 9 + R.PAD) and case["b_st"].shape == (7, 9 + R.PAD)
    assert np.isnan(case["c_st"][:, :7]).all() and not np.isnan(case["ref"]).any()


def test_shape_table_reaches_every_path():
    """Each group of the shape table lands on the kernel it is named for (dgemm_path copies launch())."""
    for s in R.DOT_SHAPES:
        assert R.dgemm_path(*s, 0) == "dot" and R.dgemm_path(*s, 1) == "dot"
    for s in R.GEMV_SHAPES:
        assert R.dgemm_path(*s, 0) == "gemv_rows" and R.dgemm_path(*s, 1) == "gemv_cols"
    for s in R.TILED_SHAPES:
        assert R.dgemm_path(*s, 0) == "tiled"
    for s in R.SPLITK_SHAPES + [R.SPLITK_BIG]:
        assert R.dgemm_path(*s, 0) == "splitk"
    assert R.splitk_splits(*R.SPLITK_BIG[:2]) == 3
    assert sorted({R.dgemm_path(*s, t) for s in R.INT8_SHAPES for t in (0, 1)}) == \
        ["dot", "gemv_cols", "gemv_rows", "splitk", "tiled"]
    for n in R.MASK_SIZES:
        assert R.dgemm_path(n, n, n, 0, mask=1) == "tiled"
    assert all(max(s) <= R.K_MAX for g in (R.DOT_SHAPES, R.GEMV_SHAPES, R.TILED_SHAPES, R.SPLITK_SHAPES) for s in g)


def test_spd_matrices_are_well_conditioned():
    for n in R.CHOL_SMALL_N:
        a = R.spd_matrix(n)
        np.testing.assert_array_equal(a, a.T)
        assert np.linalg.cond(a) <= 10.0, n


def test_longdouble_reference_matches_lapack():
    if not R.longdouble_ok():
        pytest.skip("np.longdouble is no wider than float64 here")
    for n in R.CHOL_SMALL_N:
        ref = R.chol_reference(n)
        a = ref["a"]
        np.testing.assert_allclose(ref["L"].astype(np.float64), np.linalg.cholesky(a), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(ref["linv"].astype(np.float64), np.linalg.inv(np.linalg.cholesky(a)), rtol=1e-12,
                                   atol=1e-12)
        np.testing.assert_allclose(ref["ainv"].astype(np.float64), np.linalg.inv(a), rtol=1e-12, atol=1e-12)
        sign, ld = np.linalg.slogdet(a)
        assert sign == 1.0 and abs(float(ref["logdet"]) - ld) <= 1e-12 * max(1.0, abs(ld))
        assert np.all(np.triu(ref["L"], 1) == 0) and np.all(np.triu(ref["linv"], 1) == 0)
        # the reference's own residuals sit far below float64 rounding
        assert R.resid_llt(ref["L"], a) < 1e-17 and R.resid_inverse(ref["ainv"], a) < 1e-16
        assert all(v < 1e-13 for v in ref["lapack"].values())


def test_chol_step_plan_split_steps():
    """At n = 3530 (56 blocks) every mode has a split step and an unsplit step with a D task; one block
    fewer and cholesky() alone has no split step."""
    for linv, keep_l, vinv in ((False, True, False), (True, False, False), (True, False, True)):
        plan = R.chol_step_plan(R.CHOL_SPLIT_N, linv, keep_l, vinv)
        assert any(split for _, _, _, split in plan)
        assert any(has_d and not split for _, has_d, _, split in plan)
    assert not any(split for _, _, _, split in R.chol_step_plan(55 * 64, False, True, False))
    assert any(split for _, _, _, split in R.chol_step_plan(55 * 64, True, False, False))
    assert not any(split for _, _, _, split in R.chol_step_plan(54 * 64, True, False, True))
