"""Fixed-effect tests on the GPU (gmat.uvlmm.uvlmm_gwas_add / _dom / _epiAA, gmat_lmm_snp_test /
gmat_lmm_epi_rows) against the reference's direct generalised-least-squares solve.

Expected values: the reference's own recorded output on tests/golden/gwas40 (ref.npz), and the numpy
restatement of its solve (tests/gwas_direct.py, checked against ref.npz in test_uvlmm_gwas_cpu.py) on
the whole tiny panel.  Bars: 1e-8 relative on effects, chi-squares and scale values (the project's
oracle tolerance; measured on an MI355X: add 8e-13, dom 1e-13, epiAA 4e-12 at most), 1e-6 on
p-values where noted; ill-posed tests must be NaN; results must be bit-identical under any blocking.
Shapes: n = 150 (n % 4 == 2, not a multiple of 64), m = 200 / 40.
"""
import os

import numpy as np
import pytest

import gwas_direct as D

pytestmark = pytest.mark.gpu

ADD_COLS = ["chro", "snp_ID", "pos", "allele1", "allele2", "eff_val", "scale_val", "chi_val", "p_val"]
DOM_COLS = ["chro", "snp_ID", "pos", "allele1", "allele2", "eff_val", "chi_val", "p_val"]
EPI_COLS = ["snpi", "snpj", "snp_eff", "p_val"]


@pytest.fixture(scope="module")
def tiny():
    from oracle import gmat_oracle as O
    y, ag, var = D.tiny_inputs()
    snp = O.read_plink(D.TINY)
    counts = np.array([np.sum(snp == g, axis=0) for g in (0, 1, 2)])  # [3][200]
    return {"y": y, "ag": ag, "var": var, "vc": np.array([var[0], var[-1]]), "snp": snp, "counts": counts}


@pytest.fixture(scope="module")
def ref40():
    return np.load(os.path.join(D.GOLD, "gwas40", "ref.npz"))


@pytest.fixture(scope="module")
def epi40(tiny, ref40):
    from gmat.uvlmm import uvlmm_gwas_epiAA
    return uvlmm_gwas_epiAA(tiny["y"], np.ones((150, 1)), [tiny["ag"]], ref40["var_com"], D.GWAS40)


@pytest.fixture(scope="module")
def tiny_p(tiny):
    """P and Py of tiny (X = intercept, one relationship matrix) for the C-ABI tests."""
    from scipy.sparse import identity
    from gmat_amd.uvlmm import projection
    return projection(tiny["y"], np.ones((150, 1)), identity(150, format="csr"), [tiny["ag"]], tiny["vc"])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_add_whole_panel_with_covariate(tiny):
    from gmat.uvlmm import uvlmm_gwas_add
    x = np.column_stack([np.ones(150), np.random.default_rng(3).standard_normal(150)])
    g = [tiny["ag"], tiny["ag"] * tiny["ag"]]
    res = uvlmm_gwas_add(tiny["y"], x, g, tiny["var"], D.TINY)
    assert list(res.columns) == ADD_COLS and res.shape[0] == 200
    assert all(res[c].dtype == np.float64 for c in ADD_COLS[5:])
    # a = g - 2f is identically zero: the two monomorphic SNPs and the all-heterozygous one
    zero = [17, 101, 150]
    assert np.all(np.isnan(res.loc[zero, ADD_COLS[5:]].to_numpy()))
    rest = [j for j in range(200) if j not in zero]
    exp = D.direct_add(tiny["y"], x, g, tiny["var"], tiny["snp"], rest)
    got = res.loc[rest]
    for k, (col, tol) in enumerate([("eff_val", 1e-8), ("scale_val", 1e-8), ("chi_val", 1e-8), ("p_val", 1e-6)]):
        err = np.max(np.abs(got[col].to_numpy() / exp[:, k] - 1))
        print("add %s: max relative gap %.3g" % (col, err))
        np.testing.assert_allclose(got[col].to_numpy(), exp[:, k], rtol=tol, err_msg=col)


def test_dom_matches_the_reference_on_gwas40(tiny, ref40):
    from gmat.uvlmm import uvlmm_gwas_dom
    res = uvlmm_gwas_dom(tiny["y"], np.ones((150, 1)), [tiny["ag"]], ref40["var_com"], D.GWAS40)
    assert list(res.columns) == DOM_COLS and res.shape[0] == 40
    for col, key in (("eff_val", "dom_eff"), ("chi_val", "dom_chi"), ("p_val", "dom_p")):
        print("dom %s: max relative gap %.3g" % (col, np.max(np.abs(res[col].to_numpy() / ref40[key] - 1))))
        np.testing.assert_allclose(res[col].to_numpy(), ref40[key], rtol=1e-8, err_msg=col)


def test_dom_whole_panel_degenerate_and_well_posed(tiny):
    from gmat.uvlmm import uvlmm_gwas_dom
    x = np.ones((150, 1))
    res = uvlmm_gwas_dom(tiny["y"], x, [tiny["ag"]], tiny["vc"], D.TINY)
    stats = res[["eff_val", "chi_val", "p_val"]].to_numpy()
    empty = np.where(tiny["counts"].min(axis=0) == 0)[0]  # fewer than three classes: d is affine in a
    assert {17, 101, 150} <= set(empty.tolist())
    assert np.all(np.isnan(stats[empty])), empty[~np.isnan(stats[empty]).all(axis=1)]
    good = np.where(tiny["counts"].min(axis=0) >= 5)[0]
    assert good.size == 164
    exp = D.direct_dom(tiny["y"], x, [tiny["ag"]], tiny["vc"], tiny["snp"], good)
    np.testing.assert_allclose(stats[good, 0], exp[:, 0], rtol=1e-8)
    np.testing.assert_allclose(stats[good, 1], exp[:, 1], rtol=1e-8)
    np.testing.assert_allclose(stats[good, 2], exp[:, 2], rtol=1e-6)


def test_epi_matches_the_reference_on_gwas40(epi40, ref40):
    assert list(epi40.columns) == EPI_COLS and epi40.shape[0] == 780
    assert [str(epi40[c].dtype) for c in EPI_COLS] == ["int64", "int64", "float64", "float64"]
    np.testing.assert_array_equal(epi40["snpi"].to_numpy(), ref40["epi_snpi"])
    np.testing.assert_array_equal(epi40["snpj"].to_numpy(), ref40["epi_snpj"])
    for col, key, tol in (("snp_eff", "epi_eff", 1e-8), ("p_val", "epi_p", 1e-6)):
        print("epiAA %s: max relative gap %.3g" % (col, np.max(np.abs(epi40[col].to_numpy() / ref40[key] - 1))))
        np.testing.assert_allclose(epi40[col].to_numpy(), ref40[key], rtol=tol, err_msg=col)


def test_epi_p_cut_and_row_list(tiny, ref40, epi40):
    from gmat.uvlmm import uvlmm_gwas_epiAA
    args = (tiny["y"], np.ones((150, 1)), [tiny["ag"]], ref40["var_com"], D.GWAS40)
    cut = uvlmm_gwas_epiAA(*args, p_cut=0.05)
    want = epi40[epi40["p_val"] < 0.05].reset_index(drop=True)
    assert 0 < want.shape[0] < 780
    assert list(cut.columns) == EPI_COLS
    for c in EPI_COLS:
        np.testing.assert_array_equal(_bits(cut[c]) if c in EPI_COLS[2:] else cut[c].to_numpy(),
                                      _bits(want[c]) if c in EPI_COLS[2:] else want[c].to_numpy(), err_msg=c)
    sub = uvlmm_gwas_epiAA(*args, snp_lst_0=[0, 7, 38])
    want = epi40[epi40["snpi"].isin([0, 7, 38])].reset_index(drop=True)
    assert want.shape[0] == 39 + 32 + 1 and sub.shape[0] == want.shape[0]
    np.testing.assert_array_equal(sub[["snpi", "snpj"]].to_numpy(), want[["snpi", "snpj"]].to_numpy())
    for c in EPI_COLS[2:]:
        np.testing.assert_array_equal(_bits(sub[c]), _bits(want[c]), err_msg=c)


@pytest.mark.parametrize("mode", ["add", "dom"])
def test_snp_test_does_not_depend_on_the_chunk(tiny_p, mode):
    """gmat_lmm_snp_test on tiny: passes of 64, 64, 64, 8 SNPs equal the default single pass bit for bit."""
    from gmat_amd import _native as N
    from gmat_amd.uvlmm import uvlmm_gwas as G
    pvp, py = tiny_p
    kind = N.GMAT_GRM_ADD if mode == "add" else N.GMAT_GRM_DOM
    one = G._snp_test(D.TINY, pvp, py, kind, chunk=0)
    cut = G._snp_test(D.TINY, pvp, py, kind, chunk=64)
    assert np.isfinite(one[0]).sum() > 150 and np.isnan(one[0][17])
    for a, b in zip(one[:3], cut[:3]):
        np.testing.assert_array_equal(_bits(a), _bits(b))


def test_epi_rows_do_not_depend_on_the_blocking(tiny_p):
    """gmat_lmm_epi_rows on tiny rows 0..198: block = 64 (64, 64, 64, 7 rows), the default block and the
    concatenation of single-row calls (the last row has one pair) agree bit for bit."""
    from gmat_amd.plink import Geno
    from gmat_amd.remma._scan import EpiPlan
    from gmat_amd.uvlmm import uvlmm_gwas as G
    pvp, py = tiny_p
    rows = np.arange(199)
    with Geno(D.TINY) as geno, EpiPlan(geno, pvp, py) as plan:
        whole = G.epi_rows(plan, rows, block=0)
        cut = G.epi_rows(plan, rows, block=64)
        single = [G.epi_rows(plan, rows[k:k + 1]) for k in range(199)]
    assert whole[0].size == 199 * 200 // 2 and single[-1][0].size == 1
    assert np.isfinite(whole[0]).sum() > 15000
    for c in range(4):
        np.testing.assert_array_equal(_bits(whole[c]), _bits(cut[c]))
        np.testing.assert_array_equal(_bits(whole[c]), _bits(np.concatenate([s[c] for s in single])))
