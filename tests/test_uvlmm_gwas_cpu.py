"""CPU checks of the fixed-effect tests (gmat.uvlmm.uvlmm_gwas): the public names resolve, the
expected-value code of the GPU tests (tests/gwas_direct.py) reproduces the reference's recorded
output (tests/golden/gwas40/ref.npz, written by make_golden_gwas.py), and bad calls are refused with
ValueError before the device is touched."""
import os

import numpy as np
import pytest

import gwas_direct as D


@pytest.fixture()
def no_device(monkeypatch):
    """Any use of the native library fails the test."""
    from gmat_amd import _native as N

    def boom(*a, **k):
        raise AssertionError("device work before the argument checks")
    monkeypatch.setattr(N, "load", boom)
    monkeypatch.setattr(N, "ensure_device", boom)


def test_public_names_resolve():
    from gmat.uvlmm import uvlmm_gwas_add, uvlmm_gwas_dom, uvlmm_gwas_epiAA
    import gmat.uvlmm.uvlmm_gwas as mod
    import gmat_amd.uvlmm.uvlmm_gwas as real
    assert mod is real
    assert (mod.uvlmm_gwas_add, mod.uvlmm_gwas_dom, mod.uvlmm_gwas_epiAA) == (uvlmm_gwas_add, uvlmm_gwas_dom,
                                                                             uvlmm_gwas_epiAA)
    assert not hasattr(mod, "uvlmm_gwas_add_eigen") and not hasattr(mod, "uvlmm_gwas_dom_eigen")


def test_direct_solve_reproduces_the_reference():
    """The in-test restatement against the reference's own uvlmm_gwas_dom / uvlmm_gwas_epiAA on gwas40
    (all 40 SNPs, all 780 pairs), 1e-8 relative."""
    from oracle import gmat_oracle as O
    ref = np.load(os.path.join(D.GOLD, "gwas40", "ref.npz"))
    y, ag, _ = D.tiny_inputs()
    snp = O.read_plink(D.GWAS40)
    assert snp.shape == (150, 40)
    x = np.ones((150, 1))
    dom = D.direct_dom(y, x, [ag], ref["var_com"], snp, range(40))
    np.testing.assert_allclose(dom[:, 0], ref["dom_eff"], rtol=1e-8)
    np.testing.assert_allclose(dom[:, 1], ref["dom_chi"], rtol=1e-8)
    np.testing.assert_allclose(dom[:, 2], ref["dom_p"], rtol=1e-8)
    pairs = np.column_stack([ref["epi_snpi"], ref["epi_snpj"]])
    assert pairs.shape == (780, 2)
    np.testing.assert_array_equal(pairs, [(i, j) for i in range(39) for j in range(i + 1, 40)])
    epi = D.direct_epi(y, x, [ag], ref["var_com"], snp, pairs)
    np.testing.assert_allclose(epi[:, 0], ref["epi_eff"], rtol=1e-8)
    np.testing.assert_allclose(epi[:, 1], ref["epi_p"], rtol=1e-8)
    # the fixture's panel is what its readme says: SNPs of tiny with >= 5 individuals per genotype class
    tiny = O.read_plink(D.TINY)
    np.testing.assert_array_equal(tiny[:, ref["sel"]], snp)
    assert min(np.sum(snp == g, axis=0).min() for g in (0, 1, 2)) >= 5


def test_oversized_table_is_refused_before_device_work(tmp_path, no_device):
    """20,001 SNPs = 200,010,000 pairs > 2e8 rows without p_cut."""
    from gmat.uvlmm import uvlmm_gwas_epiAA
    prefix = str(tmp_path / "big")
    n, m = 4, 20001
    with open(prefix + ".bim", "w") as f:
        f.write("".join("1 s%d 0 %d A G\n" % (j, j + 1) for j in range(m)))
    with open(prefix + ".fam", "w") as f:
        f.write("".join("F I%d 0 0 0 -9\n" % k for k in range(n)))
    args = (np.zeros(n), np.ones((n, 1)), [np.eye(n)], [1.0, 1.0], prefix)
    with pytest.raises(ValueError, match="200010000 rows"):
        uvlmm_gwas_epiAA(*args)
    # the same call restricted to a few rows, or with p_cut, passes the check (and reaches the device)
    with pytest.raises(AssertionError, match="device work"):
        uvlmm_gwas_epiAA(*args, snp_lst_0=[0, 5])
    with pytest.raises(AssertionError, match="device work"):
        uvlmm_gwas_epiAA(*args, p_cut=1e-5)
    with pytest.raises(ValueError, match="out of range"):
        uvlmm_gwas_epiAA(*args, snp_lst_0=[m - 1])


@pytest.mark.parametrize("name", ["uvlmm_gwas_add", "uvlmm_gwas_dom", "uvlmm_gwas_epiAA"])
def test_length_mismatch_is_refused_before_device_work(name, no_device):
    import gmat.uvlmm as U
    fn = getattr(U, name)
    y, ag, var = D.tiny_inputs()
    vc = [var[0], var[-1]]
    x = np.ones((150, 1))
    with pytest.raises(ValueError, match="149 records"):       # y shorter than the .fam
        fn(y[:149], x[:149], [ag[:149, :149]], vc, D.TINY)
    with pytest.raises(ValueError, match="xmat"):              # X rows
        fn(y, np.ones(149), [ag], vc, D.TINY)
    with pytest.raises(ValueError, match="relationship matrix"):
        fn(y, x, [ag[:149, :149]], vc, D.TINY)
    with pytest.raises(ValueError, match="var_com"):
        fn(y, x, [ag], var, D.TINY)
