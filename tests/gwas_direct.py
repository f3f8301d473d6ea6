"""numpy restatement of the reference's fixed-effect tests (uvlmm_gwas.py:12-198), shared by
test_uvlmm_gwas_cpu.py (where it is checked against the reference's recorded output) and
test_gpu_uvlmm_gwas.py (where it is the expected value).  It is the reference's direct form: one
generalised-least-squares solve per SNP or pair with the tested column last,
    [X, C, e]' V^-1 [X, C, e] beta = [X, C, e]' V^-1 y,
snp_eff = beta[-1], snp_var = the inverse's last diagonal entry, chi = snp_eff^2 / snp_var."""
import os

import numpy as np
from scipy.stats import chi2

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TINY = os.path.join(GOLD, "tiny", "tiny")
GWAS40 = os.path.join(GOLD, "gwas40", "plink")


def vinv(gmat_lst, var_com, n):
    v = np.diag([var_com[-1]] * n).astype(float)
    for k, g in enumerate(gmat_lst):
        v += g * var_com[k]
    return np.linalg.inv(v)


def wald(vi, y, cols):
    """(snp_eff, snp_var, chi, p) of the last column of `cols` (n x k)."""
    vx = vi @ cols
    xvx = np.linalg.inv(cols.T @ vx)
    eff = (xvx @ (vx.T @ y))[-1]
    var = xvx[-1, -1]
    chi = eff * eff / var
    return eff, var, chi, chi2.sf(chi, 1)


def codings(snp_mat):
    """Additive g - 2f and dominance [g != 2] g - 2f(1-f) columns of the n x m dosage matrix."""
    freq = np.sum(snp_mat, axis=0) / (2 * snp_mat.shape[0])
    add = snp_mat - 2 * freq
    dom = np.where(snp_mat > 1.5, 0.0, snp_mat) - 2 * freq * (1 - freq)
    return add, dom, freq


def direct_add(y, xmat, gmat_lst, var_com, snp_mat, snps):
    """Rows (eff, scale_val, chi, p) for the listed SNPs."""
    n = y.shape[0]
    vi = vinv(gmat_lst, var_com, n)
    add, _, freq = codings(snp_mat)
    scale = np.sum(2 * freq * (1 - freq))
    out = []
    for j in snps:
        eff, var, chi, p = wald(vi, y, np.column_stack([xmat, add[:, j]]))
        out.append((eff, var_com[0] / (scale * var), chi, p))
    return np.array(out)


def direct_dom(y, xmat, gmat_lst, var_com, snp_mat, snps):
    """Rows (eff, chi, p) for the listed SNPs."""
    vi = vinv(gmat_lst, var_com, y.shape[0])
    add, dom, _ = codings(snp_mat)
    out = []
    for j in snps:
        eff, _, chi, p = wald(vi, y, np.column_stack([xmat, add[:, j], dom[:, j]]))
        out.append((eff, chi, p))
    return np.array(out)


def direct_epi(y, xmat, gmat_lst, var_com, snp_mat, pairs):
    """Rows (eff, p) for the listed pairs (i, j)."""
    vi = vinv(gmat_lst, var_com, y.shape[0])
    add, _, _ = codings(snp_mat)
    out = []
    for i, j in pairs:
        eff, _, _, p = wald(vi, y, np.column_stack([xmat, add[:, i], add[:, j], add[:, i] * add[:, j]]))
        out.append((eff, p))
    return np.array(out)


def tiny_inputs():
    """y (.fam order), the agmat of tiny and its recorded variances."""
    from gmat_amd.uvlmm import design_matrix_wemai_multi_gmat
    y, _, _ = design_matrix_wemai_multi_gmat(TINY + ".pheno", TINY)
    ref = np.load(os.path.join(GOLD, "tiny", "tiny_ref.npz"))
    return y.reshape(-1), ref["agmat"], ref["var"]
