"""Fixed-effect single-marker tests on the GPU -- drop-in for gmat.uvlmm.uvlmm_gwas
(uvlmm_gwas.py:12-198).

The reference fits, per SNP or pair, the fixed effects plus the tested column(s) by one dense
generalised-least-squares solve against V^-1 (O(n^2) each) and reports the Wald test of the last
coefficient.  Here P = V^-1 - V^-1 X (X'V^-1 X)^-1 X'V^-1 and Py come from the device projection
once, and the same statistics follow from quadratic forms in P by a Schur complement
(gmat_lmm_snp_test / gmat_lmm_epi_rows, gmat_amd/csrc/lmm.hip):

    M = C'PC, c = C'Pe, r = C'Py;  snp_var = 1 / (e'Pe - c'M^-1 c),
    snp_eff = (e'Py - c'M^-1 r) snp_var,  chi = snp_eff^2 / snp_var,  p = chi2.sf(chi, 1)

with the tested column e and the conditioning columns C = [] (add), [a] (dom), [a_i, a_j] (epiAA).
Tests the data cannot answer (a monomorphic SNP, a SNP with two genotype classes in the dominance
test, collinear SNPs of a pair) are NaN; the reference returns rounding noise or raises there.

Records equal individuals here (no Z): y has the .fam length.  The reference's empty
uvlmm_gwas_add_eigen / uvlmm_gwas_dom_eigen stubs are not provided.
"""
import logging

import numpy as np
import pandas as pd
from scipy.sparse import identity
from scipy.stats import chi2

from .. import _native as N
from .. import dist
from ..plink import Geno, count_lines
from ..remma._scan import EpiPlan, resolve_rows
from .uvlmm_varcom import projection

MAX_ROWS = 2 * 10 ** 8   # uvlmm_gwas_epiAA without p_cut refuses to build a larger table
PAIRS_PER_CALL = 1 << 23  # pairs per device call of uvlmm_gwas_epiAA (bounds the host buffers)


def _check_inputs(y, xmat, gmat_lst, var_com, bed_file):
    """The reference's reshapes (uvlmm_gwas.py:23-28) with its silent assumptions checked: every
    mismatch is a ValueError, raised before any device work."""
    y = np.asarray(y, dtype=float).reshape(-1)
    n = y.shape[0]
    xmat = np.asarray(xmat, dtype=float)
    if xmat.size == 0 or xmat.size % n:
        raise ValueError("xmat has %d values, not a multiple of the %d phenotypes" % (xmat.size, n))
    xmat = xmat.reshape(n, -1)
    mats = [np.asarray(g) for g in gmat_lst]
    for g in mats:
        if g.shape != (n, n):
            raise ValueError("relationship matrix of shape %s, expected %s" % (g.shape, (n, n)))
    var_com = np.asarray(var_com, dtype=float).reshape(-1)
    if var_com.size != len(mats) + 1:
        raise ValueError("var_com has %d values, expected %d (one per relationship matrix and the residual)"
                         % (var_com.size, len(mats) + 1))
    n_fam = count_lines(bed_file + ".fam")
    if n_fam != n:
        raise ValueError("y has %d records, the .fam has %d individuals (records must equal individuals)" % (n, n_fam))
    return y, xmat, mats, var_com


def _projection(y, xmat, mats, var_com):
    logging.info("Calculate the phenotypic covariance matrix and inversion")
    return projection(y, xmat, identity(y.shape[0], format="csr"), mats, var_com)


def _snp_test(bed_file, pvp, py, mode, chunk=0):
    """(eff, var, chi, freq) of every SNP of the imputed panel (gmat_lmm_snp_test)."""
    with Geno(bed_file) as geno:
        out = [np.zeros(geno.m) for _ in range(3)]
        N.check(N.load().gmat_lmm_snp_test(geno.handle, mode, N.ptr(N.f64(pvp)), N.ptr(N.f64(py)), int(chunk),
                                           *[N.ptr(a) for a in out]), "gmat_lmm_snp_test")
        freq = geno.freq()
    return out[0], out[1], out[2], freq


def _snp_table(bed_file):
    snp_info = pd.read_csv(bed_file + ".bim", sep=r"\s+", header=None)
    res_df = snp_info.iloc[:, [0, 1, 3, 4, 5]].copy()
    res_df.columns = ["chro", "snp_ID", "pos", "allele1", "allele2"]
    return res_df


@dist.on_root
def uvlmm_gwas_add(y, xmat, gmat_lst, var_com, bed_file):
    """Additive test (uvlmm_gwas.py:12-65): the SNP's centred dosage as a fixed covariate.  Returns
    'chro snp_ID pos allele1 allele2 eff_val scale_val chi_val p_val'; var_com[0] is the additive
    variance (scale_val = var_com[0] / (sum 2f(1-f) * snp_var))."""
    y, xmat, mats, var_com = _check_inputs(y, xmat, gmat_lst, var_com, bed_file)
    pvp, py = _projection(y, xmat, mats, var_com)
    eff, var, chi, freq = _snp_test(bed_file, pvp, py, N.GMAT_GRM_ADD)
    scale = np.sum(2 * freq * (1 - freq))
    res_df = _snp_table(bed_file)
    res_df.loc[:, "eff_val"] = eff
    res_df.loc[:, "scale_val"] = var_com[0] / (scale * var)
    res_df.loc[:, "chi_val"] = chi
    res_df.loc[:, "p_val"] = chi2.sf(chi, 1)
    return res_df


@dist.on_root
def uvlmm_gwas_dom(y, xmat, gmat_lst, var_com, bed_file):
    """Dominance test adjusted for the SNP's additive effect (uvlmm_gwas.py:80-131).  Returns
    'chro snp_ID pos allele1 allele2 eff_val chi_val p_val'."""
    y, xmat, mats, var_com = _check_inputs(y, xmat, gmat_lst, var_com, bed_file)
    pvp, py = _projection(y, xmat, mats, var_com)
    eff, _, chi, _ = _snp_test(bed_file, pvp, py, N.GMAT_GRM_DOM)
    res_df = _snp_table(bed_file)
    res_df.loc[:, "eff_val"] = eff
    res_df.loc[:, "chi_val"] = chi
    res_df.loc[:, "p_val"] = chi2.sf(chi, 1)
    return res_df


def epi_rows(plan, rows, block=0):
    """(eff, var, chi, p) of gmat_lmm_epi_rows for the first SNPs `rows` (strictly increasing) of an
    EpiPlan: row i's pairs (i, i+1 .. m-1) contiguously."""
    rows = N.i64(rows)
    k = int(np.sum(plan.geno.m - 1 - rows))
    out = [np.zeros(k) for _ in range(4)]
    N.check(plan._lib.gmat_lmm_epi_rows(plan._h, N.ptr(rows), rows.size, int(block), *[N.ptr(a) for a in out]),
            "gmat_lmm_epi_rows")
    return tuple(out)


def lmm_stats():
    """Phases of the last gmat_lmm_epi_rows call of this process (gmat_lmm_stats)."""
    s = np.zeros(8)
    N.check(N.load().gmat_lmm_stats(N.ptr(s)), "gmat_lmm_stats")
    return dict(zip(("pairs", "setup_s", "pair_eval_s", "dgemm_s", "combine_s", "total_s"), s.tolist()))


def epi_table_rows(plan, uniq, p_cut=None, phases=None):
    """{i: (j, snp_eff, p_val)} for the first SNPs `uniq` (strictly increasing): the pairs of row i
    (those with p_val < p_cut when given), evaluated PAIRS_PER_CALL pairs (whole rows) at a time so
    that the host buffers stay bounded.  phases (a dict) accumulates lmm_stats() over the calls."""
    m = plan.geno.m
    per_row = {}
    r0 = 0
    while r0 < uniq.size:
        r1, np_call = r0, 0
        while r1 < uniq.size and (r1 == r0 or np_call + m - 1 - uniq[r1] <= PAIRS_PER_CALL):
            np_call += m - 1 - uniq[r1]
            r1 += 1
        eff, _, _, p = epi_rows(plan, uniq[r0:r1])
        if phases is not None:
            for k, v in lmm_stats().items():
                phases[k] = phases.get(k, 0.0) + v
        cuts = np.cumsum(m - 1 - uniq[r0:r1])[:-1]
        for i, e_i, p_i in zip(uniq[r0:r1].tolist(), np.split(eff, cuts), np.split(p, cuts)):
            j = np.arange(i + 1, m, dtype=np.int64)
            if p_cut is not None:
                keep = p_i < p_cut
                j, e_i, p_i = j[keep], e_i[keep], p_i[keep]
            per_row[i] = (j, e_i.copy(), p_i.copy())
        r0 = r1
    return per_row


@dist.on_root
def uvlmm_gwas_epiAA(y, xmat, gmat_lst, var_com, bed_file, *, snp_lst_0=None, p_cut=None):
    """Additive-by-additive interaction adjusted for both SNPs' additive effects (uvlmm_gwas.py:145-198).
    Returns 'snpi snpj snp_eff p_val' for every pair j > i, rows in order.  Extensions (defaults = the
    reference): snp_lst_0, the first SNPs to test (the rules of remma_epiAA: list order, range checked);
    p_cut, keep only p_val < p_cut (evaluated block by block: memory stays bounded).  Without p_cut a
    call that would return more than 2e8 rows is refused."""
    y, xmat, mats, var_com = _check_inputs(y, xmat, gmat_lst, var_com, bed_file)
    m = count_lines(bed_file + ".bim")
    rows = resolve_rows("AA", m, snp_lst_0)
    n_out = int(np.sum(m - 1 - rows))
    if p_cut is None and n_out > MAX_ROWS:
        raise ValueError("uvlmm_gwas_epiAA would return %d rows (more than %d): pass p_cut to keep the "
                         "significant pairs only, or test fewer first SNPs (snp_lst_0)" % (n_out, MAX_ROWS))
    pvp, py = _projection(y, xmat, mats, var_com)
    with Geno(bed_file) as geno, EpiPlan(geno, pvp, py) as plan:
        per_row = epi_table_rows(plan, np.unique(rows), p_cut)
    order = rows.tolist()
    snpi = [np.full(per_row[i][0].size, i, dtype=np.int64) for i in order]

    def cat(parts, dt):
        return np.concatenate(parts) if parts else np.zeros(0, dt)

    return pd.DataFrame({
        "snpi": cat(snpi, np.int64),
        "snpj": cat([per_row[i][0] for i in order], np.int64),
        "snp_eff": cat([per_row[i][1] for i in order], float),
        "p_val": cat([per_row[i][2] for i in order], float),
    })
