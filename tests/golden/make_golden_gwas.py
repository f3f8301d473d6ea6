"""Generate tests/golden/gwas40/ by running the REFERENCE's fixed-effect tests (uvlmm_gwas.py).

Container-only, like make_golden.py: the reference is imported through oracle/ref_shim.py and only
data is written.  Re-run with:  python tests/golden/make_golden_gwas.py

  gwas40/plink.{bed,bim,fam}  the first 40 SNPs of tiny/ with at least MIN_CLASS individuals in every
                              genotype class (so that the dominance coding is not an affine function
                              of the additive one and every test is well posed), all 150 individuals
  gwas40/ref.npz              sel (their indices in tiny), var_com, and the reference's own
                              uvlmm_gwas_dom (eff_val, chi_val, p_val) and uvlmm_gwas_epiAA (snpi, snpj,
                              snp_eff, p_val; 780 pairs) with y of tiny.pheno, X = intercept,
                              gmat_lst = [agmat of tiny], var_com = (additive, residual) of tiny_ref.npz
"""
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

from oracle.ref_shim import import_reference  # noqa: E402
from gmat_amd.plink import _codes, _pack, read_bed_body, BED_MAGIC  # noqa: E402

N_SNP = 40
MIN_CLASS = 5


def main():
    tiny = os.path.join(HERE, "tiny", "tiny")
    out = os.path.join(HERE, "gwas40")
    os.makedirs(out, exist_ok=True)
    body, n, m = read_bed_body(tiny)
    codes = _codes(body, n, m)  # PLINK codes 0 / 2 / 3 = dosage 0 / 1 / 2 (1 = missing: none in tiny)
    ok = [j for j in range(m) if min(np.sum(codes[j] == c) for c in (0, 2, 3)) >= MIN_CLASS]
    sel = np.array(ok[:N_SNP], dtype=np.int64)
    assert sel.size == N_SNP, "tiny has only %d SNPs with %d individuals per class" % (len(ok), MIN_CLASS)
    prefix = os.path.join(out, "plink")
    with open(prefix + ".bed", "wb") as f:
        f.write(BED_MAGIC + _pack(codes[sel]).tobytes())
    bim = open(tiny + ".bim").read().splitlines(keepends=True)
    with open(prefix + ".bim", "w") as f:
        f.write("".join(bim[j] for j in sel))
    shutil.copy(tiny + ".fam", prefix + ".fam")

    import_reference()
    from gmat.uvlmm.design_matrix import design_matrix_wemai_multi_gmat
    from gmat.uvlmm.uvlmm_gwas import uvlmm_gwas_dom, uvlmm_gwas_epiAA
    y, xmat, _ = design_matrix_wemai_multi_gmat(tiny + ".pheno", tiny)
    assert y.shape[0] == n and np.all(np.asarray(xmat) == 1.0) and xmat.shape[1] == 1
    tref = np.load(os.path.join(HERE, "tiny", "tiny_ref.npz"))
    var_com = np.array([tref["var"][0], tref["var"][-1]])
    gmat_lst = [tref["agmat"]]
    dom = uvlmm_gwas_dom(y, xmat, gmat_lst, var_com, prefix)
    epi = uvlmm_gwas_epiAA(y, xmat, gmat_lst, var_com, prefix)
    assert dom.shape[0] == N_SNP and epi.shape[0] == N_SNP * (N_SNP - 1) // 2
    np.savez(os.path.join(out, "ref.npz"), sel=sel, var_com=var_com,
             dom_eff=dom["eff_val"].to_numpy(float), dom_chi=dom["chi_val"].to_numpy(float),
             dom_p=dom["p_val"].to_numpy(float),
             epi_snpi=epi["snpi"].to_numpy(np.int64), epi_snpj=epi["snpj"].to_numpy(np.int64),
             epi_eff=epi["snp_eff"].to_numpy(float), epi_p=epi["p_val"].to_numpy(float))
    print("gwas40 written to", out, "SNPs", sel[:8], "...")


if __name__ == "__main__":
    main()
