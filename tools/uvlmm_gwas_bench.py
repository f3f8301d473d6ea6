#!/usr/bin/env python
"""Throughput of the fixed-effect tests (gmat.uvlmm.uvlmm_gwas) on bench.py's synthetic cohort.

Prints one JSON line: SNPs/s of the add and dom tests (gmat_lmm_snp_test) beside the random-effect
remma_add products (gmat_snp_test) on the same panel, and pairs/s of the conditional epiAA test at
p_cut (gmat_lmm_epi_rows, evaluated as uvlmm_gwas_epiAA does it) with its split into the exact pair
evaluation, the three dgemms and the combine kernel, beside the exhaustive-level random-effect scan
(GMAT_SCREEN_NONE) of the same rows.  --rows limits the first SNPs of the epiAA legs (default: the
whole triangle, minutes).

    python tools/uvlmm_gwas_bench.py [--n-id 2000 --n-snp 50000 --rows 2048]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def _time(fn, reps):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-id", type=int, default=2000)
    ap.add_argument("--n-snp", type=int, default=50000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--p-cut", type=float, default=1e-5)
    ap.add_argument("--rows", type=int, default=0, help="first SNPs of the epiAA legs (0: all)")
    ap.add_argument("--reps", type=int, default=3, help="timed calls of the single-SNP tests (best kept)")
    args = ap.parse_args()
    import bench
    from gmat_amd import _native as N
    from gmat_amd.remma._scan import EpiPlan
    from gmat_amd.uvlmm import uvlmm_gwas as G
    n, m = args.n_id, args.n_snp
    var = np.array([0.4, 0.2, 0.4])
    _, g, pvp, py, _, _ = bench.build_inputs(n, m, args.seed, var, 0, 1)
    lib = N.load()
    pvp, py = N.f64(pvp), N.f64(py)
    out = {"cohort": "%d x %d synthetic (bench.py, seed %d), [A, AxA], X = intercept" % (n, m, args.seed)}

    def snp_test(mode):
        res = [np.zeros(m) for _ in range(3)]
        N.check(lib.gmat_lmm_snp_test(g.handle, mode, N.ptr(pvp), N.ptr(py), 0, *[N.ptr(a) for a in res]),
                "gmat_lmm_snp_test")
        return res

    def remma_products():
        res = [np.zeros(m) for _ in range(2)]
        N.check(lib.gmat_snp_test(g.handle, N.GMAT_GRM_ADD, N.ptr(pvp), N.ptr(py), *[N.ptr(a) for a in res]),
                "gmat_snp_test")
        return res

    for name, fn in (("add", lambda: snp_test(N.GMAT_GRM_ADD)), ("dom", lambda: snp_test(N.GMAT_GRM_DOM)),
                     ("remma_add_products", remma_products)):
        fn()  # warm-up (allocations, code load)
        dt, res = _time(fn, args.reps)
        out[name] = {"s": dt, "snps_per_s": m / dt, "nan": int(np.isnan(res[0]).sum())}

    rows = np.arange(min(args.rows, m - 1) if args.rows > 0 else m - 1, dtype=np.int64)
    pairs = float(np.sum(m - 1 - rows))
    with EpiPlan(g, pvp, py) as plan:
        G.epi_rows(plan, rows[:1])  # the plan's one-off setup and the coding, reported apart
        setup = G.lmm_stats()["setup_s"]
        ph = {}
        t0 = time.perf_counter()
        per_row = G.epi_table_rows(plan, rows, args.p_cut, phases=ph)
        dt = time.perf_counter() - t0
        hits = int(sum(v[0].size for v in per_row.values()))
        out["epiAA_conditional"] = {"rows": int(rows.size), "pairs": pairs, "p_cut": args.p_cut, "hits": hits,
                                    "wall_s": dt, "pairs_per_s": pairs / dt, "plan_setup_s": setup,
                                    "pair_eval_s": ph["pair_eval_s"], "dgemm_s": ph["dgemm_s"],
                                    "combine_s": ph["combine_s"], "device_total_s": ph["total_s"]}
        t0 = time.perf_counter()
        hit = plan.scan("AA", rows, args.p_cut, n_slice=N.GMAT_SCREEN_NONE)
        dt = time.perf_counter() - t0
        out["epiAA_random_exhaustive"] = {"wall_s": dt, "pairs_per_s": pairs / dt, "hits": int(hit[0].size),
                                          "refine_s": plan.stats()["refine_s"]}
    g.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
