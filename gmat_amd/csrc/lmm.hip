// Fixed-effect single-marker and pair tests of a linear mixed model (the reference's
// uvlmm_gwas_add / uvlmm_gwas_dom / uvlmm_gwas_epiAA, uvlmm_gwas.py:12-198): the tested column e is a
// fixed covariate fitted together with the other fixed effects and with conditioning columns C
// (none for add, the SNP's additive coding for dom, both SNPs' additive codings for epiAA), and the
// Wald statistic of its coefficient is returned.  The reference solves one dense (p + k + 1) system
// against V^-1 per SNP or pair; with P = V^-1 - V^-1 X (X'V^-1 X)^-1 X'V^-1 (the other fixed effects
// projected out) the same numbers are a Schur complement,
//     M = C'PC, c = C'Pe, r = C'Py,   den = e'Pe - c'M^-1 c,   num = e'Py - c'M^-1 r,
//     snp_var = 1 / den,  snp_eff = num / den,  chi = num^2 / den,  p = chi2.sf(chi, 1),
// so every quantity is a quadratic form in P the library already evaluates.
// Ill-posed tests get NaN instead of rounding noise: den <= LMM_TINY e'Pe (e in the span of C, e.g. a SNP
// with two genotype classes in the dom test), det M <= LMM_TINY M11 M22 (epiAA: two collinear SNPs) or a
// zero pivot a'Pa (a monomorphic SNP).
//
//  gmat_lmm_snp_test   add / dom, every SNP of the panel.  Per chunk: coding rows A (and D) from the packed
//                      panel (eff_x_kernel), A P (and D P) on the fp64 MFMA dgemm, then lmm_snp_kernel, one
//                      wave per SNP: the row dots a'Pa, a'Py (d'Pd, a'Pd, d'Py), the Schur step and the
//                      degenerate test.
//  gmat_lmm_epi_rows   epiAA, every pair (i, j > i) of the listed first SNPs.  Once per plan: S (centred
//                      codes, fp64), Y = S P, W = S o Y, d = diag(S P S'), q = S Py.  Per block of rows:
//                      e'Py and e'Pe from the plan's exact pair evaluation (refine(), the one behind
//                      gmat_epi_pairs) on a device-built pair list, three dgemms
//                      S_rows Y' = a_i'Pa_j, W_rows S' = e'Pa_i, S_rows W' = e'Pa_j, and lmm_epi_kernel: the
//                      2 x 2 Schur step, the degenerate test and the p-value per pair.
//
// A number never depends on the chunk / block size or on the rows it was grouped with: the reductions
// run in a fixed order per SNP, and every product is issued as dgemms of exactly LMM_GB rows (dgemm
// picks its kernel and its split of the k range from the shape; with the shape fixed, an output
// element is the same sum wherever its row sits).
#include <algorithm>
#include <cmath>

#include "epi.h"

namespace {
using namespace gmat;
using namespace gmat::epi;

constexpr double LMM_TINY = 1e-10;  // degenerate threshold (~1e3 x the n eps rounding of the fp64 sums)
constexpr int64_t LMM_GB = 128;     // rows per dgemm call
constexpr int64_t LMM_BLOCK = 256;  // default first SNPs per pass of gmat_lmm_epi_rows

__device__ __forceinline__ double wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// One wave per SNP of the chunk (4 per workgroup): the lane partials run over k = lane, lane + 64, ...,
// then the xor butterfly -- a fixed order.  a / ap: the additive rows and their product with P (nc x n);
// d / dp: the dominance rows (dom test) or null.
__global__ __launch_bounds__(256) void lmm_snp_kernel(int64_t nc, int64_t n, const double *__restrict__ a,
                                                      const double *__restrict__ ap, const double *__restrict__ d,
                                                      const double *__restrict__ dp, const double *__restrict__ py,
                                                      double *__restrict__ eff, double *__restrict__ var,
                                                      double *__restrict__ chi) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= nc) return;
  const double *ar = a + r * n, *apr = ap + r * n;
  double aPa = 0.0, aPy = 0.0, dPd = 0.0, aPd = 0.0, dPy = 0.0;
  if (d) {
    const double *dr = d + r * n, *dpr = dp + r * n;
    for (int64_t k = lane; k < n; k += 64) {
      const double av = ar[k], dv = dr[k], pk = py[k], dpv = dpr[k];
      aPa += av * apr[k];
      aPy += av * pk;
      dPd += dv * dpv;
      aPd += av * dpv;
      dPy += dv * pk;
    }
    dPd = wave_sum(dPd);
    aPd = wave_sum(aPd);
    dPy = wave_sum(dPy);
  } else {
    for (int64_t k = lane; k < n; k += 64) {
      const double av = ar[k];
      aPa += av * apr[k];
      aPy += av * py[k];
    }
  }
  aPa = wave_sum(aPa);
  aPy = wave_sum(aPy);
  if (lane) return;
  double den, num, epe;
  bool ok = aPa > 0.0;  // the pivot (add: the statistic's own denominator)
  if (d) {
    den = dPd - aPd * aPd / aPa;
    num = dPy - aPd * aPy / aPa;
    epe = dPd;
  } else {
    den = aPa;
    num = aPy;
    epe = aPa;
  }
  ok = ok && den > LMM_TINY * epe;
  const double nan = __builtin_nan("");
  eff[r] = ok ? num / den : nan;
  var[r] = ok ? 1.0 / den : nan;
  chi[r] = ok ? num * num / den : nan;
}

// S[i][q] = dosage - 2 f_i for the real individuals (storage order), 0 in the padding; one workgroup per SNP
__global__ void lmm_centre_kernel(int64_t n, int64_t n_pad, const int8_t *__restrict__ dose,
                                  const double *__restrict__ off, double *__restrict__ S) {
  const int64_t i = blockIdx.x;
  const double c = off[i];
  for (int64_t q = threadIdx.x; q < n_pad; q += blockDim.x) {
    const int64_t nat = (q & ~31LL) + perm_nat((int)(q & 31));
    S[i * n_pad + q] = nat < n ? (double)dose[i * n_pad + q] - c : 0.0;
  }
}

// W = S o Y, d[i] = sum_q W[i][q] = a_i'Pa_i, qv[i] = S[i] . py = a_i'Py; one wave per SNP, fixed order
__global__ __launch_bounds__(256) void lmm_rowsum_kernel(int64_t m, int64_t n_pad, const double *__restrict__ S,
                                                         const double *__restrict__ Y, const double *__restrict__ py,
                                                         double *__restrict__ W, double *__restrict__ d,
                                                         double *__restrict__ qv) {
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= m) return;
  double sd = 0.0, sq = 0.0;
  for (int64_t k = lane; k < n_pad; k += 64) {
    const double s = S[i * n_pad + k], w = s * Y[i * n_pad + k];
    W[i * n_pad + k] = w;
    sd += w;
    sq += s * py[k];
  }
  sd = wave_sum(sd);
  sq = wave_sum(sq);
  if (lane == 0) {
    d[i] = sd;
    qv[i] = sq;
  }
}

// rows[r] of S and W gathered into the block's contiguous operands (blockIdx.x = block row)
__global__ void lmm_gather_kernel(int64_t n_pad, const int64_t *__restrict__ rows, const double *__restrict__ S,
                                  const double *__restrict__ W, double *__restrict__ Sr, double *__restrict__ Wr) {
  const int64_t r = blockIdx.x, i = rows[r];
  for (int64_t q = threadIdx.x; q < n_pad; q += blockDim.x) {
    Sr[r * n_pad + q] = S[i * n_pad + q];
    Wr[r * n_pad + q] = W[i * n_pad + q];
  }
}

// The pairs (i = rows[r], j > i) of block row r = blockIdx.y sit at offs[r] + (j - i - 1) of the pair
// list (all_pairs_kernel's layout).  On entry eff = e'Py and var = e'Pe of the exact pair evaluation;
// on exit the conditional statistics.  p = chi2.sf(chi, 1) as pvalue_kernel computes it.
__global__ void lmm_epi_kernel(int64_t m, const int64_t *__restrict__ rows, const int64_t *__restrict__ offs,
                               const double *__restrict__ c_aa, const double *__restrict__ c_ei,
                               const double *__restrict__ c_ej, const double *__restrict__ d,
                               const double *__restrict__ qv, double *__restrict__ eff, double *__restrict__ var,
                               double *__restrict__ chi, double *__restrict__ p) {
  const int64_t r = blockIdx.y, i = rows[r], j0 = i + 1, cnt = m - j0, base = offs[r];
  const double m11 = d[i], r1 = qv[i];
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < cnt; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = j0 + t, o = base + t, g = r * m + j;
    const double m22 = d[j], m12 = c_aa[g], c1 = c_ei[g], c2 = c_ej[g], r2 = qv[j];
    const double epy = eff[o], epe = var[o];
    const double det = m11 * m22 - m12 * m12;
    const double u1 = m22 * c1 - m12 * c2, u2 = m11 * c2 - m12 * c1;  // det M^-1 c
    const double den = epe - (c1 * u1 + c2 * u2) / det;
    const double num = epy - (r1 * u1 + r2 * u2) / det;
    const bool ok = det > LMM_TINY * m11 * m22 && den > LMM_TINY * epe;  // false on NaN (a monomorphic SNP)
    const double nan = __builtin_nan("");
    const double c = ok ? num * num / den : nan;
    eff[o] = ok ? num / den : nan;
    var[o] = ok ? 1.0 / den : nan;
    chi[o] = c;
    p[o] = ok ? ((c < 0.0) ? 1.0 : erfc(sqrt(0.5 * c))) : nan;
  }
}

// C (rows x N, ldc) = A (rows x K, contiguous rows) * op(B) as dgemms of exactly LMM_GB rows: A and C
// hold round_up(rows, LMM_GB) rows (the padding rows' products are never read)
int gemm_rows(hipStream_t s, int64_t rows, int64_t N, int64_t K, const double *A, DView B, double *C, int64_t ldc) {
  for (int64_t r0 = 0; r0 < rows; r0 += LMM_GB)
    GMAT_TRY(dgemm(s, LMM_GB, N, K, 1.0, DView{A + r0 * K, K, 0}, B, 0.0, C + r0 * ldc, ldc));
  return GMAT_OK;
}

double g_lmm_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};

int lmm_setup(gmat_epi *e) {
  auto &L = e->lmm;
  if (L.ready) return GMAT_OK;
  const int64_t m = e->m, n_pad = e->n_pad;
  const size_t vb = (size_t)m * n_pad * sizeof(double);
  int rc = GMAT_OK;
  if ((rc = L.S.alloc(vb)) || (rc = L.Y.alloc(vb)) || (rc = L.W.alloc(vb)) || (rc = L.d.alloc(m * sizeof(double))) ||
      (rc = L.q.alloc(m * sizeof(double)))) {
    for (DBuf *b : {&L.S, &L.Y, &L.W, &L.d, &L.q}) b->release();
    return rc;
  }
  const hipStream_t s = e->s;
  hipLaunchKernelGGL(lmm_centre_kernel, dim3((unsigned)m), dim3(256), 0, s, e->n, n_pad, e->g->dose_ptr(),
                     e->code[0].off.as<double>(), L.S.as<double>());
  GMAT_HIP(hipGetLastError());
  GMAT_TRY(dgemm(s, m, n_pad, n_pad, 1.0, DView{L.S.as<double>(), n_pad, 0}, DView{e->Ps.as<double>(), n_pad, 0}, 0.0,
                 L.Y.as<double>(), n_pad));
  hipLaunchKernelGGL(lmm_rowsum_kernel, dim3((unsigned)cdiv(m, 4)), dim3(256), 0, s, m, n_pad, L.S.as<double>(),
                     L.Y.as<double>(), e->py.as<double>(), L.W.as<double>(), L.d.as<double>(), L.q.as<double>());
  GMAT_HIP(hipGetLastError());
  GMAT_HIP(hipStreamSynchronize(s));
  L.ready = true;
  return GMAT_OK;
}

}  // namespace

extern "C" int gmat_lmm_snp_test(gmat_geno *g, int mode, const double *p, const double *py, int64_t chunk, double *eff,
                                 double *var, double *chi) {
  GMAT_CHECK(g && p && py && eff && var && chi, GMAT_E_ARG, "gmat_lmm_snp_test: bad arguments");
  GMAT_CHECK(mode == GMAT_GRM_ADD || mode == GMAT_GRM_DOM, GMAT_E_ARG, "gmat_lmm_snp_test: unknown mode %d", mode);
  GMAT_CHECK(chunk >= 0, GMAT_E_ARG, "gmat_lmm_snp_test: negative chunk");
  GMAT_CHECK(g->total_missing == 0, GMAT_E_ARG, "gmat_lmm_snp_test: panel has %lld missing genotypes (impute first)",
             (long long)g->total_missing);
  const int64_t n = g->n, m = g->m;
  const bool dom = mode == GMAT_GRM_DOM;
  std::vector<double> c(2 * m);
  for (int64_t j = 0; j < m; ++j) {
    const double freq = (double)g->sum_dose[j] / (double)(2 * n);
    c[j] = 2 * freq;
    c[m + j] = 2 * freq * (1 - freq);
  }
  const int64_t C = std::min(m, chunk > 0 ? chunk : snp_test_chunk(n, m)), Cp = round_up(C, LMM_GB);
  DBuf dc, dp, dpy, a, ap, d, dpp, o;
  GMAT_TRY(dc.alloc(2 * m * sizeof(double)));
  GMAT_TRY(dp.alloc(n * n * sizeof(double)));
  GMAT_TRY(dpy.alloc(n * sizeof(double)));
  GMAT_TRY(a.alloc(Cp * n * sizeof(double)));
  GMAT_TRY(ap.alloc(Cp * n * sizeof(double)));
  if (dom) {
    GMAT_TRY(d.alloc(Cp * n * sizeof(double)));
    GMAT_TRY(dpp.alloc(Cp * n * sizeof(double)));
  }
  GMAT_TRY(o.alloc(3 * m * sizeof(double)));
  // the padding rows of a short pass are multiplied too (gemm_rows): keep them finite
  GMAT_HIP(hipMemset(a.p, 0, Cp * n * sizeof(double)));
  if (dom) GMAT_HIP(hipMemset(d.p, 0, Cp * n * sizeof(double)));
  GMAT_HIP(hipMemcpy(dc.p, c.data(), 2 * m * sizeof(double), hipMemcpyHostToDevice));
  GMAT_HIP(hipMemcpy(dp.p, p, n * n * sizeof(double), hipMemcpyHostToDevice));
  GMAT_HIP(hipMemcpy(dpy.p, py, n * sizeof(double), hipMemcpyHostToDevice));
  double *oe = o.as<double>(), *ov = oe + m, *oc = ov + m;
  const DView P{dp.as<double>(), n, 0};
  for (int64_t j0 = 0; j0 < m; j0 += C) {
    const int64_t nc = std::min(C, m - j0);
    GMAT_TRY(snp_coding_rows(0, g, j0, nc, dc.as<double>(), 0, a.as<double>()));
    GMAT_TRY(gemm_rows(0, nc, n, n, a.as<double>(), P, ap.as<double>(), n));
    if (dom) {
      GMAT_TRY(snp_coding_rows(0, g, j0, nc, dc.as<double>() + m, 1, d.as<double>()));
      GMAT_TRY(gemm_rows(0, nc, n, n, d.as<double>(), P, dpp.as<double>(), n));
    }
    hipLaunchKernelGGL(lmm_snp_kernel, dim3((unsigned)cdiv(nc, 4)), dim3(256), 0, 0, nc, n, a.as<double>(), ap.as<double>(),
                       dom ? d.as<double>() : nullptr, dom ? dpp.as<double>() : nullptr, dpy.as<double>(), oe + j0,
                       ov + j0, oc + j0);
    GMAT_HIP(hipGetLastError());
  }
  GMAT_HIP(hipMemcpy(eff, oe, m * sizeof(double), hipMemcpyDeviceToHost));
  GMAT_HIP(hipMemcpy(var, ov, m * sizeof(double), hipMemcpyDeviceToHost));
  GMAT_HIP(hipMemcpy(chi, oc, m * sizeof(double), hipMemcpyDeviceToHost));
  return GMAT_OK;
}

extern "C" int gmat_lmm_epi_rows(gmat_epi *e, const int64_t *rows, int64_t n_rows, int64_t block, double *eff, double *var,
                                 double *chi, double *p) {
  GMAT_CHECK(e && n_rows >= 0 && block >= 0 && (n_rows == 0 || rows), GMAT_E_ARG, "gmat_lmm_epi_rows: bad arguments");
  GMAT_CHECK(block <= 65535, GMAT_E_ARG, "gmat_lmm_epi_rows: at most 65,535 rows per pass");
  GMAT_CHECK(!e->seg, GMAT_E_ARG, "gmat_lmm_epi_rows: the plan is cut into SNP segments (2 m n_pad >= 2^32): not supported");
  const int64_t m = e->m, n_pad = e->n_pad;
  int64_t total = 0;
  for (int64_t r = 0; r < n_rows; ++r) {
    GMAT_CHECK(rows[r] >= 0 && rows[r] < m - 1 && (r == 0 || rows[r] > rows[r - 1]), GMAT_E_ARG,
               "gmat_lmm_epi_rows: rows must be strictly increasing first SNPs in [0, %lld)", (long long)(m - 1));
    total += m - 1 - rows[r];
  }
  if (total == 0) return GMAT_OK;
  GMAT_CHECK(eff && var && chi && p, GMAT_E_ARG, "gmat_lmm_epi_rows: null output");
  const double t_start = now();
  GMAT_TRY(build_coding(e, 0));
  // as gmat_epi_pairs: the kernel timers record the calls since the last scan or pairs call only
  e->kev_used = 0;
  e->kmarks.clear();
  const double t_s0 = now();
  const bool first = !e->lmm.ready;
  GMAT_TRY(lmm_setup(e));
  const double t_setup = first ? now() - t_s0 : 0.0;
  const hipStream_t s = e->s;
  const int64_t B = std::min(n_rows, block > 0 ? block : LMM_BLOCK), Bp = round_up(B, LMM_GB);
  // a block's pairs: at most B rows of the longest row in the list
  const int64_t cap = B * (m - 1 - rows[0]);
  DBuf di, dj, de, dv, dc, dpv, drows, doffs, Sr, Wr, caa, cei, cej;
  for (DBuf *b : {&di, &dj, &de, &dv, &dc, &dpv}) GMAT_TRY(b->alloc((size_t)cap * 8));
  GMAT_TRY(drows.alloc(B * 8));
  GMAT_TRY(doffs.alloc(B * 8));
  GMAT_TRY(Sr.alloc((size_t)Bp * n_pad * sizeof(double)));
  GMAT_TRY(Wr.alloc((size_t)Bp * n_pad * sizeof(double)));
  for (DBuf *b : {&caa, &cei, &cej}) GMAT_TRY(b->alloc((size_t)Bp * m * sizeof(double)));
  // rows of the last dgemm of a block that no SNP fills are multiplied too: keep them finite
  GMAT_HIP(hipMemsetAsync(Sr.p, 0, (size_t)Bp * n_pad * sizeof(double), s));
  GMAT_HIP(hipMemsetAsync(Wr.p, 0, (size_t)Bp * n_pad * sizeof(double), s));
  hipEvent_t ev[4];
  for (auto &x : ev) GMAT_HIP(hipEventCreate(&x));
  struct EvFree {
    hipEvent_t *ev;
    ~EvFree() {
      for (int k = 0; k < 4; ++k) (void)hipEventDestroy(ev[k]);
    }
  } ev_free{ev};
  const double *S = e->lmm.S.as<double>(), *Y = e->lmm.Y.as<double>(), *W = e->lmm.W.as<double>();
  std::vector<int64_t> offs(B);
  double t_ref = 0, t_gemm = 0, t_comb = 0;
  int64_t done = 0;
  for (int64_t r0 = 0; r0 < n_rows; r0 += B) {
    const int64_t nr = std::min(B, n_rows - r0);
    int64_t np = 0;
    for (int64_t r = 0; r < nr; ++r) {
      offs[r] = np;
      np += m - 1 - rows[r0 + r];
    }
    GMAT_HIP(hipMemcpyAsync(drows.p, rows + r0, nr * 8, hipMemcpyHostToDevice, s));
    GMAT_HIP(hipMemcpyAsync(doffs.p, offs.data(), nr * 8, hipMemcpyHostToDevice, s));
    const int64_t per_row = m - 1 - rows[r0];  // the longest row of the block (rows increase)
    const dim3 pgrid((unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(per_row, 256), 64)), (unsigned)nr);
    hipLaunchKernelGGL(all_pairs_kernel, pgrid, dim3(256), 0, s, drows.as<int64_t>(), doffs.as<int64_t>(), m, 1,
                       (int64_t)0, di.as<int64_t>(), dj.as<int64_t>());
    GMAT_HIP(hipGetLastError());
    GMAT_HIP(hipEventRecord(ev[0], s));
    GMAT_TRY(refine(e, s, e->code[0], e->code[0], e->g->dose_ptr(), e->g->dose_ptr(), di.as<int64_t>(), dj.as<int64_t>(),
                    np, de.as<double>(), dv.as<double>(), dc.as<double>(), dpv.as<double>()));
    GMAT_HIP(hipEventRecord(ev[1], s));
    hipLaunchKernelGGL(lmm_gather_kernel, dim3((unsigned)nr), dim3(256), 0, s, n_pad, drows.as<int64_t>(), S, W,
                       Sr.as<double>(), Wr.as<double>());
    GMAT_HIP(hipGetLastError());
    GMAT_TRY(gemm_rows(s, nr, m, n_pad, Sr.as<double>(), DView{Y, n_pad, 1}, caa.as<double>(), m));
    GMAT_TRY(gemm_rows(s, nr, m, n_pad, Wr.as<double>(), DView{S, n_pad, 1}, cei.as<double>(), m));
    GMAT_TRY(gemm_rows(s, nr, m, n_pad, Sr.as<double>(), DView{W, n_pad, 1}, cej.as<double>(), m));
    GMAT_HIP(hipEventRecord(ev[2], s));
    hipLaunchKernelGGL(lmm_epi_kernel, pgrid, dim3(256), 0, s, m, drows.as<int64_t>(), doffs.as<int64_t>(),
                       caa.as<double>(), cei.as<double>(), cej.as<double>(), e->lmm.d.as<double>(), e->lmm.q.as<double>(),
                       de.as<double>(), dv.as<double>(), dc.as<double>(), dpv.as<double>());
    GMAT_HIP(hipGetLastError());
    GMAT_HIP(hipEventRecord(ev[3], s));
    GMAT_HIP(hipMemcpyAsync(eff + done, de.p, np * 8, hipMemcpyDeviceToHost, s));
    GMAT_HIP(hipMemcpyAsync(var + done, dv.p, np * 8, hipMemcpyDeviceToHost, s));
    GMAT_HIP(hipMemcpyAsync(chi + done, dc.p, np * 8, hipMemcpyDeviceToHost, s));
    GMAT_HIP(hipMemcpyAsync(p + done, dpv.p, np * 8, hipMemcpyDeviceToHost, s));
    GMAT_HIP(hipStreamSynchronize(s));  // the next block reuses the buffers (and offs)
    float ms[3];
    for (int k = 0; k < 3; ++k) GMAT_HIP(hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]));
    t_ref += ms[0] * 1e-3;
    t_gemm += ms[1] * 1e-3;
    t_comb += ms[2] * 1e-3;
    done += np;
  }
  g_lmm_stats[0] = (double)total;
  g_lmm_stats[1] = t_setup;
  g_lmm_stats[2] = t_ref;
  g_lmm_stats[3] = t_gemm;
  g_lmm_stats[4] = t_comb;
  g_lmm_stats[5] = now() - t_start;
  return GMAT_OK;
}

extern "C" int gmat_lmm_stats(double *out8) {
  GMAT_CHECK(out8, GMAT_E_ARG, "gmat_lmm_stats: null output");
  for (int k = 0; k < 8; ++k) out8[k] = g_lmm_stats[k];
  return GMAT_OK;
}
