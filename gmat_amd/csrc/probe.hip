// Diagnostics entry points that exercise single instructions the screens rely on, so that
// tests can check the rigorous error bounds the screens assume against the hardware itself.
//
// gmat_probe_mx_accum: the low-rank screen's accumulation (lr_screen_kernel, epi.hip) -- a chain of
// v_mfma_scale_f32_32x32x64_f8f6f4 (A fp6 e2m3 with one e8m0 scale per lane = per (row, 32 k),
// B fp4 e2m1) accumulated in fp32 over n_steps k-blocks of 64, exactly the instruction, operand
// formats, B scale (128: the fp4 codes hold w/2) and accumulation order of the screen.  B is the
// screen's worst case everywhere (w = 4, fp4 code 0x4 = 2.0), so every column of the result equals
// 4 sum_k A[r][k] and the exact value needs no knowledge of the lane -> k map.
#include "common.h"

namespace {
typedef int v8i_ __attribute__((ext_vector_type(8)));
typedef float v16f_ __attribute__((ext_vector_type(16)));

// codes: [n_steps][32 rows][2 halves][32] fp6 codes (0..63); scales: [n_steps][32][2] e8m0
__global__ __launch_bounds__(64) void mx_accum_probe_kernel(int n_steps, const uint8_t *codes, const uint8_t *scales,
                                                             float *out) {
  const int l = threadIdx.x, r = l & 31, h = l >> 5;
  v16f_ acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  v8i_ fb;
  for (int q = 0; q < 8; ++q) fb[q] = q < 4 ? 0x44444444 : 0;
  for (int s = 0; s < n_steps; ++s) {
    const uint8_t *cs = codes + (((int64_t)s * 32 + r) * 2 + h) * 32;
    uint32_t a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = 0; j < 32; ++j) {
      const uint32_t c = cs[j] & 63u;
      const int bit = 6 * j;
      a[bit >> 5] |= c << (bit & 31);
      if ((bit & 31) > 26) a[(bit >> 5) + 1] |= c >> (32 - (bit & 31));
    }
    v8i_ fa;
    for (int q = 0; q < 8; ++q) fa[q] = (int)a[q];
    const int sa = scales[((int64_t)s * 32 + r) * 2 + h];
    acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fa, fb, acc, 2, 4, 0, sa, 0, 128);
  }
  for (int q = 0; q < 16; ++q) {
    const int row = (q & 3) + 8 * (q >> 2) + 4 * h;
    out[row * 32 + r] = acc[q];
  }
}
}  // namespace

extern "C" int gmat_probe_mx_accum(int n_steps, const uint8_t *codes, const uint8_t *scales, float *out) {
  using namespace gmat;
  GMAT_CHECK(n_steps > 0 && n_steps <= 1024 && codes && scales && out, GMAT_E_ARG, "gmat_probe_mx_accum: bad arguments");
  DBuf dc, ds, dout;
  GMAT_TRY(dc.alloc((size_t)n_steps * 32 * 2 * 32));
  GMAT_TRY(ds.alloc((size_t)n_steps * 32 * 2));
  GMAT_TRY(dout.alloc(32 * 32 * sizeof(float)));
  GMAT_HIP(hipMemcpy(dc.p, codes, (size_t)n_steps * 32 * 2 * 32, hipMemcpyHostToDevice));
  GMAT_HIP(hipMemcpy(ds.p, scales, (size_t)n_steps * 32 * 2, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(mx_accum_probe_kernel, dim3(1), dim3(64), 0, 0, n_steps, dc.as<uint8_t>(), ds.as<uint8_t>(),
                     dout.as<float>());
  GMAT_HIP(hipGetLastError());
  GMAT_HIP(hipMemcpy(out, dout.p, 32 * 32 * sizeof(float), hipMemcpyDeviceToHost));
  return GMAT_OK;
}

// gmat_probe_eig_bottom: the plan's partial symmetric eigensolver (eig.hip: Chebyshev-filtered
// subspace iteration with a device Rayleigh-Ritz) on a host matrix, so tests can compare it with a
// dense reference decomposition.  res_out (ne residual norms) and iters_out may be null.
#include "dla.h"
extern "C" int gmat_probe_eig_bottom(int64_t n, const double *a_host, int ne, double tol, int maxit, double *w_out,
                                     double *z_out, double *res_out, int *iters_out) {
  using namespace gmat;
  GMAT_CHECK(n >= 2 && a_host && w_out && z_out && ne >= 1 && ne <= n && maxit >= 1, GMAT_E_ARG,
             "gmat_probe_eig_bottom: bad arguments");
  DBuf a, z;
  GMAT_TRY(a.alloc((size_t)n * n * sizeof(double)));
  GMAT_TRY(z.alloc((size_t)n * ne * sizeof(double)));
  GMAT_HIP(hipMemcpy(a.p, a_host, (size_t)n * n * sizeof(double), hipMemcpyHostToDevice));
  GMAT_TRY(sym_eig_bottom(n, a.as<double>(), ne, tol, maxit, w_out, z.as<double>(), res_out, iters_out));
  GMAT_HIP(hipMemcpy(z_out, z.p, (size_t)n * ne * sizeof(double), hipMemcpyDeviceToHost));
  return GMAT_OK;
}

// gmat_probe_dgemm / gmat_probe_cholesky / gmat_probe_dot_rows: the dense fp64 layer of dla.h on host
// arrays, on the null stream, so tests can compare it with exact references.  Whole host buffers go up
// (padding included) and whole output buffers come back, so a test can poison padding and see whether
// it was read or written.
namespace {
int upload(gmat::DBuf &d, const void *h, size_t bytes) {
  using namespace gmat;
  GMAT_TRY(d.alloc(bytes));
  GMAT_HIP(hipMemcpy(d.p, h, bytes, hipMemcpyHostToDevice));
  return GMAT_OK;
}
// a fresh output buffer, every byte 0xFF (a NaN in every double): what the call leaves unwritten shows
int nan_buffer(gmat::DBuf &d, size_t bytes) {
  using namespace gmat;
  GMAT_TRY(d.alloc(bytes));
  GMAT_HIP(hipMemset(d.p, 0xFF, bytes));
  return GMAT_OK;
}
}  // namespace

extern "C" int gmat_probe_dgemm(int64_t M, int64_t N, int64_t K, double alpha, double beta, int mask, const void *a,
                                int a_i8, int trans_a, int64_t lda, const void *b, int b_i8, int trans_b, int64_t ldb,
                                double *c, int64_t ldc) {
  using namespace gmat;
  GMAT_CHECK(M >= 1 && N >= 1 && K >= 1 && a && b && c && mask >= 0 && mask <= 2, GMAT_E_ARG,
             "gmat_probe_dgemm: bad arguments");
  GMAT_CHECK(!(a_i8 && b_i8), GMAT_E_ARG, "gmat_probe_dgemm: both operands int8");
  GMAT_CHECK(!((a_i8 || b_i8) && mask), GMAT_E_ARG, "gmat_probe_dgemm: the int8 products take no mask");
  GMAT_CHECK(lda >= (trans_a ? M : K) && ldb >= (trans_b ? K : N) && ldc >= N, GMAT_E_ARG,
             "gmat_probe_dgemm: leading dimension below the row length");
  const size_t na = (size_t)(trans_a ? K : M) * lda * (a_i8 ? 1 : sizeof(double));
  const size_t nb = (size_t)(trans_b ? N : K) * ldb * (b_i8 ? 1 : sizeof(double));
  const size_t nc = (size_t)M * ldc * sizeof(double);
  DBuf da, db, dc;
  GMAT_TRY(upload(da, a, na));
  GMAT_TRY(upload(db, b, nb));
  GMAT_TRY(upload(dc, c, nc));
  if (a_i8)
    GMAT_TRY(dgemm_i8a(0, M, N, K, alpha, I8View{da.as<int8_t>(), lda, trans_a}, DView{db.as<double>(), ldb, trans_b},
                       beta, dc.as<double>(), ldc));
  else if (b_i8)
    GMAT_TRY(dgemm_i8b(0, M, N, K, alpha, DView{da.as<double>(), lda, trans_a}, I8View{db.as<int8_t>(), ldb, trans_b},
                       beta, dc.as<double>(), ldc));
  else
    GMAT_TRY(dgemm(0, M, N, K, alpha, DView{da.as<double>(), lda, trans_a}, DView{db.as<double>(), ldb, trans_b}, beta,
                   dc.as<double>(), ldc, mask));
  GMAT_HIP(hipStreamSynchronize(0));
  GMAT_HIP(hipMemcpy(c, dc.p, nc, hipMemcpyDeviceToHost));
  return GMAT_OK;
}

extern "C" int gmat_probe_cholesky(int64_t n, const double *a, int64_t lda, int mode, double *a_out, double *dinv,
                                   double *linv, double *vinv, double *logdet, int *info) {
  using namespace gmat;
  GMAT_CHECK(n >= 1 && lda >= n && a && a_out && dinv && logdet && info && mode >= 0 && mode <= 3, GMAT_E_ARG,
             "gmat_probe_cholesky: bad arguments");
  GMAT_CHECK((mode == 0 || linv) && (mode < 2 || vinv), GMAT_E_ARG, "gmat_probe_cholesky: mode %d needs its outputs",
             mode);
  const size_t na = (size_t)n * lda * sizeof(double), nn = (size_t)n * n * sizeof(double);
  const size_t nd = (size_t)n * 64 * sizeof(double);
  DBuf da, dd, dl, dv, dw, sm;
  GMAT_TRY(upload(da, a, na));
  GMAT_TRY(nan_buffer(dd, nd));
  if (mode >= 1) GMAT_TRY(nan_buffer(dl, nn));
  if (mode >= 2) GMAT_TRY(nan_buffer(dv, nn));
  if (mode == 3) GMAT_TRY(nan_buffer(dw, nn));
  GMAT_TRY(nan_buffer(sm, 2 * sizeof(double)));
  double *ld = sm.as<double>();
  int *inf = reinterpret_cast<int *>(ld + 1);
  if (mode == 0 || mode == 3) {
    GMAT_TRY(cholesky(0, n, da.as<double>(), lda, dd.as<double>(), ld, inf));
    if (mode == 3) {
      GMAT_TRY(chol_lower_inverse(0, n, da.as<double>(), lda, dd.as<double>(), dl.as<double>()));
      GMAT_TRY(spd_inverse_from_chol(0, n, da.as<double>(), lda, dd.as<double>(), dw.as<double>(), dv.as<double>()));
    }
  } else {
    GMAT_TRY(cholesky_inverse(0, n, da.as<double>(), lda, dd.as<double>(), ld, inf, dl.as<double>(),
                              mode == 2 ? dv.as<double>() : nullptr));
  }
  GMAT_HIP(hipStreamSynchronize(0));
  GMAT_HIP(hipMemcpy(a_out, da.p, na, hipMemcpyDeviceToHost));
  GMAT_HIP(hipMemcpy(dinv, dd.p, nd, hipMemcpyDeviceToHost));
  if (mode >= 1) GMAT_HIP(hipMemcpy(linv, dl.p, nn, hipMemcpyDeviceToHost));
  if (mode >= 2) GMAT_HIP(hipMemcpy(vinv, dv.p, nn, hipMemcpyDeviceToHost));
  GMAT_HIP(hipMemcpy(logdet, ld, sizeof(double), hipMemcpyDeviceToHost));
  GMAT_HIP(hipMemcpy(info, inf, sizeof(int), hipMemcpyDeviceToHost));
  return GMAT_OK;  // a non-positive pivot is the caller's to see (*info > 0)
}

extern "C" int gmat_probe_dot_rows(int64_t rows, int64_t n, const double *a, int64_t lda, const double *b, int64_t ldb,
                                   double *out) {
  using namespace gmat;
  GMAT_CHECK(rows >= 1 && n >= 1 && a && out && lda >= n && (!b || ldb == 0 || ldb >= n), GMAT_E_ARG,
             "gmat_probe_dot_rows: bad arguments");
  DBuf da, db, dout;
  GMAT_TRY(upload(da, a, (size_t)rows * lda * sizeof(double)));
  // ldb == 0: one row shared by every output
  if (b) GMAT_TRY(upload(db, b, (size_t)(ldb == 0 ? n : rows * ldb) * sizeof(double)));
  GMAT_TRY(nan_buffer(dout, (size_t)rows * sizeof(double)));
  GMAT_TRY(dot_rows(0, rows, n, da.as<double>(), lda, b ? db.as<double>() : nullptr, ldb, dout.as<double>()));
  GMAT_HIP(hipStreamSynchronize(0));
  GMAT_HIP(hipMemcpy(out, dout.p, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost));
  return GMAT_OK;
}
