// Torch extension bindings for the dlaf_amd CDNA4 kernels.
//
// All entry points take CUDA (ROCm) tensors, run on the CURRENT torch stream
// (so the Python runtime's stream/event scheduling applies), and are
// asynchronous. The per-tile Cholesky (`potrf_tile`) is one launch per block
// column of the tile (csrc/factor.hip, csrc/potrf_plan.h).
//
// Every binding goes through dispatch_dtype: scalar type -> element-type tag
// -> generic lambda calling the typed entry points of kernels.h.
#include <torch/extension.h>
#include <c10/cuda/CUDAStream.h>
#include <c10/cuda/CUDACachingAllocator.h>
#include <hip/hip_runtime.h>

#include <ATen/Parallel.h>

#include <algorithm>
#include <cfloat>
#include <thread>
#include <tuple>
#include <type_traits>
#include <vector>

#include "kernels.h"
#include "potrf_plan.h"
#include "sturm.h"
#include "tridiag_lu.h"

// csrc/rocblas_batch.cpp
void lib_gemm_batched(torch::Tensor dt, torch::Tensor ptrC, torch::Tensor ptrA,
                      torch::Tensor ptrB, int64_t M, int64_t N, int64_t K,
                      int64_t lda, int64_t ldb, int64_t ldc, int64_t opA,
                      int64_t opB, double alpha_re, double alpha_im,
                      double beta_re, double beta_im);

namespace {

#define HIP_CHECK(expr)                                                     \
  do {                                                                      \
    hipError_t _e = (expr);                                                 \
    TORCH_CHECK(_e == hipSuccess, "HIP error: ", hipGetErrorString(_e));    \
  } while (0)

hipStream_t cur_stream() {
  return (hipStream_t)at::cuda::getCurrentCUDAStream().stream();
}

using dlaf::kPotrfBsz;

template <typename S>
struct Tag {
  using type = S;     // kernel element type
  using real_t = S;
  using torch_t = S;  // torch's name for it
};
template <typename T>
struct Tag<cplx<T>> {
  using type = cplx<T>;
  using real_t = T;
  using torch_t = c10::complex<T>;
};

// The single dtype dispatch: calls f(Tag<S>{}) with S the element type of `t`.
template <typename F>
auto dispatch_dtype(at::ScalarType t, F&& f) {
  switch (t) {
    case at::kDouble:
      return f(Tag<double>{});
    case at::kFloat:
      return f(Tag<float>{});
    case at::kComplexDouble:
      return f(Tag<cplx<double>>{});
    case at::kComplexFloat:
      return f(Tag<cplx<float>>{});
    default:
      TORCH_CHECK(false, "unsupported dtype");
  }
}

// The one place a torch pointer becomes a typed pointer (checks the dtype;
// cplx<T> and c10::complex<T> are both the interleaved (re, im) pair).
template <typename S>
S* ptr(const torch::Tensor& t) {
  using torch_t = typename Tag<std::remove_const_t<S>>::torch_t;
  return reinterpret_cast<S*>(t.data_ptr<torch_t>());
}

// alpha/beta arrive from Python as (re, im) doubles
template <typename S>
S scalar(double re, double im) {
  using R = typename Tag<S>::real_t;
  if constexpr (std::is_same_v<S, R>)
    return (R)re;
  else
    return S((R)re, (R)im);
}

void check_gemm_args(const torch::Tensor& desc, const torch::Tensor& A,
                     const torch::Tensor& B, const torch::Tensor& C) {
  TORCH_CHECK(C.is_cuda() && A.is_cuda() && B.is_cuda(), "tensors must be on GPU");
  TORCH_CHECK(desc.is_cuda() && desc.scalar_type() == at::kLong && desc.is_contiguous(),
              "desc must be contiguous int64 on GPU");
  TORCH_CHECK(desc.dim() == 2 && desc.size(1) == 6, "desc must be [n, 6]");
  TORCH_CHECK(A.scalar_type() == C.scalar_type() && B.scalar_type() == C.scalar_type(),
              "dtype mismatch");
}

// C[desc] = alpha * op(A) op(B) + beta * C ; desc rows are
// (c_off, a_off, b_off, ktiles, a_kstride, b_kstride) in element units.
void batch_gemm(torch::Tensor C, torch::Tensor A, torch::Tensor B,
                torch::Tensor desc, int64_t M, int64_t N, int64_t K,
                int64_t lda, int64_t ldb, int64_t ldc, int64_t opA, int64_t opB,
                double alpha_re, double alpha_im, double beta_re,
                double beta_im, bool inplace) {
  check_gemm_args(desc, A, B, C);
  const int nd = (int)desc.size(0);
  if (nd == 0) return;
  auto descs = reinterpret_cast<const GemmDesc*>(desc.data_ptr<int64_t>());
  auto s = cur_stream();
  dispatch_dtype(C.scalar_type(), [&](auto tag) {
    using S = typename decltype(tag)::type;
    dlaf::gemm_tiles(descs, nd, ptr<const S>(A), ptr<const S>(B), ptr<S>(C), M,
                     N, K, lda, ldb, ldc, opA, opB,
                     scalar<S>(alpha_re, alpha_im), scalar<S>(beta_re, beta_im),
                     s, inplace);
  });
  HIP_CHECK(hipGetLastError());
}

// T = tril(L)^-1 for an n x n view; T must not alias L.
void trtri_lower(torch::Tensor L, torch::Tensor T, int64_t n, int64_t ldl,
                 int64_t ldt, bool unit_diag) {
  TORCH_CHECK(L.is_cuda() && T.is_cuda());
  auto s = cur_stream();
  dispatch_dtype(L.scalar_type(), [&](auto tag) {
    using S = typename decltype(tag)::type;
    dlaf::trtri_lower(ptr<const S>(L), ptr<S>(T), n, ldl, ldt, unit_diag, s);
  });
  HIP_CHECK(hipGetLastError());
}

// In-place Cholesky (Lower) of the leading n x n of a tile with row stride ld.
// Also fills `dinv` ([nblocks, bsz, bsz] contiguous) with the inverses of the
// bsz x bsz diagonal blocks of the factor — the panel TRSM then becomes GEMMs.
// `side` is the workspace of dlaf::potrf_tile_fused (cached by the Python
// layer); calls that may run concurrently need separate ones.
void potrf_tile(torch::Tensor A, int64_t n, int64_t ld, torch::Tensor dinv,
                torch::Tensor side) {
  TORCH_CHECK(A.is_cuda() && dinv.is_cuda() && dinv.is_contiguous());
  TORCH_CHECK(side.is_cuda() && side.is_contiguous());
  TORCH_CHECK(dinv.scalar_type() == A.scalar_type() &&
              side.scalar_type() == A.scalar_type(), "dtype mismatch");
  TORCH_CHECK(n >= 0 && n < (int64_t(1) << 30) && ld >= n, "bad n / ld");
  constexpr int bsz = kPotrfBsz;
  const int nblocks = dlaf::potrf_plan::nblocks((int)n, bsz);
  TORCH_CHECK(dinv.numel() >= (int64_t)nblocks * bsz * bsz, "dinv too small");
  TORCH_CHECK(side.numel() >= dlaf::potrf_plan::side_elems(nblocks, bsz),
              "side workspace too small");
  auto s = cur_stream();
  dispatch_dtype(A.scalar_type(), [&](auto tag) {
    using S = typename decltype(tag)::type;
    dlaf::potrf_tile_fused(ptr<S>(A), (int)n, (int)ld, ptr<S>(dinv),
                           ptr<S>(side), s);
  });
  HIP_CHECK(hipGetLastError());
}

// Dtypes with the single-launch panel TRSM (csrc/trsm_panel.hip); the others
// solve their panels through batch_gemm.
bool trsm_panel_supported(torch::Tensor t) {
  return t.scalar_type() == at::kDouble || t.scalar_type() == at::kFloat;
}

// X <- X * tril(L)^-T for the ntiles = tile_offs.numel() tiles (mb x nb, row
// stride ld) at element offsets tile_offs (device int64) into base; dinv as
// potrf_tile fills it. strip: 0 = the kernel's own choice, else 16 or 32.
void trsm_panel(torch::Tensor base, torch::Tensor tile_offs, torch::Tensor L,
                int64_t ldl, torch::Tensor dinv, int64_t mb, int64_t nb,
                int64_t ld, int64_t strip) {
  TORCH_CHECK(base.is_cuda() && L.is_cuda() && dinv.is_cuda() &&
              dinv.is_contiguous(), "tensors must be on GPU");
  TORCH_CHECK(tile_offs.is_cuda() && tile_offs.scalar_type() == at::kLong &&
              tile_offs.is_contiguous() && tile_offs.dim() == 1,
              "tile_offs must be contiguous 1-d int64 on GPU");
  TORCH_CHECK(trsm_panel_supported(base), "trsm_panel: dtype has no kernel");
  TORCH_CHECK(L.scalar_type() == base.scalar_type() &&
              dinv.scalar_type() == base.scalar_type(), "dtype mismatch");
  TORCH_CHECK(mb >= 1 && nb >= 1 && mb < (int64_t(1) << 30) &&
              nb < (int64_t(1) << 30) && ld >= nb && ldl >= nb, "bad shape");
  TORCH_CHECK(strip == 0 || strip == 16 || strip == 32,
              "strip must be 0, 16 or 32");
  constexpr int bsz = kPotrfBsz;
  const int64_t nblocks = (nb + bsz - 1) / bsz;
  TORCH_CHECK(dinv.numel() >= nblocks * bsz * bsz, "dinv too small");
  TORCH_CHECK(L.storage_offset() + (nb - 1) * ldl + nb <=
              (int64_t)(L.storage().nbytes() / L.element_size()),
              "L view exceeds its storage");
  TORCH_CHECK((mb - 1) * ld + nb <= base.numel(), "tile exceeds base");
  const int nt = (int)tile_offs.numel();
  if (nt == 0) return;
  auto s = cur_stream();
  dispatch_dtype(base.scalar_type(), [&](auto tag) {
    using S = typename decltype(tag)::type;
    if constexpr (std::is_same_v<S, double> || std::is_same_v<S, float>) {
      const int st = strip ? (int)strip : dlaf::trsm_panel_strip(nt, (int)mb);
      dlaf::trsm_panel_fused_strip(ptr<S>(base), tile_offs.data_ptr<int64_t>(),
                                   nt, ptr<const S>(L), (int)ldl,
                                   ptr<const S>(dinv), (int)mb, (int)nb,
                                   (int)ld, st, s);
    }
  });
  HIP_CHECK(hipGetLastError());
}

// Factor (optional) + invert ONE bsz-block of a tile view; Tout = dinv[d].
void factor_invert_block(torch::Tensor A, int64_t n, int64_t ld,
                         torch::Tensor Tout, bool do_factor) {
  TORCH_CHECK(A.is_cuda() && Tout.is_cuda());
  TORCH_CHECK(n <= 64);
  auto s = cur_stream();
  dispatch_dtype(A.scalar_type(), [&](auto tag) {
    using S = typename decltype(tag)::type;
    dlaf::potrf_invert_block(ptr<S>(A), n, ld, ptr<S>(Tout), do_factor, s);
  });
  HIP_CHECK(hipGetLastError());
}

// Cooperative whole-panel QR (see csrc/panel_qr.hip). P: 2D device view with
// unit column stride; taus: [min(m,nb)]; norms/wraw: zeroed workspaces.
void panel_qr(torch::Tensor P, torch::Tensor taus, torch::Tensor norms,
              torch::Tensor wraw) {
  TORCH_CHECK(P.is_cuda() && P.dim() == 2 && P.stride(1) == 1);
  const long m = P.size(0), ldp = P.stride(0);
  const int nb = (int)P.size(1);
  const int rc = dispatch_dtype(P.scalar_type(), [&](auto tag) {
    using S = typename decltype(tag)::type;
    using R = typename decltype(tag)::real_t;
    return dlaf::panel_qr(ptr<S>(P), m, nb, ldp, ptr<S>(taus), ptr<R>(norms),
                          ptr<S>(wraw), cur_stream());
  });
  TORCH_CHECK(rc == 0, "panel_qr cooperative launch failed, hipError ", rc);
  HIP_CHECK(hipGetLastError());
}

void secular_roots(torch::Tensor d, torch::Tensor z2, double rho,
                   torch::Tensor sidx, torch::Tensor mu) {
  TORCH_CHECK(d.is_cuda() && d.scalar_type() == torch::kFloat64);
  dlaf::secular_roots(d.data_ptr<double>(), z2.data_ptr<double>(),
                      (int)d.size(0), rho, (long long*)sidx.data_ptr<int64_t>(),
                      mu.data_ptr<double>(), cur_stream());
  HIP_CHECK(hipGetLastError());
}

// ---- tridiagonal eigenvalues by Sturm bisection (sturm.h / bisect.hip) ----

void check_tridiag(const torch::Tensor& d, const torch::Tensor& e2) {
  TORCH_CHECK(d.scalar_type() == torch::kFloat64 &&
              e2.scalar_type() == torch::kFloat64, "float64 required");
  TORCH_CHECK(d.dim() == 1 && e2.dim() == 1 && d.is_contiguous() &&
              e2.is_contiguous(), "contiguous 1-D tensors required");
  TORCH_CHECK(d.size(0) < (int64_t(1) << 30), "n too large");
  TORCH_CHECK(e2.size(0) == std::max<int64_t>(d.size(0) - 1, 0),
              "e2 must have n-1 entries");
  TORCH_CHECK(e2.device() == d.device(), "d and e2 on different devices");
}

// at::parallel_for is serial in a translation unit built without OpenMP;
// plain threads over contiguous index ranges do the job (as band_chase.cpp).
template <typename F>
void host_parallel(int64_t begin, int64_t end, int64_t work_per_item, F&& f) {
  const int64_t m = end - begin;
  int64_t nt = std::min<int64_t>(at::get_num_threads(), m);
  if (m * work_per_item < (int64_t(1) << 16)) nt = 1;  // not worth a thread
  if (nt <= 1) {
    if (m > 0) f(begin, end);
    return;
  }
  std::vector<std::thread> pool;
  for (int64_t t = 0; t < nt; ++t)
    pool.emplace_back([&f, begin, m, nt, t] {
      f(begin + m * t / nt, begin + m * (t + 1) / nt);
    });
  for (auto& th : pool) th.join();
}

// Host twins of the kernels: the same sturm.h functions in a plain loop.
void tridiag_bisect_host(const double* d, const double* e2, int n, int k_begin,
                         int k_end, double gl, double gu, double pivmin,
                         double* w) {
  if (n <= 0 || k_begin >= k_end) return;
  host_parallel(k_begin, k_end, 64 * (int64_t)n, [&](int64_t b, int64_t e) {
    for (int64_t k = b; k < e; ++k) {
      dlaf::sturm::Bisect s;
      dlaf::sturm::bisect_begin(s, gl, gu, pivmin);
      while (!s.done)
        dlaf::sturm::bisect_update(
            s, dlaf::sturm::count(d, e2, n, pivmin, s.mid), (int)k, pivmin);
      w[k - k_begin] = s.mid;
    }
  });
}

void sturm_count_host(const double* d, const double* e2, int n, double pivmin,
                      const double* x, int nx, long long* count) {
  host_parallel(0, nx, n, [&](int64_t b, int64_t e) {
    for (int64_t j = b; j < e; ++j)
      count[j] = n > 0 ? dlaf::sturm::count(d, e2, n, pivmin, x[j]) : 0;
  });
}

// (gl, gu, pivmin) of sturm::interval for CPU float64 d [n], e [n-1].
std::tuple<double, double, double> sturm_interval(torch::Tensor d,
                                                  torch::Tensor e) {
  check_tridiag(d, e);
  TORCH_CHECK(!d.is_cuda(), "sturm_interval runs on the host");
  double gl = 0, gu = 0, pivmin = DBL_MIN;
  if (d.size(0) > 0)
    dlaf::sturm::interval(d.data_ptr<double>(), e.data_ptr<double>(),
                          (int)d.size(0), &gl, &gu, &pivmin);
  return {gl, gu, pivmin};
}

// w[k - k_begin] = eigenvalue k of tridiag(d, e), k in [k_begin, k_end).
void tridiag_bisect(torch::Tensor d, torch::Tensor e2, int64_t k_begin,
                    int64_t k_end, double gl, double gu, double pivmin,
                    torch::Tensor w) {
  check_tridiag(d, e2);
  const int64_t n = d.size(0);
  TORCH_CHECK(0 <= k_begin && k_begin <= k_end && k_end <= n,
              "bad eigenvalue index range");
  TORCH_CHECK(w.scalar_type() == torch::kFloat64 && w.is_contiguous() &&
              w.numel() >= k_end - k_begin && w.device() == d.device(),
              "bad output tensor");
  if (d.is_cuda()) {
    dlaf::tridiag_bisect(d.data_ptr<double>(), e2.data_ptr<double>(), (int)n,
                         (int)k_begin, (int)k_end, gl, gu, pivmin,
                         w.data_ptr<double>(), cur_stream());
    HIP_CHECK(hipGetLastError());
  } else {
    tridiag_bisect_host(d.data_ptr<double>(), e2.data_ptr<double>(), (int)n,
                        (int)k_begin, (int)k_end, gl, gu, pivmin,
                        w.data_ptr<double>());
  }
}

// count[j] = number of eigenvalues of tridiag(d, e) strictly below x[j].
void sturm_count(torch::Tensor d, torch::Tensor e2, double pivmin,
                 torch::Tensor x, torch::Tensor count) {
  check_tridiag(d, e2);
  TORCH_CHECK(x.scalar_type() == torch::kFloat64 && x.dim() == 1 &&
              x.is_contiguous() && x.device() == d.device(), "bad x");
  TORCH_CHECK(count.scalar_type() == at::kLong && count.is_contiguous() &&
              count.numel() >= x.numel() && count.device() == d.device(),
              "bad count tensor");
  const int n = (int)d.size(0), nx = (int)x.size(0);
  auto cp = (long long*)count.data_ptr<int64_t>();
  if (d.is_cuda()) {
    dlaf::sturm_count(d.data_ptr<double>(), e2.data_ptr<double>(), n, pivmin,
                      x.data_ptr<double>(), nx, cp, cur_stream());
    HIP_CHECK(hipGetLastError());
  } else {
    sturm_count_host(d.data_ptr<double>(), e2.data_ptr<double>(), n, pivmin,
                     x.data_ptr<double>(), nx, cp);
  }
}

// ---- shifted tridiagonal solves (tridiag_lu.h / invit.hip) ----

// Host twin of the kernel: the same tridiag_lu.h functions, columns in
// blocks of 64 with the row loop outside so X and U are walked row by row.
void tridiag_shifted_solve_host(const double* d, const double* e, int n,
                                const double* lam, int k, double tol,
                                double* X, int64_t ldx, double* U,
                                int64_t cols) {
  if (n <= 0 || k <= 0) return;
  constexpr int kBlock = 64;
  const int64_t nblk = (k + kBlock - 1) / kBlock;
  const int64_t plane = (int64_t)n * cols;
  host_parallel(0, nblk, 64 * (int64_t)n, [&](int64_t bb, int64_t be) {
    for (int64_t blk = bb; blk < be; ++blk) {
      const int64_t c0 = blk * kBlock;
      const int w = (int)std::min<int64_t>(kBlock, k - c0);
      double a[kBlock], b[kBlock], xcur[kBlock], y1[kBlock], y2[kBlock];
      for (int j = 0; j < w; ++j) {
        a[j] = d[0] - lam[c0 + j];
        b[j] = n > 1 ? e[0] : 0.0;
        xcur[j] = X[c0 + j];
        y1[j] = y2[j] = 0.0;
      }
      for (int64_t i = 0; i < n; ++i) {
        const double sub = i < n - 1 ? e[i] : 0.0;
        const double dn = i + 1 < n ? d[i + 1] : 0.0;
        const double ne = i + 1 < n - 1 ? e[i + 1] : 0.0;
        double* xr = X + i * ldx + c0;
        double* ur = U + i * cols + c0;
        for (int j = 0; j < w; ++j) {
          double u0, u1, u2, xi = xcur[j];
          double xj = i + 1 < n ? xr[ldx + j] : 0.0;
          dlaf::trilu::forward(a[j], b[j], sub, dn - lam[c0 + j], ne, tol, xi,
                               xj, u0, u1, u2);
          xcur[j] = xj;
          xr[j] = xi;
          ur[j] = u0;
          ur[plane + j] = u1;
          ur[2 * plane + j] = u2;
        }
      }
      for (int64_t i = n - 1; i >= 0; --i) {
        double* xr = X + i * ldx + c0;
        const double* ur = U + i * cols + c0;
        for (int j = 0; j < w; ++j) {
          const double y = dlaf::trilu::back(xr[j], ur[j], ur[plane + j],
                                             ur[2 * plane + j], y1[j], y2[j]);
          y2[j] = y1[j];
          y1[j] = y;
          xr[j] = y;
        }
      }
    }
  });
}

// X[:, j] <- (T - lam[j] I)^-1 X[:, j] for tridiag(d, e); work [3, n, cols].
void tridiag_shifted_solve(torch::Tensor d, torch::Tensor e, torch::Tensor lam,
                           double tol, torch::Tensor X, torch::Tensor work) {
  check_tridiag(d, e);
  const int64_t n = d.size(0);
  TORCH_CHECK(lam.scalar_type() == torch::kFloat64 && lam.dim() == 1 &&
              lam.is_contiguous() && lam.device() == d.device(), "bad lam");
  const int64_t k = lam.size(0);
  TORCH_CHECK(k < (int64_t(1) << 30), "too many columns");
  TORCH_CHECK(X.scalar_type() == torch::kFloat64 && X.dim() == 2 &&
              X.size(0) == n && X.size(1) == k && X.device() == d.device(),
              "X must be float64 [n, k] on d's device");
  // a column slice of a wider row-major matrix is fine: rows ldx apart
  TORCH_CHECK(k == 0 || n == 0 ||
              (X.stride(1) == 1 && (n == 1 || X.stride(0) >= k)),
              "X must be row-major with unit column stride");
  TORCH_CHECK(work.scalar_type() == torch::kFloat64 && work.dim() == 3 &&
              work.is_contiguous() && work.size(0) == 3 &&
              work.size(1) == n && work.size(2) >= k &&
              work.device() == d.device(),
              "work must be contiguous float64 [3, n, >= k]");
  TORCH_CHECK(tol > 0.0, "tol must be positive");
  if (n == 0 || k == 0) return;
  const int64_t ldx = X.stride(0), cols = work.size(2);
  if (d.is_cuda()) {
    dlaf::tridiag_shifted_solve(d.data_ptr<double>(), e.data_ptr<double>(),
                                (int)n, lam.data_ptr<double>(), (int)k, tol,
                                X.data_ptr<double>(), ldx,
                                work.data_ptr<double>(), cols, cur_stream());
    HIP_CHECK(hipGetLastError());
  } else {
    tridiag_shifted_solve_host(d.data_ptr<double>(), e.data_ptr<double>(),
                               (int)n, lam.data_ptr<double>(), (int)k, tol,
                               X.data_ptr<double>(), ldx,
                               work.data_ptr<double>(), cols);
  }
}

bool bt_apply_group(torch::Tensor E, torch::Tensor V, torch::Tensor VTt,
                    int64_t base0, int64_t b, int64_t G, int64_t R,
                    int64_t nwin) {
  TORCH_CHECK(E.is_cuda() && V.is_cuda() && VTt.is_cuda());
  TORCH_CHECK(E.is_contiguous() && V.is_contiguous() && VTt.is_contiguous());
  const int64_t npad = E.size(0), nE = E.size(1);
  const bool ok = dispatch_dtype(E.scalar_type(), [&](auto tag) {
    using S = typename decltype(tag)::type;
    // kernels exist for f64 and c128 only; the caller falls back otherwise
    if constexpr (std::is_same_v<typename decltype(tag)::real_t, double>)
      return dlaf::bt_apply_group(ptr<S>(E), nE, npad, ptr<const S>(V),
                                  ptr<const S>(VTt), base0, (int)b, (int)G,
                                  (int)R, (int)nwin, cur_stream());
    else
      return false;
  });
  HIP_CHECK(hipGetLastError());
  return ok;
}

void band_chase_gpu(torch::Tensor band, int64_t b, torch::Tensor vstore,
                    torch::Tensor offsets, torch::Tensor done,
                    torch::Tensor abortf) {
  TORCH_CHECK(band.is_cuda() && vstore.is_cuda() && offsets.is_cuda() &&
              done.is_cuda() && abortf.is_cuda(), "device tensors required");
  TORCH_CHECK(b <= 64, "band_chase_gpu handles b <= 64");
  TORCH_CHECK(done.scalar_type() == at::kInt && abortf.scalar_type() == at::kInt);
  const int64_t size = band.size(0), ld = band.size(1);
  dispatch_dtype(band.scalar_type(), [&](auto tag) {
    using S = typename decltype(tag)::type;
    dlaf::chase_gpu(ptr<S>(band), ld, size, b, ptr<S>(vstore),
                    offsets.data_ptr<int64_t>(), done.data_ptr<int32_t>(),
                    abortf.data_ptr<int32_t>(), cur_stream());
  });
}

// ---- matrix norms over the local tile storage (norms.hip) ----

// (rows [tiles_r*mb], cols [tiles_c*nb], scal [4]) of dlaf::matrix_norms for
// a contiguous device storage [tiles_r, tiles_c, mb, nb]; float64, on the
// storage's device.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> matrix_norms(
    torch::Tensor storage, int64_t m, int64_t n, int64_t gr0, int64_t grs,
    int64_t gc0, int64_t gcs, int64_t structure, int64_t uplo,
    bool unit_diag) {
  TORCH_CHECK(storage.is_cuda() && storage.dim() == 4 &&
              storage.is_contiguous(),
              "storage must be a contiguous [tiles_r, tiles_c, mb, nb] "
              "device tensor");
  TORCH_CHECK(structure >= 0 && structure <= 2 && (uplo == 0 || uplo == 1),
              "bad structure / uplo");
  const int64_t tr = storage.size(0), tc = storage.size(1),
                mb = storage.size(2), nb = storage.size(3);
  TORCH_CHECK(tr > 0 && tc > 0 && mb > 0 && nb > 0, "empty storage");
  TORCH_CHECK(m >= 0 && n >= 0 && gr0 >= 0 && gc0 >= 0 && grs >= 1 && gcs >= 1,
              "bad geometry");
  TORCH_CHECK(tr * mb < (1LL << 31) && tc * nb < (1LL << 31) &&
              (gr0 + tr * grs) * mb < (1LL << 40) &&
              (gc0 + tc * gcs) * nb < (1LL << 40) &&
              tr * tc * ((mb + dlaf::kNormStripRows - 1) /
                         dlaf::kNormStripRows) < (1LL << 31),
              "matrix too large for the norm kernel");
  auto opts = storage.options().dtype(torch::kFloat64);
  auto rows = torch::empty({tr * mb}, opts);
  auto cols = torch::empty({tc * nb}, opts);
  auto scal = torch::empty({4}, opts);
  auto work = torch::empty(
      {dlaf::matrix_norms_work_size((int)tr, (int)tc, (int)mb, (int)nb)}, opts);
  dispatch_dtype(storage.scalar_type(), [&](auto tag) {
    using S = typename decltype(tag)::type;
    dlaf::matrix_norms(ptr<const S>(storage), (int)tr, (int)tc, (int)mb,
                       (int)nb, m, n, (int)gr0, (int)grs, (int)gc0, (int)gcs,
                       (int)structure, (int)uplo, unit_diag ? 1 : 0,
                       rows.data_ptr<double>(), cols.data_ptr<double>(),
                       scal.data_ptr<double>(), work.data_ptr<double>(),
                       cur_stream());
  });
  HIP_CHECK(hipGetLastError());
  return {rows, cols, scal};
}

// ---- triangular solve for one vector over the tile storage (trsv.hip) ----

// op(T) x = b in place on x [nt * nb]; storage [nt, nt, nb, nb] holds T in
// its uplo triangle, dinv [nt, nb, nb] the inverses of its diagonal tiles.
void trsv_tiles(torch::Tensor storage, torch::Tensor dinv, torch::Tensor x,
                int64_t n, int64_t uplo, int64_t op) {
  TORCH_CHECK(storage.is_cuda() && storage.dim() == 4 &&
              storage.is_contiguous() && storage.size(0) == storage.size(1) &&
              storage.size(2) == storage.size(3),
              "storage must be a contiguous [nt, nt, nb, nb] device tensor");
  const int64_t nt = storage.size(0), nb = storage.size(2);
  TORCH_CHECK(nb > 0 && nt * nb < (1LL << 31) && nt * nt < (1LL << 20),
              "matrix too large for the solve kernel");
  TORCH_CHECK(n >= 0 && n <= nt * nb && n > (nt - 1) * nb,
              "n does not match the storage");
  TORCH_CHECK(dinv.dim() == 3 && dinv.is_contiguous() && dinv.size(0) == nt &&
              dinv.size(1) == nb && dinv.size(2) == nb &&
              dinv.scalar_type() == storage.scalar_type() &&
              dinv.device() == storage.device(),
              "dinv must be contiguous [nt, nb, nb] like the storage");
  TORCH_CHECK(x.dim() == 1 && x.is_contiguous() && x.size(0) == nt * nb &&
              x.scalar_type() == storage.scalar_type() &&
              x.device() == storage.device(),
              "x must be contiguous [nt * nb] like the storage");
  TORCH_CHECK((uplo == 0 || uplo == 1) && op >= OP_N && op <= OP_C,
              "bad uplo / op");
  if (nt == 0) return;
  auto work = torch::empty({nb}, x.options());
  dispatch_dtype(storage.scalar_type(), [&](auto tag) {
    using S = typename decltype(tag)::type;
    dlaf::trsv_tiles(ptr<const S>(storage), ptr<const S>(dinv), ptr<S>(x),
                     ptr<S>(work), (int)nt, (int)nb, n, (int)uplo, (int)op,
                     cur_stream());
  });
  HIP_CHECK(hipGetLastError());
}

// ---- Hermitian matrix-vector product over the tile storage (hemv.hip) ----

// y = A x and, unless yabs is empty, yabs = |A| |x|; storage [nt, nt, nb, nb]
// holds the Hermitian A in its uplo triangle, x / y / yabs are [nt * nb]
// (yabs of the real dtype). Entries at or beyond n are left as they are.
void hemv_tiles(torch::Tensor storage, torch::Tensor x, torch::Tensor y,
                torch::Tensor yabs, int64_t n, int64_t uplo) {
  TORCH_CHECK(storage.is_cuda() && storage.dim() == 4 &&
              storage.is_contiguous() && storage.size(0) == storage.size(1) &&
              storage.size(2) == storage.size(3),
              "storage must be a contiguous [nt, nt, nb, nb] device tensor");
  const int64_t nt = storage.size(0), nb = storage.size(2);
  const int64_t strips =
      (nb + dlaf::kHemvStripRows - 1) / dlaf::kHemvStripRows;
  TORCH_CHECK(nb > 0 && nt * nb < (1LL << 31) && nt * nt < (1LL << 20) &&
              nt * (nt + 1) / 2 * strips < (1LL << 31),
              "matrix too large for the product kernel");
  TORCH_CHECK(n >= 0 && n <= nt * nb && n > (nt - 1) * nb,
              "n does not match the storage");
  for (const torch::Tensor* v : {&x, &y})
    TORCH_CHECK(v->dim() == 1 && v->is_contiguous() && v->size(0) == nt * nb &&
                v->scalar_type() == storage.scalar_type() &&
                v->device() == storage.device(),
                "x and y must be contiguous [nt * nb] like the storage");
  TORCH_CHECK(x.data_ptr() != y.data_ptr() || nt == 0,
              "x and y must not alias");
  const bool want_abs = yabs.numel() > 0;
  if (want_abs)
    TORCH_CHECK(yabs.dim() == 1 && yabs.is_contiguous() &&
                yabs.size(0) == nt * nb &&
                yabs.scalar_type() == c10::toRealValueType(storage.scalar_type()) &&
                yabs.device() == storage.device(),
                "yabs must be empty or contiguous [nt * nb] of the real dtype");
  TORCH_CHECK(uplo == 0 || uplo == 1, "bad uplo");
  if (nt == 0) return;
  auto work = torch::empty({dlaf::hemv_work_size((int)nt, (int)nb)},
                           storage.options().dtype(torch::kFloat64));
  dispatch_dtype(storage.scalar_type(), [&](auto tag) {
    using S = typename decltype(tag)::type;
    using R = typename decltype(tag)::real_t;
    dlaf::hemv_tiles(ptr<const S>(storage), ptr<const S>(x), ptr<S>(y),
                     want_abs ? yabs.data_ptr<R>() : (R*)nullptr, (int)nt,
                     (int)nb, n, (int)uplo, work.data_ptr<double>(),
                     cur_stream());
  });
  HIP_CHECK(hipGetLastError());
}

// ---- LU panel and row interchanges over the tile storage (lu_panel.hip) ----

// Factors tile column k of the square storage [nt, nt, nb, nb] in place with
// partial pivoting; ipiv [>= n] int32 (0-based) and info [1] int32 stay on
// the device.
void lu_panel(torch::Tensor storage, int64_t n, int64_t k, torch::Tensor ipiv,
              torch::Tensor info) {
  TORCH_CHECK(storage.is_cuda() && storage.dim() == 4 &&
              storage.is_contiguous() && storage.size(0) == storage.size(1) &&
              storage.size(2) == storage.size(3),
              "storage must be a contiguous [nt, nt, nb, nb] device tensor");
  const int64_t nt = storage.size(0), nb = storage.size(2);
  TORCH_CHECK(nb > 0 && nt * nb < (1LL << 21),
              "matrix too large for the LU panel kernel");
  TORCH_CHECK(n >= 0 && n <= nt * nb && n > (nt - 1) * nb,
              "n does not match the storage");
  TORCH_CHECK(k >= 0 && k < std::max<int64_t>(nt, 1), "bad tile column");
  TORCH_CHECK(ipiv.scalar_type() == at::kInt && ipiv.is_contiguous() &&
              ipiv.dim() == 1 && ipiv.size(0) >= n &&
              ipiv.device() == storage.device(),
              "ipiv must be a contiguous int32 vector of length n on the "
              "storage's device");
  TORCH_CHECK(info.scalar_type() == at::kInt && info.numel() == 1 &&
              info.device() == storage.device(),
              "info must be one int32 on the storage's device");
  if (nt == 0 || k * nb >= n) return;
  auto ws = torch::empty({dlaf::lu_panel_work_elems(n)}, storage.options());
  auto wsrow = torch::empty({dlaf::lu_panel_work_rows(n)},
                            storage.options().dtype(torch::kInt32));
  dispatch_dtype(storage.scalar_type(), [&](auto tag) {
    using S = typename decltype(tag)::type;
    dlaf::lu_panel(ptr<S>(storage), (int)nt, (int)nb, n, (int)k,
                   ipiv.data_ptr<int32_t>(), info.data_ptr<int32_t>(),
                   ptr<S>(ws), wsrow.data_ptr<int32_t>(), cur_stream());
  });
  HIP_CHECK(hipGetLastError());
}

// Swaps rows s and ipiv[s] for s in [s0, s1) (backwards when reverse) in the
// element columns [c0, c1) of a contiguous [lr, lc, mb, nb] storage.
void laswp_tiles(torch::Tensor storage, torch::Tensor ipiv, int64_t s0,
                 int64_t s1, int64_t c0, int64_t c1, bool reverse) {
  TORCH_CHECK(storage.is_cuda() && storage.dim() == 4 &&
              storage.is_contiguous(),
              "storage must be a contiguous [lr, lc, mb, nb] device tensor");
  const int64_t lr = storage.size(0), lc = storage.size(1),
                mb = storage.size(2), nb = storage.size(3);
  TORCH_CHECK(lr * mb < (1LL << 31) && lc * nb < (1LL << 31),
              "matrix too large for the interchange kernel");
  TORCH_CHECK(ipiv.scalar_type() == at::kInt && ipiv.is_contiguous() &&
              ipiv.dim() == 1 && ipiv.device() == storage.device(),
              "ipiv must be a contiguous int32 vector on the storage's device");
  TORCH_CHECK(0 <= s0 && s0 <= s1 && s1 <= ipiv.size(0) && s1 <= lr * mb,
              "bad pivot range");
  TORCH_CHECK(0 <= c0 && c0 <= c1 && c1 <= lc * nb, "bad column range");
  if (s1 == s0 || c1 == c0) return;
  dispatch_dtype(storage.scalar_type(), [&](auto tag) {
    using S = typename decltype(tag)::type;
    dlaf::laswp_tiles(ptr<S>(storage), (int)lr, (int)lc, (int)mb, (int)nb,
                      ipiv.data_ptr<int32_t>(), s0, s1, c0, c1,
                      reverse ? 1 : 0, cur_stream());
  });
  HIP_CHECK(hipGetLastError());
}

}  // namespace

// csrc/band_chase.cpp
void band_chase(torch::Tensor band, int64_t b, torch::Tensor vstore,
                torch::Tensor offsets, int64_t nthreads);
int64_t dc_deflate_scan(torch::Tensor d, torch::Tensor z, double rho,
                        double tol, torch::Tensor deflated, torch::Tensor rots);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("panel_qr", &panel_qr, "cooperative whole-panel QR (one launch)");
  m.def("secular_roots", &secular_roots,
        "D&C secular-equation roots, one thread per root");
  m.def("tridiag_bisect", &tridiag_bisect,
        "tridiagonal eigenvalues [k_begin, k_end) by Sturm bisection, one "
        "thread per eigenvalue (host loop for CPU tensors)");
  m.def("sturm_count", &sturm_count,
        "number of tridiagonal eigenvalues strictly below each x");
  m.def("tridiag_shifted_solve", &tridiag_shifted_solve,
        "in-place (T - lam[j] I) y_j = x_j by pivoted LU, one thread per "
        "column (host loop for CPU tensors)",
        py::arg("d"), py::arg("e"), py::arg("lam"), py::arg("tol"),
        py::arg("X"), py::arg("work"));
  m.def("matrix_norms", &matrix_norms,
        "one-pass (row sums, column sums, [max, small, medium, big]) of a "
        "local tile storage, masked by global extent and structure",
        py::arg("storage"), py::arg("m"), py::arg("n"), py::arg("gr0"),
        py::arg("grs"), py::arg("gc0"), py::arg("gcs"), py::arg("structure"),
        py::arg("uplo"), py::arg("unit_diag"));
  m.def("trsv_tiles", &trsv_tiles,
        "in-place op(T) x = b for one vector over a local tile storage, "
        "diagonal tiles applied through their inverses",
        py::arg("storage"), py::arg("dinv"), py::arg("x"), py::arg("n"),
        py::arg("uplo"), py::arg("op"));
  m.def("hemv_tiles", &hemv_tiles,
        "y = A x (and yabs = |A| |x| unless yabs is empty) for one vector, A "
        "Hermitian in the uplo triangle of a local tile storage, read once",
        py::arg("storage"), py::arg("x"), py::arg("y"), py::arg("yabs"),
        py::arg("n"), py::arg("uplo"));
  m.def("lu_panel", &lu_panel,
        "in-place LU with partial pivoting of tile column k of a square "
        "local tile storage; one launch per column, pivots and the "
        "zero-pivot record stay on the device",
        py::arg("storage"), py::arg("n"), py::arg("k"), py::arg("ipiv"),
        py::arg("info"));
  m.def("laswp_tiles", &laswp_tiles,
        "row interchanges ipiv[s0:s1] on element columns [c0, c1) of a local "
        "tile storage, one thread per column",
        py::arg("storage"), py::arg("ipiv"), py::arg("s0"), py::arg("s1"),
        py::arg("c0"), py::arg("c1"), py::arg("reverse"));
  m.attr("LU_W") = dlaf::kLuW;
  m.def("hemv_work_size", &dlaf::hemv_work_size,
        "doubles of workspace hemv_tiles uses", py::arg("nt"), py::arg("nb"));
  m.def("sturm_interval", &sturm_interval,
        "(gl, gu, pivmin): widened Gershgorin interval and pivot floor");
  m.def("dc_deflate_scan", &dc_deflate_scan,
        "sequential deflation scan for the D&C merge");
  m.def("band_chase", &band_chase,
        "CPU bulge chasing band->tridiag with reflector recording",
        py::arg("band"), py::arg("b"), py::arg("vstore"), py::arg("offsets"),
        py::arg("nthreads") = 0);
  m.def("bt_apply_group", &bt_apply_group, "whole-group bt window-chain apply");
  m.def("batch_gemm", &batch_gemm,
        "fused batched tile GEMM: C[d] = alpha*op(A[d])op(B[d]) + beta*C[d]");
  m.def("factor_invert_block", &factor_invert_block,
        "fused single-workgroup [factor+]invert of a diagonal block");
  m.def("trtri_lower", &trtri_lower, "lower-triangular block inverse");
  m.def("band_chase_gpu", &band_chase_gpu,
        "GPU bulge chase (persistent wavefront workgroups)");
  m.def("lib_gemm_batched", &lib_gemm_batched,
        "rocBLAS pointer-array batched GEMM (uniform tile shape)");
  m.def("potrf_tile", &potrf_tile,
        "in-place tile Cholesky + diagonal-block inverses");
  m.def("trsm_panel", &trsm_panel,
        "single-launch panel TRSM X <- X * tril(L)^-T over a tile list",
        py::arg("base"), py::arg("tile_offs"), py::arg("L"), py::arg("ldl"),
        py::arg("dinv"), py::arg("mb"), py::arg("nb"), py::arg("ld"),
        py::arg("strip") = 0);
  m.def("trsm_panel_supported", &trsm_panel_supported,
        "whether the tensor's dtype has the single-launch panel TRSM");
  m.attr("POTRF_BSZ") = kPotrfBsz;
}
