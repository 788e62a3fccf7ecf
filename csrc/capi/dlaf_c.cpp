// libdlaf_c.so — C ABI over the dlaf_amd package via an embedded Python
// interpreter (counterpart of the reference's src/c_api/*).
//
// Caller buffers are ScaLAPACK-convention column-major with leading
// dimension ld; they are wrapped as non-owning numpy views (strides
// (itemsize, ld*itemsize)) so the Python side reads and writes the caller's
// memory directly — the flow of the reference's c_api (host matrix ->
// mirror -> algorithm -> copy back, src/c_api/eigensolver/eigensolver.h:30-73).
//
// The package is located relative to this .so (dladdr), overridable with
// DLAF_AMD_PYROOT. Multi-process grids rendezvous via the torchrun-style
// environment — see include/dlaf_c.h.

#include <pybind11/embed.h>
#include <pybind11/numpy.h>

#include <dlfcn.h>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/dlaf_c.h"

namespace py = pybind11;

namespace {

PyThreadState* main_tstate_ = nullptr;
py::module_* capi_ = nullptr;

std::string self_dir() {
  const char* env = std::getenv("DLAF_AMD_PYROOT");
  if (env) return env;
  Dl_info info;
  if (dladdr((void*)&dlaf_initialize, &info) && info.dli_fname) {
    std::string p(info.dli_fname);
    auto pos = p.rfind('/');
    return pos == std::string::npos ? "." : p.substr(0, pos);
  }
  return ".";
}

struct Gil {
  py::gil_scoped_acquire acq;
};

py::object desc_obj(const struct DLAF_descriptor& d);

py::object np_view(int ctx, void* ptr, const struct DLAF_descriptor& d,
                   const char* dtype) {
  Gil g;
  py::dtype dt(dtype);
  const long isz = dt.itemsize();
  // column-major RANK-LOCAL block-cyclic buffer (ScaLAPACK local panel):
  // (local_m, local_n) with stride ld; for a 1x1 grid this is the full matrix
  auto sh = capi_->attr("dlaf_local_shape")(ctx, desc_obj(d)).cast<py::tuple>();
  const long lm = sh[0].cast<long>();
  const long ln = sh[1].cast<long>();
  py::array arr(dt, {lm, ln}, {isz, (long)d.ld * isz}, ptr,
                py::str());  // base handle => non-owning view
  return arr;
}

py::object np_vec(void* ptr, long n, const char* dtype) {
  py::dtype dt(dtype);
  const long isz = dt.itemsize();
  return py::array(dt, {n}, {isz}, ptr, py::str());
}

py::object desc_obj(const struct DLAF_descriptor& d) {
  return capi_->attr("DLAF_descriptor")(d.m, d.n, d.mb, d.nb, d.isrc, d.jsrc,
                                        d.i, d.j, d.ld);
}

int run_inplace(const char* fn, int ctx, char uplo, void* a,
                const struct DLAF_descriptor& d, const char* dtype,
                const char* extra = nullptr) {
  Gil g;
  try {
    auto arr = np_view(ctx, a, d, dtype);
    if (extra)
      return capi_->attr(fn)(ctx, std::string(1, uplo), std::string(1, *extra),
                             arr, desc_obj(d)).cast<int>();
    return capi_->attr(fn)(ctx, std::string(1, uplo), arr, desc_obj(d)).cast<int>();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "dlaf_c: %s failed: %s\n", fn, e.what());
    return -1;
  }
}

int run_eig(int ctx, char uplo, void* a, const struct DLAF_descriptor& da,
            void* w, void* z, const struct DLAF_descriptor& dz,
            const char* adt, const char* wdt, long il, long iu) {
  Gil g;
  try {
    auto arr = np_view(ctx, a, da, adt);
    auto zv = np_view(ctx, z, dz, adt);
    auto wv = np_vec(w, da.n, wdt);
    auto kw = py::dict();
    if (iu >= 0) {
      kw["il"] = il;
      kw["iu"] = iu;
    }
    return capi_->attr("dlaf_hermitian_eigensolver")(
        ctx, std::string(1, uplo), arr, desc_obj(da), wv, zv, desc_obj(dz),
        **kw).cast<int>();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "dlaf_c: eigensolver failed: %s\n", e.what());
    return -1;
  }
}

int run_geig(int ctx, char uplo, void* a, const struct DLAF_descriptor& da,
             void* b, const struct DLAF_descriptor& db, void* w, void* z,
             const struct DLAF_descriptor& dz, const char* adt, const char* wdt,
             bool factorized) {
  Gil g;
  try {
    auto av = np_view(ctx, a, da, adt);
    auto bv = np_view(ctx, b, db, adt);
    auto zv = np_view(ctx, z, dz, adt);
    auto wv = np_vec(w, da.n, wdt);
    return capi_->attr("dlaf_hermitian_generalized_eigensolver")(
        ctx, std::string(1, uplo), av, desc_obj(da), bv, desc_obj(db), wv, zv,
        desc_obj(dz), py::arg("factorized") = factorized).cast<int>();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "dlaf_c: gen eigensolver failed: %s\n", e.what());
    return -1;
  }
}

int run_eigvals(int ctx, char uplo, void* a, const struct DLAF_descriptor& da,
                void* w, const char* adt, const char* wdt) {
  Gil g;
  try {
    auto arr = np_view(ctx, a, da, adt);
    auto wv = np_vec(w, da.n, wdt);
    return capi_->attr("dlaf_hermitian_eigenvalues")(
        ctx, std::string(1, uplo), arr, desc_obj(da), wv).cast<int>();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "dlaf_c: eigenvalues failed: %s\n", e.what());
    return -1;
  }
}

int run_geigvals(int ctx, char uplo, void* a, const struct DLAF_descriptor& da,
                 void* b, const struct DLAF_descriptor& db, void* w,
                 const char* adt, const char* wdt) {
  Gil g;
  try {
    auto av = np_view(ctx, a, da, adt);
    auto bv = np_view(ctx, b, db, adt);
    auto wv = np_vec(w, da.n, wdt);
    return capi_->attr("dlaf_hermitian_generalized_eigenvalues")(
        ctx, std::string(1, uplo), av, desc_obj(da), bv, desc_obj(db), wv)
        .cast<int>();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "dlaf_c: gen eigenvalues failed: %s\n", e.what());
    return -1;
  }
}

// norm of the leading m x n part of the caller's (read-only) buffer
double run_norm(int ctx, char norm, char structure, char uplo, char diag,
                int m, int n, const void* a, const struct DLAF_descriptor& d,
                const char* dtype) {
  Gil g;
  try {
    auto arr = np_view(ctx, const_cast<void*>(a), d, dtype);
    struct DLAF_descriptor sub = d;
    sub.m = m;
    sub.n = n;
    return capi_->attr("dlaf_matrix_norm")(
        ctx, std::string(1, norm), std::string(1, structure),
        std::string(1, uplo), std::string(1, diag), arr, desc_obj(sub))
        .cast<double>();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "dlaf_c: matrix norm failed: %s\n", e.what());
    return std::nan("");
  }
}

// rcond estimates of the leading n x n part of the caller's (read-only)
// buffer: trcon when norm != 0, else pocon with the given anorm
int run_rcond(int ctx, char norm, char uplo, char diag, int n, double anorm,
              const void* a, const struct DLAF_descriptor& d,
              const char* dtype, double* rcond) {
  Gil g;
  try {
    auto arr = np_view(ctx, const_cast<void*>(a), d, dtype);
    struct DLAF_descriptor sub = d;
    sub.m = sub.n = n;
    if (norm)
      *rcond = capi_->attr("dlaf_triangular_rcond")(
          ctx, std::string(1, norm), std::string(1, uplo),
          std::string(1, diag), arr, desc_obj(sub)).cast<double>();
    else
      *rcond = capi_->attr("dlaf_cholesky_rcond")(
          ctx, std::string(1, uplo), arr, desc_obj(sub), anorm).cast<double>();
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "dlaf_c: condition estimate failed: %s\n", e.what());
    *rcond = std::nan("");
    return -1;
  }
}

int run_potrs(int ctx, char uplo, int n, int nrhs, const void* a,
              const struct DLAF_descriptor& da, void* b,
              const struct DLAF_descriptor& db, const char* dtype) {
  Gil g;
  try {
    auto av = np_view(ctx, const_cast<void*>(a), da, dtype);
    auto bv = np_view(ctx, b, db, dtype);
    struct DLAF_descriptor sa = da, sb = db;
    sa.m = sa.n = n;
    sb.m = n;
    sb.n = nrhs;
    return capi_->attr("dlaf_cholesky_solve")(
        ctx, std::string(1, uplo), av, desc_obj(sa), bv, desc_obj(sb))
        .cast<int>();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "dlaf_c: cholesky solve failed: %s\n", e.what());
    return -1;
  }
}

// the leading m x n part of a descriptor
struct DLAF_descriptor leading(struct DLAF_descriptor d, int m, int n) {
  d.m = m;
  d.n = n;
  return d;
}

int run_porfs(int ctx, char uplo, int n, int nrhs, const void* a,
              const struct DLAF_descriptor& da, const void* af,
              const struct DLAF_descriptor& daf, const void* b,
              const struct DLAF_descriptor& db, void* x,
              const struct DLAF_descriptor& dx, double* ferr, double* berr,
              const char* dtype) {
  Gil g;
  try {
    auto av = np_view(ctx, const_cast<void*>(a), da, dtype);
    auto fv = np_view(ctx, const_cast<void*>(af), daf, dtype);
    auto bv = np_view(ctx, const_cast<void*>(b), db, dtype);
    auto xv = np_view(ctx, x, dx, dtype);
    return capi_->attr("dlaf_cholesky_refine")(
        ctx, std::string(1, uplo), av, desc_obj(leading(da, n, n)), fv,
        desc_obj(leading(daf, n, n)), bv, desc_obj(leading(db, n, nrhs)), xv,
        desc_obj(leading(dx, n, nrhs)), np_vec(ferr, nrhs, "float64"),
        np_vec(berr, nrhs, "float64")).cast<int>();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "dlaf_c: cholesky refine failed: %s\n", e.what());
    return -1;
  }
}

int run_sposv(int ctx, char uplo, int n, int nrhs, const void* a,
              const struct DLAF_descriptor& da, const void* b,
              const struct DLAF_descriptor& db, void* x,
              const struct DLAF_descriptor& dx, int* iter,
              const char* dtype) {
  Gil g;
  try {
    auto av = np_view(ctx, const_cast<void*>(a), da, dtype);
    auto bv = np_view(ctx, const_cast<void*>(b), db, dtype);
    auto xv = np_view(ctx, x, dx, dtype);
    auto out = capi_->attr("dlaf_cholesky_solve_mixed")(
        ctx, std::string(1, uplo), av, desc_obj(leading(da, n, n)), bv,
        desc_obj(leading(db, n, nrhs)), xv, desc_obj(leading(dx, n, nrhs)))
        .cast<py::tuple>();
    *iter = out[0].cast<int>();
    return out[1].cast<int>();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "dlaf_c: mixed cholesky solve failed: %s\n",
                 e.what());
    *iter = 0;
    return -1;
  }
}

// LU of the leading n x n part in place; ipiv[n] gets 1-based global rows
int run_getrf(int ctx, int n, void* a, const struct DLAF_descriptor& da,
              int* ipiv, const char* dtype) {
  Gil g;
  try {
    auto av = np_view(ctx, a, da, dtype);
    return capi_->attr("dlaf_lu_factorization")(
        ctx, av, desc_obj(leading(da, n, n)), np_vec(ipiv, n, "int32"))
        .cast<int>();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "dlaf_c: lu factorization failed: %s\n", e.what());
    return -1;
  }
}

int run_getrs(int ctx, char trans, int n, int nrhs, const void* a,
              const struct DLAF_descriptor& da, const int* ipiv, void* b,
              const struct DLAF_descriptor& db, const char* dtype) {
  Gil g;
  try {
    auto av = np_view(ctx, const_cast<void*>(a), da, dtype);
    auto bv = np_view(ctx, b, db, dtype);
    return capi_->attr("dlaf_lu_solve")(
        ctx, std::string(1, trans), av, desc_obj(leading(da, n, n)),
        np_vec(const_cast<int*>(ipiv), n, "int32"), bv,
        desc_obj(leading(db, n, nrhs))).cast<int>();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "dlaf_c: lu solve failed: %s\n", e.what());
    return -1;
  }
}

int run_gecon(int ctx, char norm, int n, const void* a,
              const struct DLAF_descriptor& da, double anorm, double* rcond,
              const char* dtype) {
  Gil g;
  try {
    auto av = np_view(ctx, const_cast<void*>(a), da, dtype);
    *rcond = capi_->attr("dlaf_lu_rcond")(
        ctx, std::string(1, norm), av, desc_obj(leading(da, n, n)), anorm)
        .cast<double>();
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "dlaf_c: lu condition estimate failed: %s\n",
                 e.what());
    *rcond = std::nan("");
    return -1;
  }
}

struct DLAF_descriptor from_sl(int n, const int d[9], int m = -1) {
  struct DLAF_descriptor out;
  out.m = m >= 0 ? m : d[2];
  out.n = d[3];
  out.mb = d[4];
  out.nb = d[5];
  out.isrc = d[6];
  out.jsrc = d[7];
  out.i = 1;
  out.j = 1;
  out.ld = d[8];
  (void)n;
  return out;
}

int sl_ctx_ = -1;

int sl_grid() {  // lazy local 1x1 context for the ScaLAPACK shims
  if (sl_ctx_ < 0) {
    dlaf_initialize(0, nullptr);
    sl_ctx_ = dlaf_create_grid(1, 1, 'R');
  }
  return sl_ctx_;
}

}  // namespace

extern "C" {

int dlaf_initialize(int, const char* const*) {
  if (capi_) return 0;
  if (!Py_IsInitialized()) {
    py::initialize_interpreter();
    {
      auto sys = py::module_::import("sys");
      sys.attr("path").attr("insert")(0, self_dir());
    }
    try {
      capi_ = new py::module_(py::module_::import("dlaf_amd.capi"));
    } catch (const std::exception& e) {
      std::fprintf(stderr, "dlaf_c: cannot import dlaf_amd.capi: %s\n", e.what());
      return -1;
    }
    main_tstate_ = PyEval_SaveThread();  // release GIL; calls re-acquire
  } else {
    py::gil_scoped_acquire g;
    auto sys = py::module_::import("sys");
    sys.attr("path").attr("insert")(0, self_dir());
    capi_ = new py::module_(py::module_::import("dlaf_amd.capi"));
  }
  return 0;
}

void dlaf_finalize(void) {
  // keep the interpreter alive: torch/HIP teardown from a foreign main is
  // not worth the risk, and the reference's dlaf_finalize is also a no-op
  // when pika was externally started.
}

int dlaf_create_grid(int nprow, int npcol, char order) {
  // Multi-process grids: the Python side initializes torch.distributed
  // (RCCL on GPU, gloo on CPU) from the torchrun-style launcher env
  // (RANK/WORLD_SIZE/MASTER_ADDR/MASTER_PORT); nprow*npcol must equal
  // WORLD_SIZE. Reference counterpart: src/c_api/grid.cpp (MPI_Comm in,
  // CommunicatorGrid out) — the rendezvous here is the launcher env
  // instead of an MPI communicator.
  Gil g;
  try {
    return capi_->attr("dlaf_create_grid")(nprow, npcol, std::string(1, order))
        .cast<int>();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "dlaf_c: dlaf_create_grid failed: %s\n", e.what());
    return -1;
  }
}

void dlaf_free_grid(int ctx) {
  Gil g;
  capi_->attr("dlaf_free_grid")(ctx);
}

#define CHOL(suf, ctype, npdt)                                                 \
  int dlaf_cholesky_factorization_##suf(int ctx, char uplo, ctype* a,          \
                                        struct DLAF_descriptor d) {            \
    return run_inplace("dlaf_cholesky_factorization", ctx, uplo, a, d, npdt);  \
  }                                                                            \
  int dlaf_inverse_from_cholesky_factor_##suf(int ctx, char uplo, ctype* a,    \
                                              struct DLAF_descriptor d) {      \
    return run_inplace("dlaf_inverse_from_cholesky_factor", ctx, uplo, a, d,   \
                       npdt);                                                  \
  }

CHOL(s, float, "float32")
CHOL(d, double, "float64")
CHOL(c, dlaf_complex_c, "complex64")
CHOL(z, dlaf_complex_z, "complex128")
#undef CHOL

int dlaf_symmetric_eigensolver_s(int ctx, char uplo, float* a,
                                 struct DLAF_descriptor da, float* w, float* z,
                                 struct DLAF_descriptor dz) {
  return run_eig(ctx, uplo, a, da, w, z, dz, "float32", "float32", 0, -1);
}
int dlaf_symmetric_eigensolver_d(int ctx, char uplo, double* a,
                                 struct DLAF_descriptor da, double* w, double* z,
                                 struct DLAF_descriptor dz) {
  return run_eig(ctx, uplo, a, da, w, z, dz, "float64", "float64", 0, -1);
}
int dlaf_hermitian_eigensolver_c(int ctx, char uplo, dlaf_complex_c* a,
                                 struct DLAF_descriptor da, float* w,
                                 dlaf_complex_c* z, struct DLAF_descriptor dz) {
  return run_eig(ctx, uplo, a, da, w, z, dz, "complex64", "float32", 0, -1);
}
int dlaf_hermitian_eigensolver_z(int ctx, char uplo, dlaf_complex_z* a,
                                 struct DLAF_descriptor da, double* w,
                                 dlaf_complex_z* z, struct DLAF_descriptor dz) {
  return run_eig(ctx, uplo, a, da, w, z, dz, "complex128", "float64", 0, -1);
}
int dlaf_symmetric_eigensolver_partial_spectrum_d(
    int ctx, char uplo, double* a, struct DLAF_descriptor da, double* w,
    double* z, struct DLAF_descriptor dz, long il, long iu) {
  return run_eig(ctx, uplo, a, da, w, z, dz, "float64", "float64", il, iu);
}
int dlaf_hermitian_eigensolver_partial_spectrum_z(
    int ctx, char uplo, dlaf_complex_z* a, struct DLAF_descriptor da, double* w,
    dlaf_complex_z* z, struct DLAF_descriptor dz, long il, long iu) {
  return run_eig(ctx, uplo, a, da, w, z, dz, "complex128", "float64", il, iu);
}

int dlaf_symmetric_generalized_eigensolver_d(
    int ctx, char uplo, double* a, struct DLAF_descriptor da, double* b,
    struct DLAF_descriptor db, double* w, double* z, struct DLAF_descriptor dz) {
  return run_geig(ctx, uplo, a, da, b, db, w, z, dz, "float64", "float64", false);
}
int dlaf_symmetric_generalized_eigensolver_factorized_d(
    int ctx, char uplo, double* a, struct DLAF_descriptor da, double* b,
    struct DLAF_descriptor db, double* w, double* z, struct DLAF_descriptor dz) {
  return run_geig(ctx, uplo, a, da, b, db, w, z, dz, "float64", "float64", true);
}
int dlaf_hermitian_generalized_eigensolver_z(
    int ctx, char uplo, dlaf_complex_z* a, struct DLAF_descriptor da,
    dlaf_complex_z* b, struct DLAF_descriptor db, double* w, dlaf_complex_z* z,
    struct DLAF_descriptor dz) {
  return run_geig(ctx, uplo, a, da, b, db, w, z, dz, "complex128", "float64",
                  false);
}
int dlaf_hermitian_generalized_eigensolver_factorized_z(
    int ctx, char uplo, dlaf_complex_z* a, struct DLAF_descriptor da,
    dlaf_complex_z* b, struct DLAF_descriptor db, double* w, dlaf_complex_z* z,
    struct DLAF_descriptor dz) {
  return run_geig(ctx, uplo, a, da, b, db, w, z, dz, "complex128", "float64",
                  true);
}

int dlaf_symmetric_eigenvalues_d(int ctx, char uplo, double* a,
                                 struct DLAF_descriptor da, double* w) {
  return run_eigvals(ctx, uplo, a, da, w, "float64", "float64");
}
int dlaf_hermitian_eigenvalues_z(int ctx, char uplo, dlaf_complex_z* a,
                                 struct DLAF_descriptor da, double* w) {
  return run_eigvals(ctx, uplo, a, da, w, "complex128", "float64");
}
int dlaf_symmetric_generalized_eigenvalues_d(
    int ctx, char uplo, double* a, struct DLAF_descriptor da, double* b,
    struct DLAF_descriptor db, double* w) {
  return run_geigvals(ctx, uplo, a, da, b, db, w, "float64", "float64");
}
int dlaf_hermitian_generalized_eigenvalues_z(
    int ctx, char uplo, dlaf_complex_z* a, struct DLAF_descriptor da,
    dlaf_complex_z* b, struct DLAF_descriptor db, double* w) {
  return run_geigvals(ctx, uplo, a, da, b, db, w, "complex128", "float64");
}

#define SL_POTRF(name, suf, ctype)                                            \
  void name(char uplo, int n, ctype* a, int ia, int ja, const int desca[9],    \
            int* info) {                                                       \
    (void)ia;                                                                  \
    (void)ja;                                                                  \
    *info = dlaf_cholesky_factorization_##suf(sl_grid(), uplo, a,              \
                                              from_sl(n, desca));              \
  }

SL_POTRF(dlaf_pdpotrf, d, double)
SL_POTRF(dlaf_pspotrf, s, float)
SL_POTRF(dlaf_pzpotrf, z, dlaf_complex_z)
SL_POTRF(dlaf_pcpotrf, c, dlaf_complex_c)
#undef SL_POTRF

void dlaf_pdpotri(char uplo, int n, double* a, int ia, int ja,
                  const int desca[9], int* info) {
  (void)ia;
  (void)ja;
  *info = dlaf_inverse_from_cholesky_factor_d(sl_grid(), uplo, a,
                                              from_sl(n, desca));
}

void dlaf_pdsyevd(char uplo, int n, double* a, int ia, int ja,
                  const int desca[9], double* w, double* z, int iz, int jz,
                  const int descz[9], int* info) {
  (void)ia; (void)ja; (void)iz; (void)jz;
  *info = dlaf_symmetric_eigensolver_d(sl_grid(), uplo, a, from_sl(n, desca), w,
                                       z, from_sl(n, descz));
}

void dlaf_pzheevd(char uplo, int n, dlaf_complex_z* a, int ia, int ja,
                  const int desca[9], double* w, dlaf_complex_z* z, int iz,
                  int jz, const int descz[9], int* info) {
  (void)ia; (void)ja; (void)iz; (void)jz;
  *info = dlaf_hermitian_eigensolver_z(sl_grid(), uplo, a, from_sl(n, desca), w,
                                       z, from_sl(n, descz));
}

void dlaf_pdsygvd(char uplo, int n, double* a, int ia, int ja,
                  const int desca[9], double* b, int ib, int jb,
                  const int descb[9], double* w, double* z, int iz, int jz,
                  const int descz[9], int* info) {
  (void)ia; (void)ja; (void)ib; (void)jb; (void)iz; (void)jz;
  *info = dlaf_symmetric_generalized_eigensolver_d(
      sl_grid(), uplo, a, from_sl(n, desca), b, from_sl(n, descb), w, z,
      from_sl(n, descz));
}

double dlaf_pdlange(char norm, int m, int n, const double* a, int ia, int ja,
                    const int desca[9]) {
  (void)ia; (void)ja;
  return run_norm(sl_grid(), norm, 'G', 'L', 'N', m, n, a, from_sl(n, desca),
                  "float64");
}
double dlaf_pzlange(char norm, int m, int n, const dlaf_complex_z* a, int ia,
                    int ja, const int desca[9]) {
  (void)ia; (void)ja;
  return run_norm(sl_grid(), norm, 'G', 'L', 'N', m, n, a, from_sl(n, desca),
                  "complex128");
}
double dlaf_pdlansy(char norm, char uplo, int n, const double* a, int ia,
                    int ja, const int desca[9]) {
  (void)ia; (void)ja;
  return run_norm(sl_grid(), norm, 'H', uplo, 'N', n, n, a, from_sl(n, desca),
                  "float64");
}
double dlaf_pzlanhe(char norm, char uplo, int n, const dlaf_complex_z* a,
                    int ia, int ja, const int desca[9]) {
  (void)ia; (void)ja;
  return run_norm(sl_grid(), norm, 'H', uplo, 'N', n, n, a, from_sl(n, desca),
                  "complex128");
}
double dlaf_pdlantr(char norm, char uplo, char diag, int m, int n,
                    const double* a, int ia, int ja, const int desca[9]) {
  (void)ia; (void)ja;
  return run_norm(sl_grid(), norm, 'T', uplo, diag, m, n, a,
                  from_sl(n, desca), "float64");
}

void dlaf_pdpocon(char uplo, int n, const double* a, int ia, int ja,
                  const int desca[9], double anorm, double* rcond, int* info) {
  (void)ia; (void)ja;
  *info = run_rcond(sl_grid(), 0, uplo, 'N', n, anorm, a, from_sl(n, desca),
                    "float64", rcond);
}
void dlaf_pzpocon(char uplo, int n, const dlaf_complex_z* a, int ia, int ja,
                  const int desca[9], double anorm, double* rcond, int* info) {
  (void)ia; (void)ja;
  *info = run_rcond(sl_grid(), 0, uplo, 'N', n, anorm, a, from_sl(n, desca),
                    "complex128", rcond);
}
void dlaf_pdtrcon(char norm, char uplo, char diag, int n, const double* a,
                  int ia, int ja, const int desca[9], double* rcond,
                  int* info) {
  (void)ia; (void)ja;
  *info = run_rcond(sl_grid(), norm, uplo, diag, n, 0.0, a, from_sl(n, desca),
                    "float64", rcond);
}
void dlaf_pztrcon(char norm, char uplo, char diag, int n,
                  const dlaf_complex_z* a, int ia, int ja, const int desca[9],
                  double* rcond, int* info) {
  (void)ia; (void)ja;
  *info = run_rcond(sl_grid(), norm, uplo, diag, n, 0.0, a, from_sl(n, desca),
                    "complex128", rcond);
}
void dlaf_pdpotrs(char uplo, int n, int nrhs, const double* a, int ia, int ja,
                  const int desca[9], double* b, int ib, int jb,
                  const int descb[9], int* info) {
  (void)ia; (void)ja; (void)ib; (void)jb;
  *info = run_potrs(sl_grid(), uplo, n, nrhs, a, from_sl(n, desca), b,
                    from_sl(nrhs, descb), "float64");
}

#define DLAF_PORFS(name, T, dtype)                                            \
  void name(char uplo, int n, int nrhs, const T* a, int ia, int ja,           \
            const int desca[9], const T* af, int iaf, int jaf,                \
            const int descaf[9], const T* b, int ib, int jb,                  \
            const int descb[9], T* x, int ix, int jx, const int descx[9],     \
            double* ferr, double* berr, int* info) {                          \
    (void)ia; (void)ja; (void)iaf; (void)jaf;                                 \
    (void)ib; (void)jb; (void)ix; (void)jx;                                   \
    *info = run_porfs(sl_grid(), uplo, n, nrhs, a, from_sl(n, desca), af,     \
                      from_sl(n, descaf), b, from_sl(nrhs, descb), x,         \
                      from_sl(nrhs, descx), ferr, berr, dtype);               \
  }
DLAF_PORFS(dlaf_pdporfs, double, "float64")
DLAF_PORFS(dlaf_pzporfs, dlaf_complex_z, "complex128")
#undef DLAF_PORFS

#define DLAF_SPOSV(name, T, dtype)                                            \
  void name(char uplo, int n, int nrhs, const T* a, int ia, int ja,           \
            const int desca[9], const T* b, int ib, int jb,                   \
            const int descb[9], T* x, int ix, int jx, const int descx[9],     \
            int* iter, int* info) {                                           \
    (void)ia; (void)ja; (void)ib; (void)jb; (void)ix; (void)jx;               \
    *info = run_sposv(sl_grid(), uplo, n, nrhs, a, from_sl(n, desca), b,      \
                      from_sl(nrhs, descb), x, from_sl(nrhs, descx), iter,    \
                      dtype);                                                 \
  }
DLAF_SPOSV(dlaf_pdsposv, double, "float64")
DLAF_SPOSV(dlaf_pzcposv, dlaf_complex_z, "complex128")
#undef DLAF_SPOSV

#define DLAF_GETRF(name, T, dtype)                                            \
  void name(int m, int n, T* a, int ia, int ja, const int desca[9],           \
            int* ipiv, int* info) {                                           \
    (void)ia; (void)ja;                                                       \
    *info = m == n ? run_getrf(sl_grid(), n, a, from_sl(n, desca), ipiv,      \
                               dtype)                                         \
                   : -1;                                                      \
  }
DLAF_GETRF(dlaf_pdgetrf, double, "float64")
DLAF_GETRF(dlaf_pzgetrf, dlaf_complex_z, "complex128")
#undef DLAF_GETRF

#define DLAF_GETRS(name, T, dtype)                                            \
  void name(char trans, int n, int nrhs, const T* a, int ia, int ja,          \
            const int desca[9], const int* ipiv, T* b, int ib, int jb,        \
            const int descb[9], int* info) {                                  \
    (void)ia; (void)ja; (void)ib; (void)jb;                                   \
    *info = run_getrs(sl_grid(), trans, n, nrhs, a, from_sl(n, desca), ipiv,  \
                      b, from_sl(nrhs, descb), dtype);                        \
  }
DLAF_GETRS(dlaf_pdgetrs, double, "float64")
DLAF_GETRS(dlaf_pzgetrs, dlaf_complex_z, "complex128")
#undef DLAF_GETRS

void dlaf_pdgecon(char norm, int n, const double* a, int ia, int ja,
                  const int desca[9], double anorm, double* rcond, int* info) {
  (void)ia; (void)ja;
  *info = run_gecon(sl_grid(), norm, n, a, from_sl(n, desca), anorm, rcond,
                    "float64");
}

void dlaf_pdgesv(int n, int nrhs, double* a, int ia, int ja,
                 const int desca[9], int* ipiv, double* b, int ib, int jb,
                 const int descb[9], int* info) {
  (void)ia; (void)ja; (void)ib; (void)jb;
  *info = run_getrf(sl_grid(), n, a, from_sl(n, desca), ipiv, "float64");
  if (*info == 0)
    *info = run_getrs(sl_grid(), 'N', n, nrhs, a, from_sl(n, desca), ipiv, b,
                      from_sl(nrhs, descb), "float64");
}

}  // extern "C"
