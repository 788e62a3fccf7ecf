// Fused batched tile GEMM for CDNA4 (gfx950) on fp64/fp32 MFMA: the entry
// points (dlaf::gemm_tiles) and the guarded register-staged kernels.
//
// One kernel launch processes a LIST of tile-triples (GemmDesc): this is how a
// whole trailing update (SYRK/HERK sweep), panel solve, or back-transform step
// becomes a single launch with enough workgroups to fill 256 CUs.
//
// Layout of the GEMM layer:
//   gemm_common.h      Mfma<T>, v4d/v4f, xcd_remap
//   gemm_tiles_v2.hip  glds kernels: full tiles, C not aliasing A (hot phases)
//   gemm_tiles.hip     this file: gemm_tiles() tries v2, else launches the
//                      kernels below, which take edge shapes (M, N, K not
//                      multiples of the block) and in-place panel applies.
// Each workgroup here computes one BMxBN block of one C tile:
//   real    (f64/f32): BM=128, BN=64|128, BK=16, 4 waves, 4 x BN/32 frags of
//                      mfma_{f64,f32}_16x16x4.
//   complex (c128/c64): BM=BN=64, BK=16, 4 waves, 32x32 per wave, 2x2 frags,
//                      4 MFMA per fragment pair (re/im cross terms).
//
// K-tiling pipeline: single LDS buffer; global loads of K-step s+1 issue while
// MFMAs of step s run from LDS (register staging, write-after-barrier — the
// pattern cdna_hip_programming.md §5 recommends when not using glds).
//
// Operand layout: row-major tiles. op(A) is resolved during LDS staging, so the
// inner loop is layout-independent. Out-of-range rows/cols (edge blocks when
// M,N,K are not multiples of the block sizes) stage zeros and stores are
// guarded, so arbitrary sizes are supported.
#include "gemm_common.h"

namespace {

// ---------------- real kernel ----------------

// Geometry: block = BM x BN of C, BK-deep K steps, 4 waves.
//   BN = 64 (default): wave tile 64x32, 8 accumulator fragments (64 regs) ->
//        fits 2 waves/SIMD (VGPR+AGPR <= 256), latency hidden by the partner.
//   BN = 128 ("in-place-safe"): wave tile 64x64 -> a single column block spans
//        the whole N of a panel-apply, making X = X * dinv^H safe in place
//        (every workgroup reads all of its A rows before writing them).
template <typename T, int OPA, int OPB, int BN, bool GUARD>
__launch_bounds__(256) __global__ void gemm_tiles_k(
    const GemmDesc* __restrict__ descs, const T* __restrict__ A,
    const T* __restrict__ B, T* __restrict__ C, int M, int N, int K, int lda,
    int ldb, int ldc, T alpha, T beta, int mblocks, int nblocks) {
  constexpr int BM = 128, BK = 16;
  constexpr int LA = BM * BK / 256;  // elements staged per thread (A)
  constexpr int LB = BK * BN / 256;
  constexpr int WCW = BN / 2;        // wave tile columns
  constexpr int NFRAG = WCW / 16;
  using acc_t = typename Mfma<T>::acc_t;

  __shared__ T As[1][BM][BK + 1];
  __shared__ T Bs[1][BK][BN + 2];

  const int wg = blockIdx.x;
  const int per_desc = mblocks * nblocks;
  const GemmDesc d = descs[wg / per_desc];
  const int rem = wg % per_desc;
  const int bi = rem / nblocks, bj = rem % nblocks;
  const int i0 = bi * BM, j0 = bj * BN;

  const int tid = threadIdx.x;
  const int lane = tid & 63, w = tid >> 6;
  const int wrow = (w >> 1) * 64, wcol = (w & 1) * WCW;
  const int li = lane & 15, lk = lane >> 4;

  const int steps_per_tile = (K + BK - 1) / BK;
  const int total_steps = (int)d.ktiles * steps_per_tile;

  acc_t acc[4][NFRAG];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < NFRAG; ++b) acc[a][b] = {0, 0, 0, 0};

  T ra[LA], rb[LB];

  auto load_step = [&](int s, T* va, T* vb) {
    const int kt = s / steps_per_tile;
    const int k0 = (s % steps_per_tile) * BK;
    const T* Ab = A + d.a_off + (int64_t)kt * d.a_kstride;
    const T* Bb = B + d.b_off + (int64_t)kt * d.b_kstride;
#pragma unroll
    for (int j = 0; j < LA; ++j) {
      const int e = j * 256 + tid;
      int i, k;
      if (OPA == OP_N) {
        i = e / BK;
        k = e % BK;
      } else {
        k = e / BM;
        i = e % BM;
      }
      const int gi = i0 + i, gk = k0 + k;
      if constexpr (GUARD) {
        T v = T(0);
        if (gi < M && gk < K)
          v = (OPA == OP_N) ? Ab[(int64_t)gi * lda + gk] : Ab[(int64_t)gk * lda + gi];
        va[j] = v;
      } else {
        va[j] = (OPA == OP_N) ? Ab[(int64_t)gi * lda + gk] : Ab[(int64_t)gk * lda + gi];
      }
    }
#pragma unroll
    for (int j = 0; j < LB; ++j) {
      const int e = j * 256 + tid;
      int k, c;
      if (OPB == OP_N) {
        k = e / BN;
        c = e % BN;
      } else {
        c = e / BK;
        k = e % BK;
      }
      const int gk = k0 + k, gc = j0 + c;
      if constexpr (GUARD) {
        T v = T(0);
        if (gk < K && gc < N)
          v = (OPB == OP_N) ? Bb[(int64_t)gk * ldb + gc] : Bb[(int64_t)gc * ldb + gk];
        vb[j] = v;
      } else {
        vb[j] = (OPB == OP_N) ? Bb[(int64_t)gk * ldb + gc] : Bb[(int64_t)gc * ldb + gk];
      }
    }
  };

  auto stage = [&](int buf, T* va, T* vb) {
#pragma unroll
    for (int j = 0; j < LA; ++j) {
      const int e = j * 256 + tid;
      int i, k;
      if (OPA == OP_N) {
        i = e / BK;
        k = e % BK;
      } else {
        k = e / BM;
        i = e % BM;
      }
      As[buf][i][k] = va[j];
    }
#pragma unroll
    for (int j = 0; j < LB; ++j) {
      const int e = j * 256 + tid;
      int k, c;
      if (OPB == OP_N) {
        k = e / BN;
        c = e % BN;
      } else {
        c = e / BK;
        k = e % BK;
      }
      Bs[buf][k][c] = vb[j];
    }
  };
  auto compute = [&](int buf) {
    // software-pipelined fragment loads: ds_reads for step ks+1 issue while
    // the MFMAs of step ks run (MfmaUtil measured 57% without this — the
    // read->mma dependency chain stalls the MAI pipe between steps)
    T af[2][4], bf[2][NFRAG];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
      af[0][mi] = As[buf][wrow + mi * 16 + li][lk];
#pragma unroll
    for (int ni = 0; ni < NFRAG; ++ni)
      bf[0][ni] = Bs[buf][lk][wcol + ni * 16 + li];
#pragma unroll
    for (int ks = 0; ks < BK / 4; ++ks) {
      const int cur = ks & 1;
      if (ks + 1 < BK / 4) {
        const int nxt = 1 - cur;
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
          af[nxt][mi] = As[buf][wrow + mi * 16 + li][(ks + 1) * 4 + lk];
#pragma unroll
        for (int ni = 0; ni < NFRAG; ++ni)
          bf[nxt][ni] = Bs[buf][(ks + 1) * 4 + lk][wcol + ni * 16 + li];
      }
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < NFRAG; ++ni)
          acc[mi][ni] = Mfma<T>::mma(af[cur][mi], bf[cur][ni], acc[mi][ni]);
    }
  };

  load_step(0, ra, rb);

  for (int s = 0; s < total_steps; ++s) {
    stage(0, ra, rb);
    __syncthreads();
    if (s + 1 < total_steps) load_step(s + 1, ra, rb);  // overlaps MFMA below
    compute(0);
    __syncthreads();  // LDS reuse barrier
  }

  // epilogue: C = alpha*acc + beta*C
  T* Cb = C + d.c_off;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < NFRAG; ++ni) {
      const acc_t v = acc[mi][ni];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = i0 + wrow + mi * 16 + Mfma<T>::acc_row(lk, r);
        const int col = j0 + wcol + ni * 16 + li;
        if (!GUARD || (row < M && col < N)) {
          const int64_t off = (int64_t)row * ldc + col;
          T out = alpha * (T)v[r];
          if (beta != T(0)) out += beta * Cb[off];
          Cb[off] = out;
        }
      }
    }
}

// ---------------- complex kernel ----------------
// Interleaved (re, im); offsets/strides from the descriptor are in COMPLEX
// elements. Conjugation (OP_C) is applied to the staged fragments.

template <typename T, int OPA, int OPB>
__launch_bounds__(256) __global__ void gemm_tiles_cplx_k(
    const GemmDesc* __restrict__ descs, const T* __restrict__ A,
    const T* __restrict__ B, T* __restrict__ C, int M, int N, int K, int lda,
    int ldb, int ldc, T alpha_re, T alpha_im, T beta_re, T beta_im, int mblocks,
    int nblocks) {
  constexpr int BM = 64, BN = 64, BK = 16;
  constexpr int LA = BM * BK / 256;  // complex elements per thread
  constexpr int LB = BK * BN / 256;
  using acc_t = typename Mfma<T>::acc_t;

  __shared__ T Asr[BM][BK + 1];
  __shared__ T Asi[BM][BK + 1];
  __shared__ T Bsr[BK][BN + 2];
  __shared__ T Bsi[BK][BN + 2];

  const int wg = blockIdx.x;
  const int per_desc = mblocks * nblocks;
  const GemmDesc d = descs[wg / per_desc];
  const int rem = wg % per_desc;
  const int bi = rem / nblocks, bj = rem % nblocks;
  const int i0 = bi * BM, j0 = bj * BN;

  const int tid = threadIdx.x;
  const int lane = tid & 63, w = tid >> 6;
  const int wrow = (w >> 1) * 32, wcol = (w & 1) * 32;
  const int li = lane & 15, lk = lane >> 4;

  const int steps_per_tile = (K + BK - 1) / BK;
  const int total_steps = (int)d.ktiles * steps_per_tile;

  acc_t accr[2][2], acci[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      accr[a][b] = {0, 0, 0, 0};
      acci[a][b] = {0, 0, 0, 0};
    }

  T rar[LA], rai[LA], rbr[LB], rbi[LB];

  auto load_step = [&](int s) {
    const int kt = s / steps_per_tile;
    const int k0 = (s % steps_per_tile) * BK;
    const T* Ab = A + 2 * (d.a_off + (int64_t)kt * d.a_kstride);
    const T* Bb = B + 2 * (d.b_off + (int64_t)kt * d.b_kstride);
#pragma unroll
    for (int j = 0; j < LA; ++j) {
      const int e = j * 256 + tid;
      int i, k;
      if (OPA == OP_N) {
        i = e / BK;
        k = e % BK;
      } else {
        k = e / BM;
        i = e % BM;
      }
      const int gi = i0 + i, gk = k0 + k;
      T vr = T(0), vi = T(0);
      if (gi < M && gk < K) {
        const int64_t off =
            (OPA == OP_N) ? ((int64_t)gi * lda + gk) : ((int64_t)gk * lda + gi);
        vr = Ab[2 * off];
        vi = Ab[2 * off + 1];
      }
      if (OPA == OP_C) vi = -vi;
      rar[j] = vr;
      rai[j] = vi;
    }
#pragma unroll
    for (int j = 0; j < LB; ++j) {
      const int e = j * 256 + tid;
      int k, c;
      if (OPB == OP_N) {
        k = e / BN;
        c = e % BN;
      } else {
        c = e / BK;
        k = e % BK;
      }
      const int gk = k0 + k, gc = j0 + c;
      T vr = T(0), vi = T(0);
      if (gk < K && gc < N) {
        const int64_t off =
            (OPB == OP_N) ? ((int64_t)gk * ldb + gc) : ((int64_t)gc * ldb + gk);
        vr = Bb[2 * off];
        vi = Bb[2 * off + 1];
      }
      if (OPB == OP_C) vi = -vi;
      rbr[j] = vr;
      rbi[j] = vi;
    }
  };

  load_step(0);

  for (int s = 0; s < total_steps; ++s) {
#pragma unroll
    for (int j = 0; j < LA; ++j) {
      const int e = j * 256 + tid;
      int i, k;
      if (OPA == OP_N) {
        i = e / BK;
        k = e % BK;
      } else {
        k = e / BM;
        i = e % BM;
      }
      Asr[i][k] = rar[j];
      Asi[i][k] = rai[j];
    }
#pragma unroll
    for (int j = 0; j < LB; ++j) {
      const int e = j * 256 + tid;
      int k, c;
      if (OPB == OP_N) {
        k = e / BN;
        c = e % BN;
      } else {
        c = e / BK;
        k = e % BK;
      }
      Bsr[k][c] = rbr[j];
      Bsi[k][c] = rbi[j];
    }
    __syncthreads();
    if (s + 1 < total_steps) load_step(s + 1);  // overlaps MFMA below

#pragma unroll
    for (int ks = 0; ks < BK / 4; ++ks) {
      T ar[2], ai[2], br[2], bi_[2];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        ar[mi] = Asr[wrow + mi * 16 + li][ks * 4 + lk];
        ai[mi] = Asi[wrow + mi * 16 + li][ks * 4 + lk];
      }
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        br[ni] = Bsr[ks * 4 + lk][wcol + ni * 16 + li];
        bi_[ni] = Bsi[ks * 4 + lk][wcol + ni * 16 + li];
      }
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
          accr[mi][ni] = Mfma<T>::mma(ar[mi], br[ni], accr[mi][ni]);
          accr[mi][ni] = Mfma<T>::mma(-ai[mi], bi_[ni], accr[mi][ni]);
          acci[mi][ni] = Mfma<T>::mma(ar[mi], bi_[ni], acci[mi][ni]);
          acci[mi][ni] = Mfma<T>::mma(ai[mi], br[ni], acci[mi][ni]);
        }
    }
    __syncthreads();
  }

  T* Cb = C + 2 * d.c_off;
  const bool beta0 = (beta_re == T(0)) && (beta_im == T(0));
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const acc_t vr = accr[mi][ni];
      const acc_t vi = acci[mi][ni];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = i0 + wrow + mi * 16 + Mfma<T>::acc_row(lk, r);
        const int col = j0 + wcol + ni * 16 + li;
        if (row < M && col < N) {
          const int64_t off = 2 * ((int64_t)row * ldc + col);
          T outr = alpha_re * (T)vr[r] - alpha_im * (T)vi[r];
          T outi = alpha_re * (T)vi[r] + alpha_im * (T)vr[r];
          if (!beta0) {
            const T cr = Cb[off], ci = Cb[off + 1];
            outr += beta_re * cr - beta_im * ci;
            outi += beta_re * ci + beta_im * cr;
          }
          Cb[off] = outr;
          Cb[off + 1] = outi;
        }
      }
    }
}

// The op-pair tables below are indexed [opA][opB] with the OP_* codes.
template <typename T, int BN, bool GUARD>
auto real_kernel(int oa, int ob) {
#define K(OA, OB) gemm_tiles_k<T, OA, OB, BN, GUARD>
  static constexpr decltype(&K(OP_N, OP_N)) table[2][2] = {
      {K(OP_N, OP_N), K(OP_N, OP_T)}, {K(OP_T, OP_N), K(OP_T, OP_T)}};
#undef K
  return table[oa][ob];
}

template <typename T>
auto cplx_kernel(int oa, int ob) {
#define K(OA, OB) gemm_tiles_cplx_k<T, OA, OB>
  static constexpr decltype(&K(OP_N, OP_N)) table[3][3] = {
      {K(OP_N, OP_N), K(OP_N, OP_T), K(OP_N, OP_C)},
      {K(OP_T, OP_N), K(OP_T, OP_T), K(OP_T, OP_C)},
      {K(OP_C, OP_N), K(OP_C, OP_T), K(OP_C, OP_C)}};
#undef K
  return table[oa][ob];
}

}  // namespace

template <typename T>
void dlaf::gemm_tiles(const GemmDesc* descs, int ndesc, const T* A, const T* B,
                      T* C, int M, int N, int K, int lda, int ldb, int ldc,
                      int opA, int opB, T alpha, T beta, hipStream_t stream,
                      int inplace) {
  if (ndesc <= 0 || M <= 0 || N <= 0 || !valid_op(opA) || !valid_op(opB)) return;
  // glds fast path for full-tile non-inplace batches (the hot phases)
  if (!inplace && gemm_tiles_v2(descs, ndesc, A, B, C, M, N, K, lda, ldb, ldc,
                                opA, opB, alpha, beta, stream))
    return;
  // OP_C == OP_T for real scalars
  const int oa = (opA == OP_C) ? OP_T : opA;
  const int ob = (opB == OP_C) ? OP_T : opB;
  // In-place applies take the 128-wide block (N <= 128 is then one column
  // block, see the kernel comment); its guard-free form needs full blocks.
  // Everything else is BN=64, guarded: with v2 in front, a full-tile
  // non-inplace batch arrives here only for K == 0, where the guarded kernel
  // computes the same C = beta*C without touching A or B.
  const int BN = inplace ? 128 : 64;
  const bool full = inplace && M % 128 == 0 && N % 128 == 0 && K % 16 == 0;
  const int mblocks = (M + 127) / 128, nblocks = (N + BN - 1) / BN;
  const auto kern = !inplace ? real_kernel<T, 64, true>(oa, ob)
                    : full   ? real_kernel<T, 128, false>(oa, ob)
                             : real_kernel<T, 128, true>(oa, ob);
  hipLaunchKernelGGL(kern, dim3(ndesc * mblocks * nblocks), dim3(256), 0,
                     stream, descs, A, B, C, M, N, K, lda, ldb, ldc, alpha,
                     beta, mblocks, nblocks);
}

template <typename T>
void dlaf::gemm_tiles(const GemmDesc* descs, int ndesc, const cplx<T>* A,
                      const cplx<T>* B, cplx<T>* C, int M, int N, int K,
                      int lda, int ldb, int ldc, int opA, int opB,
                      cplx<T> alpha, cplx<T> beta, hipStream_t stream,
                      int /*inplace*/) {
  if (ndesc <= 0 || M <= 0 || N <= 0 || !valid_op(opA) || !valid_op(opB)) return;
  if (gemm_tiles_v2(descs, ndesc, A, B, C, M, N, K, lda, ldb, ldc, opA, opB,
                    alpha, beta, stream))
    return;
  const int mblocks = (M + 63) / 64, nblocks = (N + 63) / 64;
  hipLaunchKernelGGL(cplx_kernel<T>(opA, opB),
                     dim3(ndesc * mblocks * nblocks), dim3(256), 0, stream,
                     descs, interleaved(A), interleaved(B), interleaved(C), M,
                     N, K, lda, ldb, ldc, alpha.re, alpha.im, beta.re, beta.im,
                     mblocks, nblocks);
}

#define INSTANTIATE(S)                                                        \
  template void dlaf::gemm_tiles(const GemmDesc*, int, const S*, const S*, S*, \
                                 int, int, int, int, int, int, int, int, S, S, \
                                 hipStream_t, int);
INSTANTIATE(double)
INSTANTIATE(float)
INSTANTIATE(cplx<double>)
INSTANTIATE(cplx<float>)
#undef INSTANTIATE
