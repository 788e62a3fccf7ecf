// Fused batched tile GEMM for CDNA4 (gfx950) — the glds full-tile fast path
// behind dlaf::gemm_tiles (gemm_tiles.hip holds the entry points and the
// guarded kernels; gemm_common.h the shared Mfma<T> / xcd_remap).
//
// Written from the ISA analysis of the register-staged kernel
// (profiles/gemm_isa_analysis.md): that loop was a serial stage->compute
// structure with 8-byte global loads and ~650 addressing instructions per
// 32 MFMA (MfmaUtil 57.5%). This kernel fixes all three findings at once by
// staging through LDS-DMA (`global_load_lds_dwordx4`, 16 B per lane):
//   * no register staging, no ds_write pass, no per-element address VALU —
//     each 1024-B LDS row is ONE instruction with per-lane global addresses
//     held in incremented registers;
//   * ping-pong LDS buffers with ONE barrier per K-step: the DMA of step
//     s+1 is issued before the MFMA block of step s, so its latency lands
//     under the 4096-cycle f64 MFMA span;
//   * 128x128 C blocks (4 waves, 64x64 per wave, 4x4 fragments of
//     mfma_f64_16x16x4) double the flop:LDS-byte ratio of the 128x64 block.
// Workgroup ids go through xcd_remap so one desc's blocks share an L2.
//
// Scope: full tiles only (M%128==0, N%64==0, K%16==0 real; 64/64/16
// complex), not in-place. Edge shapes and in-place panel applies stay on
// the guarded kernels (gemm_tiles.hip). Role parity: the per-tile gemm of
// the reference (include/dlaf/blas/tile.h) — here one launch covers a whole
// fused phase.
#include "gemm_common.h"

namespace {

__device__ inline void glds16(const void* g, void* lds) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) void*)g,
      (__attribute__((address_space(3))) void*)lds, 16, 0, 0);
}

// ---------------- real kernel ----------------
// BM=128 x BN (template 64/128), BK=16, 256 threads; 4 waves as a 2x2 grid
// of (64 x BN/2) tiles; NFRAG = BN/32 fragments of mfma_{f64,f32}_16x16x4.
// LDS (one __shared__ object — §5 trap 4a): S[2][A: 128*BK | B: BK*BN].
//   A image: OPA==N -> row-major [i][k] (XOR chunk swizzle, below), else
//   k-major [k][i]; B image: OPB==N -> k-major [k][c], else row-major
//   [c][k] (swizzled). Images are glds-lane-linear: instr t covers LDS
//   elems t*64*EPL..+64*EPL-1.
//
// Swizzle: a row-major image read column-wise is up to 8-way bank
// conflicted (rows are 128 B = 2 banks apart). The 16-B chunk at (row, c)
// holds global chunk c ^ (row & (CPR-1)) — applied on the per-lane glds
// SOURCE address (LDS stays lane-linear, the glds contract) and undone in
// the fragment index; residual conflict is 2-way.
template <typename T, int OPA, int OPB, int BN>
__launch_bounds__(256, 2) __global__ void gemm_v2_k(
    const GemmDesc* __restrict__ descs, const T* __restrict__ A,
    const T* __restrict__ B, T* __restrict__ C, int M, int N, int K, int lda,
    int ldb, int ldc, T alpha, T beta, int mblocks, int nblocks) {
  constexpr int BM = 128, BK = 16;
  constexpr int DEPTH = 2;             // LDS ping-pong buffers
  constexpr int EPL = 16 / sizeof(T);  // elements per lane per glds
  constexpr int CPR = BK / EPL;        // 16-B chunks per rk-image row
  constexpr int AEL = BM * BK;         // A image elements
  constexpr int BEL = BK * BN;         // B image elements
  constexpr int NFRAG = BN / 32;  // col frags per wave
  constexpr int MFRAG = BM / 32;  // row frags per wave
  __shared__ T S[DEPTH][AEL + BEL];

  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  const int per_desc = mblocks * nblocks;
  const GemmDesc d = descs[wg / per_desc];
  const int rem = wg % per_desc;
  const int i0 = (rem / nblocks) * BM, j0 = (rem % nblocks) * BN;

  const int tid = threadIdx.x;
  const int lane = tid & 63, w = tid >> 6;
  const int wrow = (w >> 1) * (BM / 2), wcol = (w & 1) * (BN / 2);
  const int li = lane & 15, lk = lane >> 4;

  const int spt = K / BK;  // steps per K-tile
  const int total = (int)d.ktiles * spt;
  // glds instructions per wave per step, per operand
  constexpr int NAW = AEL / (64 * EPL) / 4;
  constexpr int NBW = BEL / (64 * EPL) / 4;

  using acc_t = typename Mfma<T>::acc_t;
  acc_t acc[MFRAG][NFRAG];
#pragma unroll
  for (int a = 0; a < MFRAG; ++a)
#pragma unroll
    for (int b = 0; b < NFRAG; ++b) acc[a][b] = {0, 0, 0, 0};

  // per-lane glds source offsets for instr j=0 of this wave (element units,
  // relative to the K-tile base) and the per-instr / per-step increments
  const T* Abase0 = A + d.a_off;
  const T* Bbase0 = B + d.b_off;
  int64_t a_l0, a_jinc, a_sinc;
  if constexpr (OPA == OP_N) {  // swizzled rk image [i][k]
    constexpr int RPI = 64 / CPR;  // rows per instr
    const int r_in = lane / CPR;   // row within instr; also the swizzle mask
    a_l0 = (int64_t)(i0 + (NAW * w) * RPI + r_in) * lda +
           EPL * ((lane % CPR) ^ (r_in & (CPR - 1)));
    a_jinc = (int64_t)RPI * lda;
    a_sinc = BK;
  } else {  // kr image [k][BM]
    constexpr int KPI = 64 * EPL / BM;
    a_l0 = (int64_t)(NAW * w * KPI + lane / (BM / EPL)) * lda + i0 +
           (lane % (BM / EPL)) * EPL;
    a_jinc = (int64_t)KPI * lda;
    a_sinc = (int64_t)BK * lda;
  }
  int64_t b_l0, b_jinc, b_sinc;
  if constexpr (OPB == OP_N) {  // kr image [k][BN]
    constexpr int KPI = 64 * EPL / BN;
    b_l0 = (int64_t)(NBW * w * KPI + lane / (BN / EPL)) * ldb + j0 +
           (lane % (BN / EPL)) * EPL;
    b_jinc = (int64_t)KPI * ldb;
    b_sinc = (int64_t)BK * ldb;
  } else {  // swizzled rk image [c][k]
    constexpr int RPI = 64 / CPR;
    const int r_in = lane / CPR;
    b_l0 = (int64_t)(j0 + (NBW * w) * RPI + r_in) * ldb +
           EPL * ((lane % CPR) ^ (r_in & (CPR - 1)));
    b_jinc = (int64_t)RPI * ldb;
    b_sinc = BK;
  }

  // running state of the issue pipeline
  const T* aP = Abase0 + a_l0;
  const T* bP = Bbase0 + b_l0;
  int ks_cnt = 0;
  int64_t kt = 0;
  T* const Sflat = &S[0][0];
  constexpr int BUFE = AEL + BEL;
  const int ldsa = w * NAW * 64 * EPL;  // this wave's A LDS offset (j=0)
  const int ldsb = AEL + w * NBW * 64 * EPL;

  auto issue = [&](int buf) {
#pragma unroll
    for (int j = 0; j < NAW; ++j)
      glds16(aP + j * a_jinc, Sflat + buf * BUFE + ldsa + j * 64 * EPL);
#pragma unroll
    for (int j = 0; j < NBW; ++j)
      glds16(bP + j * b_jinc, Sflat + buf * BUFE + ldsb + j * 64 * EPL);
    // advance to the next K step (next K tile when this one is done)
    if (++ks_cnt == spt) {
      ks_cnt = 0;
      ++kt;
      aP = Abase0 + kt * d.a_kstride + a_l0;
      bP = Bbase0 + kt * d.b_kstride + b_l0;
    } else {
      aP += a_sinc;
      bP += b_sinc;
    }
  };

  auto compute = [&](int buf) {
    const T* sa = Sflat + buf * BUFE;
    const T* sb = sa + AEL;
    // fragment index helpers (undo the rk swizzle)
    auto aidx = [&](int row, int k) {
      return (OPA == OP_N)
                 ? row * BK + EPL * ((k / EPL) ^ (row & (CPR - 1))) + k % EPL
                 : k * BM + row;
    };
    auto bidx = [&](int col, int k) {
      return (OPB == OP_N)
                 ? k * BN + col
                 : col * BK + EPL * ((k / EPL) ^ (col & (CPR - 1))) + k % EPL;
    };
    T af[2][MFRAG], bf[2][NFRAG];
#pragma unroll
    for (int mi = 0; mi < MFRAG; ++mi)
      af[0][mi] = sa[aidx(wrow + mi * 16 + li, lk)];
#pragma unroll
    for (int ni = 0; ni < NFRAG; ++ni)
      bf[0][ni] = sb[bidx(wcol + ni * 16 + li, lk)];
#pragma unroll
    for (int ks = 0; ks < BK / 4; ++ks) {
      const int cur = ks & 1;
      if (ks + 1 < BK / 4) {
        const int nxt = 1 - cur;
        const int k = (ks + 1) * 4 + lk;
#pragma unroll
        for (int mi = 0; mi < MFRAG; ++mi)
          af[nxt][mi] = sa[aidx(wrow + mi * 16 + li, k)];
#pragma unroll
        for (int ni = 0; ni < NFRAG; ++ni)
          bf[nxt][ni] = sb[bidx(wcol + ni * 16 + li, k)];
      }
#pragma unroll
      for (int mi = 0; mi < MFRAG; ++mi)
#pragma unroll
        for (int ni = 0; ni < NFRAG; ++ni)
          acc[mi][ni] = Mfma<T>::mma(af[cur][mi], bf[cur][ni], acc[mi][ni]);
    }
  };

  // pipeline: DEPTH buffers, DEPTH-1 steps in flight; the vmcnt(0) drain of
  // __syncthreads() IS the completion wait.
  int ibuf = 0, cbuf = 0;
  for (int p = 0; p < DEPTH - 1 && p < total; ++p) {
    issue(ibuf);
    if (++ibuf == DEPTH) ibuf = 0;
  }
  for (int s = 0; s < total; ++s) {
    __syncthreads();  // drains the in-flight glds (vmcnt 0) + LDS reuse
    if (s + DEPTH - 1 < total) {
      issue(ibuf);
      if (++ibuf == DEPTH) ibuf = 0;
    }
    compute(cbuf);
    if (++cbuf == DEPTH) cbuf = 0;
  }

  // epilogue: C = alpha*acc + beta*C. The beta path batches its C loads per
  // mi-chunk (loads, then uses) — interleaved load/use would eat a full
  // vmcnt(0) drain per element (hipcc is conservative about ordinary loads
  // in a function that issued glds).
  T* Cb = C + d.c_off;
  if (beta != T(0)) {
#pragma unroll
    for (int mi = 0; mi < MFRAG; ++mi) {
      T cv[4 * NFRAG];
#pragma unroll
      for (int ni = 0; ni < NFRAG; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = i0 + wrow + mi * 16 + Mfma<T>::acc_row(lk, r);
          const int col = j0 + wcol + ni * 16 + li;
          cv[ni * 4 + r] = Cb[(int64_t)row * ldc + col];
        }
#pragma unroll
      for (int ni = 0; ni < NFRAG; ++ni) {
        const acc_t v = acc[mi][ni];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = i0 + wrow + mi * 16 + Mfma<T>::acc_row(lk, r);
          const int col = j0 + wcol + ni * 16 + li;
          Cb[(int64_t)row * ldc + col] = alpha * (T)v[r] + beta * cv[ni * 4 + r];
        }
      }
    }
  } else {
#pragma unroll
    for (int mi = 0; mi < MFRAG; ++mi)
#pragma unroll
      for (int ni = 0; ni < NFRAG; ++ni) {
        const acc_t v = acc[mi][ni];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = i0 + wrow + mi * 16 + Mfma<T>::acc_row(lk, r);
          const int col = j0 + wcol + ni * 16 + li;
          Cb[(int64_t)row * ldc + col] = alpha * (T)v[r];
        }
      }
  }
}

// ---------------- complex kernel ----------------
// Interleaved (re,im); one lane's 16-B glds = one complex f64 element (f32:
// two). BM=BN=64, BK=16; wave w owns the 32x32 quadrant; 2x2 fragments,
// 4 MFMA per fragment pair. LDS images mirror the real kernel with complex
// elements; fragments are read as (re,im) pairs in one ds_read_b128 (f64).
template <typename T, int OPA, int OPB>
__launch_bounds__(256, 2) __global__ void gemm_v2_cplx_k(
    const GemmDesc* __restrict__ descs, const T* __restrict__ A,
    const T* __restrict__ B, T* __restrict__ C, int M, int N, int K, int lda,
    int ldb, int ldc, T alpha_re, T alpha_im, T beta_re, T beta_im,
    int mblocks, int nblocks) {
  constexpr int BK = 16;
  constexpr int DEPTH = 2;            // LDS ping-pong buffers
  constexpr int CPL = 8 / sizeof(T);  // complex elems per lane per glds
  // S[buf][A: 64*16 | B: 16*64] complex elems, interleaved re/im
  __shared__ T S[DEPTH][4096 * (8 / sizeof(T))];

  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  const int per_desc = mblocks * nblocks;
  const GemmDesc d = descs[wg / per_desc];
  const int rem = wg % per_desc;
  const int i0 = (rem / nblocks) * 64, j0 = (rem % nblocks) * 64;

  const int tid = threadIdx.x;
  const int lane = tid & 63, w = tid >> 6;
  const int wrow = (w >> 1) * 32, wcol = (w & 1) * 32;
  const int li = lane & 15, lk = lane >> 4;

  const int spt = K / BK;
  const int total = (int)d.ktiles * spt;
  constexpr int NAW = 1024 / (64 * CPL) / 4;  // glds per wave (c128: 4, c64: 2)

  using acc_t = typename Mfma<T>::acc_t;
  acc_t accr[2][2], acci[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      accr[a][b] = {0, 0, 0, 0};
      acci[a][b] = {0, 0, 0, 0};
    }

  const T* Abase0 = A + 2 * d.a_off;
  const T* Bbase0 = B + 2 * d.b_off;
  // offsets in COMPLEX elements (scaled by 2 at use)
  int64_t a_l0, a_jinc, a_sinc;
  if constexpr (OPA == OP_N) {  // [i][k] image, 16-elem rows
    constexpr int RPI = 64 * CPL / BK;  // rows per instr (c128: 4, c64: 8)
    a_l0 = (int64_t)(i0 + (NAW * w) * RPI + lane / (BK / CPL)) * lda +
           (lane % (BK / CPL)) * CPL;
    a_jinc = (int64_t)RPI * lda;
    a_sinc = BK;
  } else {  // [k][i] image, 64-elem k-rows
    constexpr int KPI = 64 * CPL / 64;  // k-rows per instr (c128: 1, c64: 2)
    a_l0 = (int64_t)(NAW * w * KPI + lane / (64 / CPL)) * lda + i0 +
           (lane % (64 / CPL)) * CPL;
    a_jinc = (int64_t)KPI * lda;
    a_sinc = (int64_t)BK * lda;
  }
  int64_t b_l0, b_jinc, b_sinc;
  if constexpr (OPB == OP_N) {
    constexpr int KPI = 64 * CPL / 64;
    b_l0 = (int64_t)(NAW * w * KPI + lane / (64 / CPL)) * ldb + j0 +
           (lane % (64 / CPL)) * CPL;
    b_jinc = (int64_t)KPI * ldb;
    b_sinc = (int64_t)BK * ldb;
  } else {
    constexpr int RPI = 64 * CPL / BK;
    b_l0 = (int64_t)(j0 + (NAW * w) * RPI + lane / (BK / CPL)) * ldb +
           (lane % (BK / CPL)) * CPL;
    b_jinc = (int64_t)RPI * ldb;
    b_sinc = BK;
  }

  const T* aP = Abase0 + 2 * a_l0;
  const T* bP = Bbase0 + 2 * b_l0;
  int ks_cnt = 0;
  int64_t kt = 0;
  T* const Sflat = &S[0][0];
  constexpr int BUFE = 4096 * (8 / sizeof(T));
  constexpr int BOFF = 2048 * (8 / sizeof(T));
  const int ldsw = w * NAW * 64 * CPL * 2;  // real-T units

  auto issue = [&](int buf) {
#pragma unroll
    for (int j = 0; j < NAW; ++j)
      glds16(aP + 2 * j * a_jinc, Sflat + buf * BUFE + ldsw + j * 64 * CPL * 2);
#pragma unroll
    for (int j = 0; j < NAW; ++j)
      glds16(bP + 2 * j * b_jinc,
             Sflat + buf * BUFE + BOFF + ldsw + j * 64 * CPL * 2);
    if (++ks_cnt == spt) {
      ks_cnt = 0;
      ++kt;
      aP = Abase0 + 2 * (kt * d.a_kstride + a_l0);
      bP = Bbase0 + 2 * (kt * d.b_kstride + b_l0);
    } else {
      aP += 2 * a_sinc;
      bP += 2 * b_sinc;
    }
  };

  auto compute = [&](int buf) {
    const T* sa = Sflat + buf * BUFE;
    const T* sb = sa + BOFF;
    auto aidx = [&](int row, int k) {
      return 2 * ((OPA == OP_N) ? row * BK + k : k * 64 + row);
    };
    auto bidx = [&](int col, int k) {
      return 2 * ((OPB == OP_N) ? k * 64 + col : col * BK + k);
    };
#pragma unroll
    for (int ks = 0; ks < BK / 4; ++ks) {
      const int k = ks * 4 + lk;
      T ar[2], ai[2], br[2], bi_[2];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        const int ix = aidx(wrow + mi * 16 + li, k);
        ar[mi] = sa[ix];
        ai[mi] = (OPA == OP_C) ? -sa[ix + 1] : sa[ix + 1];
      }
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        const int ix = bidx(wcol + ni * 16 + li, k);
        br[ni] = sb[ix];
        bi_[ni] = (OPB == OP_C) ? -sb[ix + 1] : sb[ix + 1];
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
  };

  int ibuf = 0, cbuf = 0;
  for (int p = 0; p < DEPTH - 1 && p < total; ++p) {
    issue(ibuf);
    if (++ibuf == DEPTH) ibuf = 0;
  }
  for (int s = 0; s < total; ++s) {
    __syncthreads();
    if (s + DEPTH - 1 < total) {
      issue(ibuf);
      if (++ibuf == DEPTH) ibuf = 0;
    }
    compute(cbuf);
    if (++cbuf == DEPTH) cbuf = 0;
  }

  T* Cb = C + 2 * d.c_off;
  if (beta_re != T(0) || beta_im != T(0)) {
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      T cv[16];
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = i0 + wrow + mi * 16 + Mfma<T>::acc_row(lk, r);
          const int col = j0 + wcol + ni * 16 + li;
          const int64_t off = 2 * ((int64_t)row * ldc + col);
          cv[(ni * 4 + r) * 2] = Cb[off];
          cv[(ni * 4 + r) * 2 + 1] = Cb[off + 1];
        }
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        const acc_t vr = accr[mi][ni];
        const acc_t vi = acci[mi][ni];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = i0 + wrow + mi * 16 + Mfma<T>::acc_row(lk, r);
          const int col = j0 + wcol + ni * 16 + li;
          const int64_t off = 2 * ((int64_t)row * ldc + col);
          const T cr = cv[(ni * 4 + r) * 2], ci = cv[(ni * 4 + r) * 2 + 1];
          Cb[off] = alpha_re * (T)vr[r] - alpha_im * (T)vi[r] +
                    beta_re * cr - beta_im * ci;
          Cb[off + 1] = alpha_re * (T)vi[r] + alpha_im * (T)vr[r] +
                        beta_re * ci + beta_im * cr;
        }
      }
    }
  } else {
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
          const int64_t off = 2 * ((int64_t)row * ldc + col);
          Cb[off] = alpha_re * (T)vr[r] - alpha_im * (T)vi[r];
          Cb[off + 1] = alpha_re * (T)vi[r] + alpha_im * (T)vr[r];
        }
      }
  }
}

// The op-pair tables below are indexed [opA][opB] with the OP_* codes.
template <typename T, int BN>
auto real_kernel(int oa, int ob) {
#define K(OA, OB) gemm_v2_k<T, OA, OB, BN>
  static constexpr decltype(&K(OP_N, OP_N)) table[2][2] = {
      {K(OP_N, OP_N), K(OP_N, OP_T)}, {K(OP_T, OP_N), K(OP_T, OP_T)}};
#undef K
  return table[oa][ob];
}

template <typename T>
auto cplx_kernel(int oa, int ob) {
#define K(OA, OB) gemm_v2_cplx_k<T, OA, OB>
  static constexpr decltype(&K(OP_N, OP_N)) table[3][3] = {
      {K(OP_N, OP_N), K(OP_N, OP_T), K(OP_N, OP_C)},
      {K(OP_T, OP_N), K(OP_T, OP_T), K(OP_T, OP_C)},
      {K(OP_C, OP_N), K(OP_C, OP_T), K(OP_C, OP_C)}};
#undef K
  return table[oa][ob];
}

}  // namespace

template <typename T>
bool dlaf::gemm_tiles_v2(const GemmDesc* descs, int ndesc, const T* A,
                         const T* B, T* C, int M, int N, int K, int lda,
                         int ldb, int ldc, int opA, int opB, T alpha, T beta,
                         hipStream_t stream) {
  if (M % 128 || N % 64 || K % 16 || K <= 0) return false;
  if (!valid_op(opA) || !valid_op(opB)) return false;
  // OP_C == OP_T for real scalars
  const int oa = (opA == OP_C) ? OP_T : opA;
  const int ob = (opB == OP_C) ? OP_T : opB;
  const int BN = (N % 128 == 0) ? 128 : 64;
  const int mblocks = M / 128, nblocks = N / BN;
  const auto kern =
      BN == 128 ? real_kernel<T, 128>(oa, ob) : real_kernel<T, 64>(oa, ob);
  hipLaunchKernelGGL(kern, dim3(ndesc * mblocks * nblocks), dim3(256), 0, stream,
                     descs, A, B, C, M, N, K, lda, ldb, ldc, alpha, beta,
                     mblocks, nblocks);
  return true;
}

template <typename T>
bool dlaf::gemm_tiles_v2(const GemmDesc* descs, int ndesc, const cplx<T>* A,
                         const cplx<T>* B, cplx<T>* C, int M, int N, int K,
                         int lda, int ldb, int ldc, int opA, int opB,
                         cplx<T> alpha, cplx<T> beta, hipStream_t stream) {
  if (M % 64 || N % 64 || K % 16 || K <= 0) return false;
  if (!valid_op(opA) || !valid_op(opB)) return false;
  const int mblocks = M / 64, nblocks = N / 64;
  hipLaunchKernelGGL(cplx_kernel<T>(opA, opB),
                     dim3(ndesc * mblocks * nblocks), dim3(256), 0, stream,
                     descs, interleaved(A), interleaved(B), interleaved(C), M,
                     N, K, lda, ldb, ldc, alpha.re, alpha.im, beta.re, beta.im,
                     mblocks, nblocks);
  return true;
}

#define INSTANTIATE(S)                                                     \
  template bool dlaf::gemm_tiles_v2(const GemmDesc*, int, const S*,        \
                                    const S*, S*, int, int, int, int, int, \
                                    int, int, int, S, S, hipStream_t);
INSTANTIATE(double)
INSTANTIATE(float)
INSTANTIATE(cplx<double>)
INSTANTIATE(cplx<float>)
#undef INSTANTIATE
