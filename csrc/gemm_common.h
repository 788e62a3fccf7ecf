// Device pieces shared by the two fused-GEMM translation units
// (gemm_tiles.hip, gemm_tiles_v2.hip).
#pragma once
#include "kernels.h"

typedef double v4d __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));

// 16x16x4 MFMA in the operand precision (exact fp64/fp32, the CDNA4
// "SGEMM-class" MFMA at the vector-f64/f32 rate) and the D-fragment layout:
// the row of accumulator register `r` held by lane group lk = lane>>4.
template <typename T>
struct Mfma;
template <>
struct Mfma<double> {
  using acc_t = v4d;
  static __device__ inline acc_t mma(double a, double b, acc_t c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  // D row of (lane, reg): measured on gfx950 (tools/probe_mfma_f64.hip):
  // row = (lane>>4) + 4*reg  (stride-4 between regs, UNLIKE the f32 form)
  static __device__ inline int acc_row(int lk, int r) { return lk + 4 * r; }
};
template <>
struct Mfma<float> {
  using acc_t = v4f;
  static __device__ inline acc_t mma(float a, float b, acc_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  // f32 16x16x4: row = 4*(lane>>4) + reg (cdna_hip_programming.md §3)
  static __device__ inline int acc_row(int lk, int r) { return lk * 4 + r; }
};

// Bijective XCD remap (8 XCDs, one L2 each): consecutive output ids land on
// one XCD so the blocks of one desc (which share A/B slabs) co-reside in one
// L2.
__device__ inline int xcd_remap(int wg, int nwg) {
  const int nx = 8;
  const int q = nwg / nx, r = nwg % nx;
  const int xcd = wg % nx, pos = wg / nx;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + pos;
}

// The launchers index their kernel tables with the op codes.
inline bool valid_op(int op) { return op == OP_N || op == OP_T || op == OP_C; }
