// Work decomposition of the fused tile Cholesky (csrc/factor.hip), in plain
// C++ so the same arithmetic runs in the kernels, on the host launcher and in
// the stand-alone check tools/check_potrf_plan.cpp.
//
// A tile of nbk x nbk blocks of kPotrfBsz is factored by nbk launches; launch
// boundaries are the only synchronisation between workgroups.
//
//   launch 0      one workgroup: factor block (0,0), write dinv[0].
//   launch d >= 1 one workgroup per lower block (I,J), d <= J <= I < nbk, of
//                 the trailing part. With c = d-1 it forms
//                 X_I = A[I,c] dinv[c]^H and X_J, applies A[I,J] -= X_I X_J^H,
//                 and workgroup (d,d) factors its block and writes dinv[d].
//
// Who writes what in launch d (nobody else touches these in that launch):
//   A[I,J]            workgroup (I,J): its own block (diagonal blocks: lower
//                     triangle only); read by nobody else.
//   dinv[d]           workgroup (d,d); dinv[c] is only read.
//   X_I (= L[I,c])    workgroup (I,d). Every workgroup of row I or column I
//                     still reads A[I,c] in this launch, so X_I goes to the
//                     side buffer half (c & 1), not into the tile -- except in
//                     the last launch (d == nbk-1), whose single workgroup
//                     writes it in place.
//   A[R,d-2] (d >= 2) copied from side half ((d-2) & 1), which launch d-1
//                     wrote and launch d does not write: workgroup (I,d)
//                     copies R = I, and workgroup (nbk-1,d) also R = d-1.
//                     Column d-2 of the tile is read by nobody from launch d-1
//                     on.
#pragma once

#if defined(__HIPCC__)
#define POTRF_PLAN_HD __host__ __device__
#else
#define POTRF_PLAN_HD
#endif

namespace dlaf {
namespace potrf_plan {

POTRF_PLAN_HD inline int nblocks(int n, int bsz) { return (n + bsz - 1) / bsz; }

// workgroups of launch d
POTRF_PLAN_HD inline int grid(int nbk, int d) {
  if (d == 0) return 1;
  const int t = nbk - d;
  return t * (t + 1) / 2;
}

// linear workgroup id -> block (I,J), column by column; id 0 is (d,d), the
// workgroup on the critical path
POTRF_PLAN_HD inline void block_of(int wg, int nbk, int d, int* I, int* J) {
  int j = d, len = nbk - d;
  while (wg >= len) {
    wg -= len;
    --len;
    ++j;
  }
  *J = j;
  *I = j + wg;
}

POTRF_PLAN_HD inline bool factors(int I, int J, int d) { return I == d && J == d; }

// X_I of launch d goes to the side buffer (half (d-1) & 1) ...
POTRF_PLAN_HD inline bool writes_side(int I, int J, int nbk, int d) {
  (void)I;
  return d >= 1 && J == d && d < nbk - 1;
}
// ... or straight into A[I,d-1]
POTRF_PLAN_HD inline bool writes_panel_in_place(int I, int J, int nbk, int d) {
  (void)I;
  return d >= 1 && J == d && d == nbk - 1;
}
// does workgroup (I,J) of launch d copy block row R of column d-2 into the tile
POTRF_PLAN_HD inline bool copies_row(int I, int J, int nbk, int d, int R) {
  if (d < 2 || J != d) return false;
  return R == I || (I == nbk - 1 && R == d - 1);
}

// elements of the side buffer: two halves of (nbk * bsz) x bsz
POTRF_PLAN_HD inline long side_elems(int nbk, int bsz) {
  return 2L * nbk * bsz * bsz;
}
POTRF_PLAN_HD inline long side_offset(int half, int R, int nbk, int bsz) {
  return ((long)half * nbk + R) * bsz * bsz;
}

}  // namespace potrf_plan
}  // namespace dlaf
