// Pieces shared by the one-vector kernels over the tile storage (trsv.hip,
// hemv.hip): V-element loads with a guarded scalar twin, the double
// accumulator type of each element type, and the wave reduction.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "cplx.h"

namespace dlaf::vecacc {

template <typename S, int V>
struct alignas(V > 1 ? sizeof(S) * V : alignof(S)) Vec {
  S v[V];
};

// The V elements at p (element c of a row of `limit` valid ones): one 16-byte
// load when the row is aligned (then all V are valid), else V guarded scalar
// loads. Both give a lane the same elements, so both paths sum in the same
// order and return the same bits.
template <typename S, int V, bool ALIGNED>
__device__ inline void load_vec(Vec<S, V>& x, const S* p, int c, int limit) {
  if constexpr (ALIGNED) {
    x = *reinterpret_cast<const Vec<S, V>*>(p);
  } else {
#pragma unroll
    for (int k = 0; k < V; ++k)
      if (c + k < limit) x.v[k] = p[k];
  }
}

template <typename S>
struct IsCplx : std::false_type {};
template <typename T>
struct IsCplx<cplx<T>> : std::true_type {};

// accumulator type: single precision sums in double
template <typename S>
struct Acc {
  using type = S;
};
template <>
struct Acc<float> {
  using type = double;
};
template <>
struct Acc<cplx<float>> {
  using type = cplx<double>;
};

template <typename S>
__device__ inline typename Acc<S>::type widen(S x) {
  using A = typename Acc<S>::type;
  if constexpr (IsCplx<S>::value)
    return A(x.re, x.im);
  else
    return (A)x;
}
template <typename S>
__device__ inline S narrow(typename Acc<S>::type x) {
  if constexpr (IsCplx<S>::value) {
    using R = typename ScalarTraits<S>::real_t;
    return S((R)x.re, (R)x.im);
  } else {
    return (S)x;
  }
}

__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ inline cplx<double> wave_sum(cplx<double> v) {
  return {wave_sum(v.re), wave_sum(v.im)};
}

}  // namespace dlaf::vecacc
