// "The n-th ranked word of a row" without a sort, for one block per row: the order-preserving integer key of a float, the
// block-wide count / mass sum with one barrier per call, and the bit-by-bit bisection over keys (or indices) that
// sample_filter.hip and contrast_rows.hip share.
#pragma once
#include "row_select.h"

// float → unsigned, order-preserving (a < b ⇔ key(a) < key(b), -0 = +0); every non-NaN float has a key > 0
__device__ __forceinline__ unsigned rank_key(float z) {
  unsigned b = __float_as_uint(z);
  if ((b << 1) == 0) b = 0;
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float key_value(unsigned key) {
  return __uint_as_float(key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

// Block sums of a count and (MASS) a mass over a block of NWV waves, every thread ends with both.  One barrier per call:
// call number rd writes slot set rd & 1 (block_argmax's scheme, row_select.h); the waves are combined in ascending order.
template <int NWV> struct CountMassSlots { double m[2][NWV]; int c[2][NWV]; };

template <bool MASS, int NWV>
__device__ __forceinline__ void block_count_mass(int& c, double& m, CountMassSlots<NWV>& s, int& rd) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if constexpr (MASS) m = wave_sum(m);
  const int p = rd++ & 1;
  if ((threadIdx.x & 63) == 0) {
    s.c[p][threadIdx.x >> 6] = c;
    if constexpr (MASS) s.m[p][threadIdx.x >> 6] = m;
  }
  __syncthreads();
  int tc = 0; double tm = 0.0;
#pragma unroll
  for (int w = 0; w < NWV; ++w) { tc += s.c[p][w]; if constexpr (MASS) tm += s.m[p][w]; }
  c = tc; m = tm;
}

// the largest t of `bits` bits with pred(t), for a block-uniform pred that holds at 0 and, once false, stays false
template <typename Pred> __device__ __forceinline__ unsigned bisect_max(int bits, Pred pred) {
  unsigned t = 0;
  for (int b = bits - 1; b >= 0; --b) {
    const unsigned c = t | (1u << b);
    if (pred(c)) t = c;
  }
  return t;
}
