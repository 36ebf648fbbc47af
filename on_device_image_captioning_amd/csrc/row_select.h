// Selection and reduction over one row of vocabulary scores by one block: what decoder_ops.hip, search_constraints.hip
// and decoder_seq.hip share.  The ranking rule that makes every search reproduce the reference word for word — larger
// value first, ties to the lower index — is spelled in ranks_before and nowhere else in those files (the beam
// selection's wave_extract_best ranks by its own key).
#pragma once
#include "odic_common.h"

// (v, i) comes before (bv, bi).  The conditions are joined with | and &: with || and && hipcc branches once per
// element scanned (profiles/r21_one_selection_core.txt).  A NaN ranks neither before nor after anything.
__device__ __forceinline__ bool ranks_before(float v, int i, float bv, int bi) {
  return (v > bv) | ((v == bv) & (i < bi));
}
// (v, i) comes after the last winner (pv, pi): what a later round of a k-round selection may still take
__device__ __forceinline__ bool ranks_after(float v, int i, float pv, int pi) { return ranks_before(pv, pi, v, i); }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ void wave_argmax(float& best, int& besti) {        // every lane ends with the winner
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(besti, o, 64);
    if (ranks_before(ov, oi, best, besti)) { best = ov; besti = oi; }
  }
}

// Block reductions over `red` (one slot per wave), every thread ends with the result; the waves are combined in
// ascending order.  The leading barrier lets consecutive calls share one `red`.
template <typename T> __device__ __forceinline__ T block_sum(T v, T* red) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  T t = 0;
  for (int i = 0; i < nw; ++i) t += red[i];
  return t;
}
__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  float t = red[0];
  for (int i = 1; i < nw; ++i) t = fmaxf(t, red[i]);
  return t;
}

// Block arg-max of a block of NWV waves: every thread ends with the block's winner.  Synchronisation: call number
// `rd` of a kernel (0, 1, 2, ...) writes slot set rd & 1 and has ONE barrier, between the wave winners' stores and
// everybody's loads.  A wave that is still loading set rd & 1 cannot be overtaken by a store to it: that store belongs
// to call rd + 2, behind the barrier of call rd + 1, which the slow wave has yet to reach.
template <int NWV> struct ArgmaxSlots { float v[2][NWV]; int i[2][NWV]; };

template <int NWV>
__device__ __forceinline__ void block_argmax(float& best, int& besti, ArgmaxSlots<NWV>& s, int rd) {
  wave_argmax(best, besti);
  if ((threadIdx.x & 63) == 0) { s.v[rd & 1][threadIdx.x >> 6] = best; s.i[rd & 1][threadIdx.x >> 6] = besti; }
  __syncthreads();
  best = s.v[rd & 1][0]; besti = s.i[rd & 1][0];
#pragma unroll
  for (int w = 1; w < NWV; ++w) {
    const float ov = s.v[rd & 1][w]; const int oi = s.i[rd & 1][w];
    if (ranks_before(ov, oi, best, besti)) { best = ov; besti = oi; }
  }
}

// The k best of a row in rank order, exact for any number of ties: k rounds of a block-wide arg-max over the elements
// ranked after the last winner.  scan(pv, pi, best, besti) is the calling thread's share of a round: it leaves in
// (best, besti) the first of its elements that ranks_after (pv, pi), or (-inf, INT_MAX) untouched when it has none.
// Thread 0 stores top_val[rd] = value - lse and top_idx[rd].
template <int NTH, typename Scan>
__device__ __forceinline__ void block_ranked_topk(Scan scan, int k, float lse, float* top_val, int* top_idx,
                                                  ArgmaxSlots<NTH / 64>& s) {
  float pv = INFINITY; int pi = -1;                 // last winner
  for (int rd = 0; rd < k; ++rd) {
    float best = -INFINITY; int besti = 0x7fffffff;
    scan(pv, pi, best, besti);
    block_argmax<NTH / 64>(best, besti, s, rd);
    if (threadIdx.x == 0) { top_val[rd] = best - lse; top_idx[rd] = besti; }
    pv = best; pi = besti;
  }
}
