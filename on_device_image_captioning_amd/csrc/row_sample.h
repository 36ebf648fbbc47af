// Drawing words from one row of vocabulary scores by one block of 1024 threads: the noise, the per-thread candidate
// lists and the k draw rounds that logsoftmax_sample_kernel (decoder_ops.hip) and sample_filter_kernel
// (sample_filter.hip) share, so that the filtered draw with its filter off IS the plain draw.
#pragma once
#include "row_select.h"

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                              unsigned k1, unsigned (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// Gumbel noise from the upper 24 bits.  16777215 + 0.5 rounds to 2^24 in fp32: without the clamp that one pattern gives
// u = 1, noise +inf, and its word is drawn whatever its probability.
__device__ __forceinline__ float gumbel_from_bits(unsigned b) {
  const float u = fminf(((float)(b >> 8) + 0.5f) * (1.0f / 16777216.0f), 0x1.fffffep-1f);       // (0,1), 24 bits
  return -logf(-logf(u));
}

// A thread's KM best perturbed scores so far, best first; an equal score stays behind the one met earlier.
template <int KM> struct DrawList {
  float v[KM]; int i[KM];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int q = 0; q < KM; ++q) { v[q] = -INFINITY; i[q] = 0x7fffffff; }
  }
  __device__ __forceinline__ void offer(float s, int si) {
    if (s > v[KM - 1]) {
#pragma unroll
      for (int q = 0; q < KM; ++q) {
        if (s > v[q]) { const float fv = v[q]; const int fi = i[q]; v[q] = s; i[q] = si; s = fv; si = fi; }
      }
    }
  }
  __device__ __forceinline__ void pop() {
#pragma unroll
    for (int q = 0; q + 1 < KM; ++q) { v[q] = v[q + 1]; i[q] = i[q + 1]; }
    v[KM - 1] = -INFINITY; i[KM - 1] = 0x7fffffff;
  }
};

// The k draws of row x (V words, log-sum-exp lse) from the threads' lists: round r takes the block's best head, thread 0
// stores its word and the word's log-probability x[v] - lse; its perturbed score (x[v] + noise) - lse goes to top_pert
// where the caller wants it (nullptr: not stored) — stochastic beam search ranks whole captions by it.
template <int KM>
__device__ __forceinline__ void block_draw_rounds(DrawList<KM>& l, const float* __restrict__ x, int V, int k, float lse,
                                                  float* __restrict__ top_val, int* __restrict__ top_idx,
                                                  float* __restrict__ top_pert, ArgmaxSlots<16>& win) {
  const int tid = threadIdx.x;
  for (int r = 0; r < k; ++r) {
    float best = l.v[0]; int besti = l.i[0];
    block_argmax<16>(best, besti, win, r);
    if (besti == 0x7fffffff) {                           // (block-uniform) every list is empty: a short row
      // Fewer than k words have a non-zero probability.  No list ever overflowed (one that did holds KM >= k words), so
      // the words drawn so far are ALL the words above -inf; slots r .. k-1 take the others by ascending index with
      // log-prob -inf.  V >= k, so there are enough of them: no index outside [0, V) is formed and x[] is not read there.
      int pi = -1;
      for (int rr = r; rr < k; ++rr) {
        float fv = -INFINITY; int fi = 0x7fffffff;
        for (int i = tid; i < V; i += 1024)
          if (i > pi && !(x[i] > -INFINITY)) { fi = i; break; }
        block_argmax<16>(fv, fi, win, rr + 1);            // equal values: the lowest index wins
        if (tid == 0) { top_val[rr] = -INFINITY; top_idx[rr] = fi; if (top_pert) top_pert[rr] = -INFINITY; }
        pi = fi;
      }
      break;
    }
    if (tid == 0) { top_val[r] = x[besti] - lse; top_idx[r] = besti; if (top_pert) top_pert[r] = best - lse; }
    if (l.i[0] == besti) l.pop();
  }
}
