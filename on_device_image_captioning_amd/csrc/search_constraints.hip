// Constrained word selection for the search step: odic_topk_rows_constrained, the sibling of odic_topk_rows.
//
// The rows hold log-probabilities already (logp_out of odic_logsoftmax_topk, or the output of odic_ensemble_logprobs) and
// are taken as they are: this file has no normaliser, so a constrained caption's per-token log-probs are bit for bit the
// numbers the unconstrained kernel computes.  One 512-thread block per row:
//   1. the row's inadmissible words as a bitmap of ceil(V/32) words in LDS: zeroed, then threads run over the banned
//      list, the EOS rule and the start positions j of the no-repeat rule, each setting bits with atomicOr;
//   2. a thread keeps its 20-value slice of the row and the admissibility bit of each value in registers (V <= 10240;
//      longer rows stream from memory and look the bitmap up again in every round);
//   3. block_ranked_topk (row_select.h), the routine the overflow path of row_logsoftmax_topk calls too: k rounds of a
//      block-wide arg-max over the elements ranked after the last winner, here with a scan that skips the inadmissible
//      ones.  There is no candidate list, so any number of ties is exact for every k <= 16.
// A finished row (row_valid == 0) builds no bitmap and gets what odic_topk_rows gives it.
#include "row_select.h"

namespace {

constexpr int SC_NTH = 512;
constexpr int SC_NPT = 10240 / SC_NTH;              // values a thread keeps in registers
constexpr int SC_MAX_V = 32768 * 8;                 // the bitmap may take 32 KB of LDS
constexpr int SC_MAX_K = 16;                        // odic_beam_step's limits
constexpr int SC_MAX_T = 128;
constexpr int SC_MAX_BANNED = 1024;

struct ConstraintParams {
  const long long* tokens; const int* pos; const int* row_valid; const int* banned;
  int n_banned, ngram, min_words, T;
  long long eos;
};

__device__ __forceinline__ void ban(unsigned* bm, long long w, int V) {
  if (w >= 0 && w < V) atomicOr(&bm[w >> 5], 1u << (w & 31));
}

__global__ __launch_bounds__(SC_NTH) void topk_rows_constrained_kernel(const float* __restrict__ logp, long ldl,
                                                                       ConstraintParams c, float* __restrict__ top_val,
                                                                       int* __restrict__ top_idx, int V, int k) {
  extern __shared__ unsigned bm[];                  // bit w set: word w is inadmissible
  __shared__ ArgmaxSlots<SC_NTH / 64> win;
  const int tid = threadIdx.x;
  const int n = blockIdx.x;
  const float* x = logp + (long)n * ldl;
  const int nw = (V + 31) >> 5;
  for (int i = tid; i < nw; i += SC_NTH) bm[i] = 0u;
  __syncthreads();
  if (!c.row_valid || c.row_valid[n] != 0) {        // (block-uniform) a growing row
    const int pos = min(max(*c.pos, 0), c.T - 1);   // the prefix is tokens[n][0 .. pos], never read outside the row
    const long long* p = c.tokens + (long)n * c.T;
    for (int i = tid; i < c.n_banned; i += SC_NTH) ban(bm, c.banned[i], V);
    if (tid == 0 && pos < c.min_words) ban(bm, c.eos, V);
    const int ng = c.ngram;
    if (ng > 0) {
      // start j repeats the last ng-1 words: p[j .. j+ng-2] == p[pos-ng+2 .. pos]; the word behind it may not follow again
      for (int j = tid; j <= pos - ng + 1; j += SC_NTH) {
        bool same = true;
        for (int u = 0; u < ng - 1; ++u) same = same && p[j + u] == p[pos - ng + 2 + u];
        if (same) ban(bm, p[j + ng - 1], V);
      }
    }
  }
  __syncthreads();
  const bool small = V <= SC_NPT * SC_NTH;
  float xv[SC_NPT];
  unsigned adm = 0u;                                // bit u: element tid + u·SC_NTH exists and is admissible
  if (small) {
#pragma unroll
    for (int u = 0; u < SC_NPT; ++u) {
      const int i = tid + u * SC_NTH;
      const bool in = i < V;
      xv[u] = in ? x[i] : -INFINITY;
      if (in && !((bm[i >> 5] >> (i & 31)) & 1u)) adm |= 1u << u;
    }
  }
  // one call of scan: the thread's best admissible element ranked after the last winner (pv, pi)
  block_ranked_topk<SC_NTH>([&](float pv, int pi, float& best, int& besti) {
    if (small) {
#pragma unroll
      for (int u = 0; u < SC_NPT; ++u) {
        const float v = xv[u];
        const int i = tid + u * SC_NTH;
        const bool after = ranks_after(v, i, pv, pi), before = ranks_before(v, i, best, besti);
        if (((adm >> u) & 1u) & after & before) { best = v; besti = i; }
      }
    } else {
      for (int i = tid; i < V; i += SC_NTH) {
        const float v = x[i];
        if (ranks_after(v, i, pv, pi) && !((bm[i >> 5] >> (i & 31)) & 1u) && ranks_before(v, i, best, besti)) { best = v; besti = i; }
      }
    }
  }, k, 0.f, top_val + (long)n * k, top_idx + (long)n * k, win);
}

}  // namespace

extern "C" int odic_topk_rows_constrained(const float* logp, int64_t ldl, const odic_search_constraints* c,
                                          float* top_val, int32_t* top_idx, int32_t N, int32_t V, int32_t k,
                                          void* stream) {
  // one refusal code, a missing pointer included (include/odic_hip.h)
  if (!logp || !c || !top_val || !top_idx || !c->tokens || !c->pos) return ODIC_EINVAL;
  if (N <= 0 || V <= 0 || V > SC_MAX_V || ldl < V || k < 1 || k > SC_MAX_K) return ODIC_EINVAL;
  if (c->T < 2 || c->T > SC_MAX_T) return ODIC_EINVAL;
  if (c->n_banned < 0 || c->n_banned > SC_MAX_BANNED || (c->n_banned > 0 && !c->banned)) return ODIC_EINVAL;
  if (c->no_repeat_ngram < 0 || c->no_repeat_ngram > c->T || c->min_words < 0) return ODIC_EINVAL;
  // a row loses at most n_banned + 1 (EOS) + T - 1 (one word per start position) words: k admissible ones remain
  if ((int64_t)c->n_banned + c->T + k > V) return ODIC_EINVAL;
  ConstraintParams p;
  p.tokens = (const long long*)c->tokens; p.pos = c->pos; p.row_valid = c->row_valid; p.banned = c->banned;
  p.n_banned = c->n_banned; p.ngram = c->no_repeat_ngram; p.min_words = c->min_words; p.T = c->T;
  p.eos = (long long)c->eos_idx;
  const size_t lds = (size_t)((V + 31) / 32) * sizeof(unsigned);
  hipLaunchKernelGGL(topk_rows_constrained_kernel, dim3(N), dim3(SC_NTH), lds, (hipStream_t)stream, logp, (long)ldl, p,
                     top_val, top_idx, V, k);
  return odic_launch_status();
}
