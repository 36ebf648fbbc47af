// Stochastic beam search (Kool, van Hoof & Welling, "Stochastic Beams and Where to Find Them", ICML 2019): the step that
// keeps, per image, the k captions with the largest PERTURBED log-probability — k captions sampled from the model without
// replacement — as the sibling of beam_step_kernel on the same state (beam_step.h).
//
// Every row j carries, besides its log-probability phi_j (cumul), its perturbed score G_j (gscore): phi_j plus Gumbel noise,
// conditioned top-down so that the largest perturbed score among the continuations of a prefix IS the prefix's own.  A step
// gets, from odic_logsoftmax_sample_scored with k = beams, the k continuations of every row with the largest
//   g_r = phi_j + cand_pert[r]      (cand_pert[r] = log-prob of the word + its Gumbel noise, rank 0 the largest: Z = g_0)
// and turns them into scores conditioned on max_r g_r = G_j:
//   G~_r = -log(e^-G_j - e^-Z + e^-g_r)
// evaluated in the stable form below, in which neither exponential is ever formed and phi_j cancels out of d_r.  The k
// largest G~ over all rows of the image are the new rows, in that order: row 0 is always the first sample.
//
// Wave 0 computes the (at most 256) G~ — one lane per candidate, four at k = 16 — leaves them in LDS, and runs k rounds of
// wave_extract_best on them with the flat index row·k + rank as the key (ties: source row, then rank, ascending).
// Everything after the choice is beam_apply.
#include "beam_step.h"

namespace {

// log(1 - e^d) for d < 0 (Mächler, "Accurately computing log(1 - exp(-|a|))"): the branch keeps the argument of the
// logarithm away from the cancellation each form has on the other side of -ln 2
__device__ __forceinline__ float log1mexp(float d) {
  return d > -0.693147180559945f ? logf(-expm1f(d)) : log1pf(-expf(d));
}

// G~ of a candidate of a growing row: G the row's perturbed score, phi its log-prob, pert / pert0 the candidate's and the
// row's largest perturbed word score.  Never above G; exactly G for rank 0 and for an exact tie with it.
// (This file is built with -fno-slp-vectorize, see the Makefile: hipcc's SLP pass pairs the double-float additions inside
//  expm1f / log1pf into packed fp32 ops with `op_sel` source selection — tests/test_isa_lint.py)
__device__ __forceinline__ float child_gscore(float G, float phi, float pert, float pert0) {
  const float d = pert - pert0;                        // g_r - Z <= 0
  if (d == 0.f) return G;
  const float u = (G - phi) - pert;                    // G_j - g_r
  const float v = u + log1mexp(d);
  return G - fmaxf(v, 0.f) - log1pf(expf(-fabsf(v)));  // G - softplus(v)
}

struct StochasticShared {
  float cp[MAX_K * MAX_K];              // cand_pert [beam][rank]
  float gt[MAX_K * MAX_K];              // G~ of every candidate; -inf: not offered
  float g[MAX_K];                       // gscore of the rows before the step
};

// Offers: a live (cumul > -inf; t = 0: row 0 alone, phi = G = 0) growing row every candidate with a finite log-prob; a
// live finished row itself — the word of its rank-0 slot at 0, as in beam_select — at its own G.  A slot for which no
// offer is left becomes an EMPTY row with the convention of require_beam_select, and gscore -inf.
__device__ __forceinline__ void stochastic_beam_select(const BeamParams& p, BeamShared& s, StochasticShared& x,
                                                       float* __restrict__ gscore, int b, int t) {
  if (threadIdx.x >= 64) return;
  const int lane = threadIdx.x, k = p.k;
  float tot[BEAM_CPL], val[BEAM_CPL]; int key[BEAM_CPL];
#pragma unroll
  for (int u = 0; u < BEAM_CPL; ++u) {
    const int i = lane + 64 * u;
    tot[u] = -INFINITY; val[u] = 0.f; key[u] = NO_KEY<int>;
    if (i < k * k) {
      const int j = i / k, c = i - j * k;
      const bool live = t == 0 ? j == 0 : s.cu[j] > -INFINITY;
      const bool fin = t > 0 && s.eos[j];
      const float G = t == 0 ? 0.f : x.g[j], phi = t == 0 ? 0.f : s.cu[j];
      float gv = -INFINITY, v = 0.f;
      if (live && fin) {
        if (c == 0) gv = G;
      } else if (live && s.cv[i] > -INFINITY) {
        v = s.cv[i];
        gv = child_gscore(G, phi, x.cp[i], x.cp[j * k]);
      }
      x.gt[i] = gv;
      if (gv > -INFINITY) { tot[u] = gv; val[u] = v; key[u] = i; }
    }
  }
  // lane 0 reads the G~ every lane of this wave has just stored
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  for (int r = 0; r < k; ++r) {
    int bi; float bval;
    const bool found = wave_extract_best(tot, key, val, bi, bval);
    if (lane == 0) {
      s.parent[r] = found ? bi / k : (t == 0 ? 0 : r);
      s.word[r] = found ? s.ci[bi] : (int)p.eos;
      s.lp[r] = found ? bval : -INFINITY;
      gscore[b * k + r] = found ? x.gt[bi] : -INFINITY;   // (every read of the old gscore is behind beam_load_rows' barrier)
    }
  }
}

__global__ __launch_bounds__(256) void stochastic_beam_step_kernel(BeamParams p, EmbedArgs e,
                                                                   const float* __restrict__ cand_pert,
                                                                   float* __restrict__ gscore) {
  __shared__ BeamShared s;
  __shared__ StochasticShared x;
  const int b = blockIdx.x, k = p.k;
  const int t = *p.pos;
  if (t + 1 >= p.T) return;
  for (int i = threadIdx.x; i < k * k; i += BEAM_NT) x.cp[i] = cand_pert[(long)b * k * k + i];
  if (threadIdx.x < k) x.g[threadIdx.x] = gscore[b * k + threadIdx.x];      // (not used at t = 0: need not be initialised)
  beam_load_rows(p, s, b, t);
  stochastic_beam_select(p, s, x, gscore, b, t);
  beam_apply(p, e, s, b, t);
}

}  // namespace

extern "C" int odic_stochastic_beam_step(const float* cand_val, const int32_t* cand_idx, const float* cand_pert,
                                         float* gscore, const odic_beam_state* st, const odic_embed_args* emb,
                                         int32_t n_img, int32_t beams, int32_t T, int64_t eos_idx, void* stream) {
  if (!cand_val || !cand_idx || !cand_pert || !gscore || eos_idx < 0) return ODIC_EINVAL;
  BeamParams p; EmbedArgs e;
  if (beam_params(p, e, st, emb, n_img, beams, T, eos_idx) != 0) return ODIC_EINVAL;     // one refusal code here
  p.cand_val = cand_val; p.cand_idx = cand_idx;
  hipLaunchKernelGGL(stochastic_beam_step_kernel, dim3(n_img), dim3(BEAM_NT), 0, (hipStream_t)stream, p, e, cand_pert,
                     gscore);
  return odic_launch_status();
}
