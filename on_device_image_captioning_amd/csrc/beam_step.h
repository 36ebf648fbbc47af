// The state of a beam-search step and the parts of it that every step kernel shares (decoder_ops.hip: beam, group and
// required-words steps; stochastic_beam.hip): the rows staged in LDS, the extraction a selection repeats, and the update
// half that follows whatever rule chose the rows.  A step kernel = beam_load_rows, its own selection by wave 0 (s.parent /
// s.word / s.lp), beam_apply.  The layout of the state and the order of a step are described in decoder_ops.hip.
#pragma once
#include "odic_common.h"

namespace {

constexpr int MAX_T = 128;     // max decode positions supported by the LDS scratch below
constexpr int MAX_K = 16;      // max beam size

struct BeamParams {
  const float* cand_val; const int* cand_idx;
  long long* tok; float* lp; int* anc;
  float* cumul; int* n_elem; int* has_eos; int* row_valid; long long* next_tok;
  int* pos; int* done; int* ctr;
  int n_img, k, T; long long eos;
};
struct BeamShared {
  float cv[MAX_K * MAX_K]; int ci[MAX_K * MAX_K];      // candidates: log-prob, word  [beam][rank]
  int eos[MAX_K]; int ne[MAX_K]; float cu[MAX_K];
  float lpm[MAX_K][MAX_T];                             // per-token log-probs of the k prefixes
  int parent[MAX_K]; int word[MAX_K]; float lp[MAX_K]; float cumul[MAX_K];
};

constexpr int BEAM_NT = 256;                           // threads of beam_step_kernel / group_beam_step_kernel

// The three parts of a step, shared by the three step kernels: beam_load_rows (the image's k x k candidates, per-beam
// flags and per-token log-probs into LDS; ends with a barrier that also covers the caller's own prologue), a selection
// by wave 0 that fills s.parent (row within the image) / s.word / s.lp, and beam_apply (everything after).
__device__ __forceinline__ void beam_load_rows(const BeamParams& p, BeamShared& s, int b, int t) {
  constexpr int NT = BEAM_NT;
  const int tid = threadIdx.x, k = p.k, T = p.T;
  for (int i = tid; i < k * k; i += NT) {
    s.cv[i] = p.cand_val[(long)b * k * k + i];
    s.ci[i] = p.cand_idx[(long)b * k * k + i];
  }
  for (int r = tid; r < k; r += NT) {
    s.eos[r] = p.has_eos[b * k + r]; s.ne[r] = p.n_elem[b * k + r]; s.cu[r] = p.cumul[b * k + r];
  }
  for (int i = tid; i < k * (t + 1); i += NT) {
    const int r = i / (t + 1), j = i - r * (t + 1);
    s.lpm[r][j] = p.lp[((long)b * k + r) * T + j];
  }
  __syncthreads();
}

// The extraction all three selections repeat (wave 0 only, all 64 lanes).  A lane holds BEAM_CPL candidates in registers:
// tot (what is ranked; -inf = none), key (unique among the live candidates) and val (the payload: what s.lp will hold).
// One call takes out the largest total, a tie going to the smaller key: every lane returns with the winner's key and
// payload and found = (its total > -inf; else bk = NO_KEY<K>), and the lane that owns the winner has retired it — by
// comparing every register slot with the winning key: a runtime index would send the arrays to scratch.  A selection =
// fill tot / key / val, extract n times, lane 0 decodes each key.
constexpr int BEAM_CPL = MAX_K * MAX_K / 64;           // candidates per lane: every selection ranks 256 at most
template <typename K> constexpr K NO_KEY = (K)(0x7fffffffffffffffLL >> (64 - 8 * (int)sizeof(K)));

template <typename K>
__device__ __forceinline__ bool wave_extract_best(float (&tot)[BEAM_CPL], K (&key)[BEAM_CPL], const float (&val)[BEAM_CPL],
                                                  K& bk, float& bval) {
  // (conditions joined with | and & on purpose: the short-circuit forms compile to a branch per candidate)
  float best = tot[0]; bval = val[0]; bk = key[0];
#pragma unroll
  for (int u = 1; u < BEAM_CPL; ++u) {
    const bool take = (tot[u] > best) | ((tot[u] == best) & (key[u] < bk));
    best = take ? tot[u] : best; bval = take ? val[u] : bval; bk = take ? key[u] : bk;
  }
  if (!(best > -INFINITY)) bk = NO_KEY<K>;             // nothing left in this lane
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64), ol = __shfl_xor(bval, o, 64);
    const K ok = __shfl_xor(bk, o, 64);
    const bool take = (ov > best) | ((ov == best) & (ok < bk));
    best = take ? ov : best; bval = take ? ol : bval; bk = take ? ok : bk;
  }
  const bool found = best > -INFINITY;
#pragma unroll
  for (int u = 0; u < BEAM_CPL; ++u) {
    const bool hit = found & (key[u] == bk);
    tot[u] = hit ? -INFINITY : tot[u]; key[u] = hit ? NO_KEY<K> : key[u];
  }
  return found;
}

// The arrival of one image's block (one thread): the block that arrives last advances *pos, raises *done when no image
// has a row still growing, and re-arms the counter.
__device__ __forceinline__ void beam_arrive(const BeamParams& p, int alive_any, int t) {
  const int prev = atomicAdd(p.ctr, 1 + (alive_any << 16));
  if ((prev & 0xffff) == p.n_img - 1) {                 // every block has read *pos before arriving here
    const int al = (prev >> 16) + alive_any;
    if (!al) *p.done = 1;
    *p.pos = t + 1;
    *p.ctr = 0;
  }
}

// s.parent / s.word / s.lp of the k rows are chosen (by wave 0; the barrier is here): new cumulative scores, the in-place
// permutation, the embedding tail, the per-beam outputs and the arrival counter.  `closing` (pool_beam.hip alone; block
// uniform): the image ends its search with this step — its rows are written as always but leave with row_valid = 0 and
// do not count as growing.
__device__ __forceinline__ void beam_apply(const BeamParams& p, const EmbedArgs& e, BeamShared& s, int b, int t,
                                           bool closing = false) {
  constexpr int NT = BEAM_NT;
  const int tid = threadIdx.x, k = p.k, T = p.T;
  __syncthreads();
  // cumulative score = re-summed per-token log-probs of the parent prefix + the new one (:213), in position order
  if (tid < k) {
    const float* src = s.lpm[s.parent[tid]];
    float cs = 0.f;
    for (int j = 0; j <= t; ++j) cs += src[j];
    s.cumul[tid] = cs + s.lp[tid];
  }
  const long base = (long)b * k * T;
  // one (row, column) element per thread and pass: all reads of the old rows, a barrier, then the writes
  constexpr int EPT = (MAX_K * MAX_T + NT - 1) / NT;
  long long tv[EPT]; float lv[EPT]; int av[EPT];
  const int cols = t + 1;
#pragma unroll
  for (int u = 0; u < EPT; ++u) {
    const int i = tid + u * NT;
    if (i < k * cols) {
      const int r = i / cols, j = i - r * cols;
      const long src = base + (long)s.parent[r] * T + j;
      tv[u] = p.tok[src]; lv[u] = p.lp[src];
      av[u] = j < t ? p.anc[src] : b * k + s.parent[r];
    }
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < EPT; ++u) {
    const int i = tid + u * NT;
    if (i < k * cols) {
      const int r = i / cols, j = i - r * cols;
      const long dst = base + (long)r * T + j;
      p.tok[dst] = tv[u]; p.lp[dst] = lv[u]; p.anc[dst] = av[u];
    }
  }
  if (e.embed && t + 2 < T && t + 1 < e.pos_rows) {     // input of the next position for the k chosen words (the
                                                        // last prefix position T-1 is never fed back; never past the table)
    const float* prow = e.pos_table + (long)(t + 1) * e.d;
    for (int i = tid; i < k * e.d; i += NT) {
      const int r = i / e.d, c = i - r * e.d;
      e.y[(long)(b * k + r) * e.ldy + c] = e.embed[(long)s.word[r] * e.d + c] * e.scale + prow[c];
    }
  }
  __syncthreads();                                      // s.cumul; every thread's reads of the old rows are done
  int alive = 0;
  if (tid < k) {
    const int r = tid, par = s.parent[r];
    const int pe = t == 0 ? 0 : s.eos[par];
    const int ne = t == 0 ? 1 : s.ne[par];
    const long dst = base + (long)r * T;
    p.tok[dst + t + 1] = (long long)s.word[r];
    p.lp[dst + t + 1] = s.lp[r];
    p.cumul[b * k + r] = s.cumul[r];
    p.n_elem[b * k + r] = ne + (pe ? 0 : 1);
    p.has_eos[b * k + r] = (pe || ((long long)s.word[r] == p.eos)) ? 1 : 0;
    p.row_valid[b * k + r] = (pe || closing) ? 0 : 1;
    p.next_tok[b * k + r] = (long long)s.word[r];
    alive = (pe || closing) ? 0 : 1;
  }
  if (tid < 64) {
    const int alive_any = __any(alive) ? 1 : 0;         // (k <= 16 lanes of wave 0 carry the flags)
    if (tid == 0) beam_arrive(p, alive_any, t);
  }
}

}  // namespace

// odic_beam_state / odic_embed_args → the kernel arguments, with the limits every step shares
static int beam_params(BeamParams& p, EmbedArgs& e, const odic_beam_state* st, const odic_embed_args* emb,
                       int32_t n_img, int32_t beams, int32_t T, int64_t eos_idx) {
  if (!st) return ODIC_ENULL;
  // T: k x (t+1) per-token log-probs are staged in LDS [MAX_K][MAX_T]; n_img: `alive << 16` in the counter
  if (n_img <= 0 || beams <= 0 || beams > MAX_K || T <= 1 || T > MAX_T || n_img > 32767) return ODIC_EINVAL;
  if (!st->tokens || !st->logprobs || !st->anc || !st->cumul || !st->n_elem || !st->has_eos || !st->row_valid ||
      !st->next_tok || !st->pos || !st->done || !st->ctr)
    return ODIC_ENULL;
  p.cand_val = nullptr; p.cand_idx = nullptr;
  p.tok = (long long*)st->tokens; p.lp = st->logprobs; p.anc = st->anc;
  p.cumul = st->cumul; p.n_elem = st->n_elem; p.has_eos = st->has_eos; p.row_valid = st->row_valid;
  p.next_tok = (long long*)st->next_tok; p.pos = st->pos; p.done = st->done; p.ctr = st->ctr;
  p.n_img = n_img; p.k = beams; p.T = T; p.eos = eos_idx;
  return odic_embed_args_from(e, emb);
}
