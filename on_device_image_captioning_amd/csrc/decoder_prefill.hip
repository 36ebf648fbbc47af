// Starting a search from a given prefix (gfx950, fp32): the two kernels that bring a beam state to position P without
// running P step chains.
//
//   dynexp_fill_caches_kernel   the per-position caches of dynexp_step_kernel (decoder_ops.hip) for positions 0..P-1 of a
//                               known sequence, written from the `lin` rows of the whole-sequence pass (decoder_seq.hip)
//   beam_reset_prefix_kernel    the beam state at *pos = P: every row of an image holds [sos, prefix], and only the first
//                               row of every group has a finite cumulative score, so that the unchanged step kernels seed
//                               at position P as they seed at position 0
#include "odic_common.h"
#include "dynexp_tiles.h"

namespace {

constexpr int FILL_MAX_T = 128;
constexpr int FILL_NT = 1024;     // threads per sequence
constexpr int RESET_MAX_K = 16;   // rows per image (odic_beam_step)

// ---------------------------------------------------------------------------------------------
// With s = 1/sqrt(d), for positions i <= t < P of sequence n (cache slot sl = n·rows_per_image):
//   cond | key | va | vb [t][sl]   = lin columns 0..4d of row n·P + t
//   qk[t][sl][e]                   = QK[e][t] = qexp[e]·key_t
//   wfa[t][sl][i][e]               = relu(z)·nfa[t][e],  z = (QK[e][i] + CK[t][i])·s,  CK[t][i] = cond_t·key_i,
//                                    nfa[t][e] = 1/(Σ_{i<=t} relu(z) + eps)           (wfb, nfb: relu(-z))
// the definitions of dynexp_step_kernel, expression for expression: `(q + dk) * inv_sqrt_d`, and the normaliser as 32
// lanes per (t, e), lane q summing i = q, q + 32, ... and the xor-shuffle 16, 8, 4, 2, 1 — given the same dot products the
// weights are the step kernel's bit for bit.  Nothing is written at i > t, at positions >= P or in another slot.
// One 1024-thread block per sequence.  LDS words: (E + P)·PS + 2·P·E with PS = P rounded up to 1 mod 4:
//   P = 19, E = 16 (a long prompt on the shipped decoder): 5.3 KB;  P = 127, E = 32 (the limits): 112 KB of the CU's
//   160 KB.  One block per CU at every P, and registers set it, not LDS: 75 VGPRs allow 6 waves per SIMD = 24 per CU, and a
//   block is 16 waves (no scratch).
// ---------------------------------------------------------------------------------------------
struct FillParams {
  const float* lin; long ldlin; const float* qexp;
  float* cond_c; float* key_c; float* va_c; float* vb_c; float* wfa_c; float* wfb_c; float* qk_c;
  int P, rpi, N, T, d, E, PS; float eps;
};

__global__ __launch_bounds__(FILL_NT) void dynexp_fill_caches_kernel(FillParams p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int d = p.d, E = p.E, P = p.P, PS = p.PS, tid = threadIdx.x;
  float* QK = sm;                                   // [E][PS]
  float* CK = QK + E * PS;                          // [P][PS]
  float* nfa = CK + P * PS;                         // [P][E]
  float* nfb = nfa + P * E;                         // [P][E]
  const float* lin = p.lin + (long)blockIdx.x * P * p.ldlin;
  const long NT = (long)p.N, sl = (long)blockIdx.x * p.rpi;
  const float inv_sqrt_d = rsqrtf((float)d);

  // the four row caches: whole rows, consecutive lanes = consecutive channels
  for (int q = tid; q < P * d; q += FILL_NT) {
    const int t = q / d, c = q - t * d;
    const float* row = lin + (long)t * p.ldlin + c;
    const long o = ((long)t * NT + sl) * d + c;
    p.cond_c[o] = row[0]; p.key_c[o] = row[d]; p.va_c[o] = row[2 * d]; p.vb_c[o] = row[3 * d];
  }
  dynexp_qk_ck_tiles<FILL_NT>(lin, p.ldlin, p.qexp, d, E, P, PS, QK, CK, tid);
  __syncthreads();

  for (int q = tid; q < P * E; q += FILL_NT) {
    const int t = q / E, e = q - t * E;
    p.qk_c[((long)t * NT + sl) * E + e] = QK[e * PS + t];
  }
  // forward normalisers: 32 lanes per (t, e); the trip count is the same for every lane (shuffles inside)
  for (int g0 = 0; g0 < P * E; g0 += FILL_NT / 32) {
    const int g = g0 + (tid >> 5), q = tid & 31;
    const int t = g / E, e = g - t * E;
    float sp = 0.f, sn = 0.f;
    if (g < P * E)
      for (int j = q; j <= t; j += 32) {
        const float z = (QK[e * PS + j] + CK[t * PS + j]) * inv_sqrt_d;
        sp += fmaxf(z, 0.f); sn += fmaxf(-z, 0.f);
      }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) { sp += __shfl_xor(sp, o, 64); sn += __shfl_xor(sn, o, 64); }
    if (q == 0 && g < P * E) { nfa[g] = 1.0f / (sp + p.eps); nfb[g] = 1.0f / (sn + p.eps); }
  }
  __syncthreads();

  // forward weights: wave w writes the rows t = w, w + 16, ...; a row is (t + 1)·E consecutive floats
  const int wave = tid >> 6, lane = tid & 63;
  for (int t = wave; t < P; t += FILL_NT / 64) {
    const long base = ((long)t * NT + sl) * p.T * E;
    float* wfa_t = p.wfa_c + base;
    float* wfb_t = p.wfb_c + base;
    for (int i = lane; i < (t + 1) * E; i += 64) {
      const int j = i / E, e = i - j * E;
      const float zf = (QK[e * PS + j] + CK[t * PS + j]) * inv_sqrt_d;
      wfa_t[i] = fmaxf(zf, 0.f) * nfa[t * E + e];
      wfb_t[i] = fmaxf(-zf, 0.f) * nfb[t * E + e];
    }
  }
}

// ---------------------------------------------------------------------------------------------
// One 256-thread block per image.  Row n = b·k + r:  tokens [sos, prefix[b]], logprobs [0, prefix_logp[b]], ancestors of
// the P cached positions = the image's first row (the slot odic_dynexp_fill_caches wrote), cumul = the log-probs summed
// in position order (what beam_apply re-sums) on the first row of every group of kg rows and -inf on the others: a
// total of -inf is never ranked (beam_select, group_beam_select), so the step at position P chooses among the candidates
// of one row per group — the seeding of position 0.
// ---------------------------------------------------------------------------------------------
struct ResetPrefixParams {
  long long* tok; float* lp; int* anc; float* cumul; int* n_elem; int* has_eos; int* row_valid; long long* next_tok;
  int* pos; int* done; int* ctr;
  const long long* prefix; const float* prefix_logp;
  EmbedArgs e;
  int k, kg, T, P; long long sos;
};

__global__ __launch_bounds__(256) void beam_reset_prefix_kernel(ResetPrefixParams p) {
  const int b = blockIdx.x, tid = threadIdx.x, k = p.k, T = p.T, P = p.P;
  const long long* pre = p.prefix + (long)b * P;
  const float* plp = p.prefix_logp + (long)b * P;
  for (int i = tid; i < k * (P + 1); i += 256) {
    const int r = i / (P + 1), j = i - r * (P + 1);
    const long o = ((long)b * k + r) * T + j;
    p.tok[o] = j == 0 ? p.sos : pre[j - 1];
    p.lp[o] = j == 0 ? 0.f : plp[j - 1];
    if (j < P) p.anc[o] = b * k;
  }
  if (tid < k) {
    const int n = b * k + tid;
    float cs = -INFINITY;
    if (tid % p.kg == 0) {
      cs = 0.f;                                   // (slot 0 holds 0)
      for (int j = 0; j < P; ++j) cs += plp[j];
    }
    p.cumul[n] = cs; p.n_elem[n] = P + 1; p.has_eos[n] = 0; p.row_valid[n] = 1; p.next_tok[n] = pre[P - 1];
  }
  if (b == 0 && tid == 0) { *p.pos = P; *p.done = 0; *p.ctr = 0; }
  const EmbedArgs& e = p.e;
  if (e.embed) {                                  // input of position P: the last prefix word
    const float* er = e.embed + pre[P - 1] * (long)e.d;
    const float* prow = e.pos_table + (long)P * e.d;
    for (int i = tid; i < k * e.d; i += 256) {
      const int r = i / e.d, c = i - r * e.d;
      e.y[((long)b * k + r) * e.ldy + c] = er[c] * e.scale + prow[c];
    }
  }
}

}  // namespace

extern "C" int odic_dynexp_fill_caches(const float* lin, int64_t ldlin, const float* qexp, float* cond_c, float* key_c,
                                       float* va_c, float* vb_c, float* wfa_c, float* wfb_c, float* qk_c, int32_t n_seq,
                                       int32_t P, int32_t rows_per_image, int32_t N_cache, int32_t T_cache, int32_t d,
                                       int32_t E, float eps, void* stream) {
  if (!lin || !qexp || !cond_c || !key_c || !va_c || !vb_c || !wfa_c || !wfb_c || !qk_c) return ODIC_ENULL;
  if (n_seq <= 0 || P < 1 || T_cache > FILL_MAX_T || P >= T_cache || d <= 0 || d % 64) return ODIC_EINVAL;
  if (E != 4 && E != 8 && E != 16 && E != 32) return ODIC_EINVAL;
  if (rows_per_image < 1 || N_cache < 1 || (int64_t)(n_seq - 1) * rows_per_image >= N_cache) return ODIC_EINVAL;
  if (ldlin < 5 * (int64_t)d || (ldlin & 3) || ((uintptr_t)lin & 15) || ((uintptr_t)qexp & 15)) return ODIC_EINVAL;
  FillParams p;
  p.lin = lin; p.ldlin = ldlin; p.qexp = qexp; p.cond_c = cond_c; p.key_c = key_c; p.va_c = va_c; p.vb_c = vb_c;
  p.wfa_c = wfa_c; p.wfb_c = wfb_c; p.qk_c = qk_c;
  p.P = P; p.rpi = rows_per_image; p.N = N_cache; p.T = T_cache; p.d = d; p.E = E; p.eps = eps;
  p.PS = P + ((5 - (P & 3)) & 3);           // P rounded up to 1 mod 4: odd row stride
  const size_t shmem = ((size_t)(E + P) * p.PS + 2 * (size_t)P * E) * sizeof(float);
  if (shmem > 160 * 1024) return ODIC_EINVAL;
  static bool raised = false;               // the first call is never inside a capture
  if (!raised) {
    (void)hipFuncSetAttribute((const void*)dynexp_fill_caches_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    raised = true;
  }
  hipLaunchKernelGGL(dynexp_fill_caches_kernel, dim3(n_seq), dim3(FILL_NT), shmem, (hipStream_t)stream, p);
  return odic_launch_status();
}

extern "C" int odic_beam_reset_prefix(const odic_beam_state* st, const odic_embed_args* emb, const int64_t* prefix,
                                      const float* prefix_logp, int32_t n_img, int32_t beams, int32_t group_beams,
                                      int32_t T, int32_t P, int64_t sos_idx, void* stream) {
  if (!st || !prefix || !prefix_logp) return ODIC_ENULL;
  if (n_img <= 0 || n_img > 32767 || beams <= 0 || beams > RESET_MAX_K || T <= 1 || T > FILL_MAX_T) return ODIC_EINVAL;
  if (group_beams < 1 || beams % group_beams || P < 1 || P > T - 2) return ODIC_EINVAL;
  if (!st->tokens || !st->logprobs || !st->anc || !st->cumul || !st->n_elem || !st->has_eos || !st->row_valid ||
      !st->next_tok || !st->pos || !st->done || !st->ctr)
    return ODIC_ENULL;
  ResetPrefixParams p;
  p.tok = (long long*)st->tokens; p.lp = st->logprobs; p.anc = st->anc; p.cumul = st->cumul; p.n_elem = st->n_elem;
  p.has_eos = st->has_eos; p.row_valid = st->row_valid; p.next_tok = (long long*)st->next_tok;
  p.pos = st->pos; p.done = st->done; p.ctr = st->ctr;
  p.prefix = (const long long*)prefix; p.prefix_logp = prefix_logp;
  const int rc = odic_embed_args_from(p.e, emb);
  if (rc != 0) return rc;
  if (emb && (p.e.pos_rows <= P || p.e.ldy < p.e.d)) return ODIC_EINVAL;               // pos_table row P is read
  p.k = beams; p.kg = group_beams; p.T = T; p.P = P; p.sos = sos_idx;
  hipLaunchKernelGGL(beam_reset_prefix_kernel, dim3(n_img), dim3(256), 0, (hipStream_t)stream, p);
  return odic_launch_status();
}
