// Whole-sequence (teacher-forced) decoder kernels for gfx950 (fp32): every position of every sequence in one launch.
//
// The search path (decoder_ops.hip) processes ONE new position per launch against per-position caches in global memory,
// because the next token is not known yet.  Scoring a caption that already exists knows every token up front, so the
// N·T rows go through the linear layers as one M = N·T product each (odic_gemm) and the kernels here do the parts that
// couple the positions of a sequence:
//
//   dec_embed_seq_kernel   y[n·T + t] = embed[tok[n][t]]·sqrt(d) + pos_table[t]  (+ the [N·T] row-validity flags)
//   dynexp_seq_kernel      DynamicExpansionBlock (layers.py:152-204) for all positions of a sequence, nothing cached
//                          in global memory
//   token_stats_kernel     the scoring tail: per logits row the target's log-prob, Σ_v log-prob, arg-max and its
//                          log-prob — one number per quantity instead of an [R, V] log-prob tensor (ranking
//                          and block reductions: row_select.h)
//   cross_attn_probs_kernel  the softmax probabilities of the cross attention themselves (where the model looked for
//                          each word): what cross_attn_step_kernel computes in LDS, uses for P·V and discards
#include "row_select.h"
#include "dynexp_tiles.h"

namespace {

constexpr int SEQ_MAX_T = 128;
constexpr int SEQ_NT = 1024;      // threads per sequence
constexpr int SEQ_TR = 16;        // output rows per phase-2 tile

// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dec_embed_seq_kernel(const long long* __restrict__ tokens,
                                                            const float* __restrict__ embed,
                                                            const float* __restrict__ pos_table,
                                                            const int* __restrict__ dec_len, int* __restrict__ row_valid,
                                                            float* __restrict__ y, long ldy, int T, int d, int vocab,
                                                            float scale) {
  const long row = blockIdx.x;            // n·T + t
  const int n = (int)(row / T), t = (int)(row - (long)n * T);
  const long tok = tokens[row];
  const bool ok = tok >= 0 && tok < vocab;      // an id outside the table embeds as zero: nothing is read out of bounds
  const float* er = embed + (ok ? tok : 0) * (long)d;
  const float sc = ok ? scale : 0.f;
  for (int c = threadIdx.x; c < d; c += blockDim.x) y[row * ldy + c] = er[c] * sc + pos_table[(long)t * d + c];
  if (row_valid && threadIdx.x == 0) row_valid[row] = t < dec_len[n] ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------
// Dynamic expansion of a whole sequence.  With s = 1/sqrt(d), L = dec_len[n] and, for positions i, j, t < L,
//   QK[e][j] = qexp[e]·key_j          CK[i][j] = cond_i·key_j                 (an E x L and an L x L product)
//   forward   zf(j,e,i) = (QK[e][i] + CK[j][i])·s,  i <= j     nfa[e][j] = 1/(Σ_{i<=j} relu(zf) + eps)   (nfb: relu(-zf))
//   backward  zb(t,j,e) = (QK[e][t] + CK[j][t])·s,  j <= t     nba[t]   = 1/(Σ_{j<=t,e} relu(zb) + eps)  (nbb: relu(-zb))
// the reference's output row t is  Σ_{j<=t,e} wba(t,j,e)·(Σ_{i<=j} wfa(j,e,i)·va_i + bexp[e] + cond_j); re-associated as in
// dynexp_step_kernel (include/odic_hip.h) it is
//   out_a[t] = Σ_{i<=t} ca[t][i]·va_i + Σ_{j<=t} wja[t][j]·cond_j + Σ_e wea[t][e]·bexp[e]
//   ca[t][i] = nba[t]·Σ_{j=i..t} Σ_e relu(zb(t,j,e))·relu(zf(j,e,i))·nfa[e][j]
//   wja[t][j] = nba[t]·Σ_e relu(zb(t,j,e))          wea[t][e] = nba[t]·Σ_{j<=t} relu(zb(t,j,e))
// and the same with relu(-z) for out_b;  y[t] = y_in[t] + σ(sel_t)·out_a[t] + (1-σ(sel_t))·out_b[t].
// Causality and the padding mask are the loop bounds: a position t >= L adds nothing (its weights are 0/(0+eps)) and no
// valid position ever looks at one.
//
// One 1024-thread block per sequence.  QK, CK and the normalisers live in LDS for the whole block (the forward weights
// themselves — L·E·L values — would not fit and are recomputed from QK / CK where they are used: two adds, two max and
// a multiply); the coefficient rows ca | cb | wja | wjb exist for SEQ_TR = 16 output rows at a time.
//   LDS words: E·TS + T·TS + 2·E·TS + 2·T + 4·TR·T + 2·TR·E   with TS = T rounded up to 1 mod 4
//     T = 73, E = 16 (COCO evaluation length, the shipped decoder): 57 KB;  T = 128, E = 32 (the limits): 153 KB of the
//     CU's 160 KB.  Occupancy is ONE block per CU at every T, and registers set it, not LDS: 90 VGPRs allocate 96, that
//     is 5 waves per SIMD = 20 per CU, and a block is 16 waves.
//   phase 1  (L+E) x L dot products of length d as 4 x 4 register tiles, float4 loads from the lin rows
//   phase 2  per row tile: coefficients (one thread per (t, i), consecutive lanes = consecutive i: QK / nf rows are read
//            at consecutive addresses, CK rows with an odd stride), then thread = (channel, 8 rows) accumulates the three
//            sums over i with coalesced loads of va_i | vb_i | cond_i and one 16-byte LDS read per (row, i).
// ---------------------------------------------------------------------------------------------
struct DynSeqParams {
  const float* lin; long ldlin; const float* qexp; const float* bexp; const int* dec_len;
  const float* y_in; long ldyi; float* y; long ldy;
  int N, T, d, E, TS; float eps;
};

__global__ __launch_bounds__(SEQ_NT) void dynexp_seq_kernel(DynSeqParams p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int d = p.d, E = p.E, T = p.T, TS = p.TS, n = blockIdx.x, tid = threadIdx.x;
  constexpr int TR = SEQ_TR;
  float4* coef = (float4*)sm;                       // [T][TR] {ca, cb, wja, wjb}
  float* we = sm + 4 * TR * T;                      // [TR][E][2]
  float* QK = we + 2 * TR * E;                      // [E][TS]
  float* CK = QK + E * TS;                          // [T][TS]
  float* nfa = CK + T * TS;                         // [E][TS]
  float* nfb = nfa + E * TS;                        // [E][TS]
  float* nba = nfb + E * TS;                        // [T]
  float* nbb = nba + T;                             // [T]

  const int L = max(0, min(p.dec_len[n], T));
  const float* lin = p.lin + (long)n * T * p.ldlin;
  const float* yin = p.y_in + (long)n * T * p.ldyi;
  float* yout = p.y + (long)n * T * p.ldy;
  const float s = rsqrtf((float)d);

  // rows [L, T): nothing is added
  for (long q = tid; q < (long)(T - L) * d; q += SEQ_NT) {
    const int t = L + (int)(q / d), c = (int)(q % d);
    yout[(long)t * p.ldy + c] = yin[(long)t * p.ldyi + c];
  }
  if (L == 0) return;

  // ---- phase 1: rows a < L are cond_a, rows L..L+E-1 are qexp; columns are key_b
  dynexp_qk_ck_tiles<SEQ_NT>(lin, p.ldlin, p.qexp, d, E, L, TS, QK, CK, tid);       // (dynexp_tiles.h)
  __syncthreads();

  // ---- normalisers.  forward: one thread per (e, j); backward: 16 lanes per t, fixed shuffle order
  for (int it = tid; it < E * L; it += SEQ_NT) {
    const int e = it / L, j = it - e * L;
    float sp = 0.f, sn = 0.f;
    for (int i = 0; i <= j; ++i) {
      const float z = (QK[e * TS + i] + CK[j * TS + i]) * s;
      sp += fmaxf(z, 0.f); sn += fmaxf(-z, 0.f);
    }
    nfa[e * TS + j] = 1.0f / (sp + p.eps);
    nfb[e * TS + j] = 1.0f / (sn + p.eps);
  }
  {
    const int grp = tid >> 4, gl = tid & 15;
    for (int t = grp; t < ((L + SEQ_NT / 16 - 1) / (SEQ_NT / 16)) * (SEQ_NT / 16); t += SEQ_NT / 16) {
      float sp = 0.f, sn = 0.f;
      if (t < L)
        for (int q = gl; q < (t + 1) * E; q += 16) {
          const int j = q / E, e = q - j * E;
          const float z = (QK[e * TS + t] + CK[j * TS + t]) * s;
          sp += fmaxf(z, 0.f); sn += fmaxf(-z, 0.f);
        }
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) { sp += __shfl_xor(sp, o, 64); sn += __shfl_xor(sn, o, 64); }
      if (gl == 0 && t < L) { nba[t] = 1.0f / (sp + p.eps); nbb[t] = 1.0f / (sn + p.eps); }
    }
  }
  __syncthreads();

  // ---- phase 2, SEQ_TR output rows at a time
  for (int t0 = 0; t0 < L; t0 += TR) {
    const int rows = min(TR, L - t0);            // valid rows of this tile
    const int tmax = t0 + rows - 1;              // last position any of them looks at
    // coefficients; entries with i > t are zero so that the channel loop below needs no per-row bound
    for (int it = tid; it < TR * (tmax + 1); it += SEQ_NT) {
      const int r = it / (tmax + 1), i = it - r * (tmax + 1);
      const int t = t0 + r;
      float sa = 0.f, sb = 0.f, ja = 0.f, jb = 0.f;
      if (r < rows && i <= t) {
        for (int j = i; j <= t; ++j) {
          const float ckt = CK[j * TS + t], cki = CK[j * TS + i];
          for (int e = 0; e < E; ++e) {
            const float zb = (QK[e * TS + t] + ckt) * s;
            const float zf = (QK[e * TS + i] + cki) * s;
            sa = fmaf(fmaxf(zb, 0.f) * fmaxf(zf, 0.f), nfa[e * TS + j], sa);
            sb = fmaf(fmaxf(-zb, 0.f) * fmaxf(-zf, 0.f), nfb[e * TS + j], sb);
          }
        }
        const float cit = CK[i * TS + t];        // wja[t][i]: the backward weights of position i summed over e
        for (int e = 0; e < E; ++e) {
          const float zb = (QK[e * TS + t] + cit) * s;
          ja += fmaxf(zb, 0.f); jb += fmaxf(-zb, 0.f);
        }
        const float na = nba[t], nb = nbb[t];
        sa *= na; ja *= na; sb *= nb; jb *= nb;
      }
      coef[i * TR + r] = make_float4(sa, sb, ja, jb);
    }
    for (int it = tid; it < TR * E; it += SEQ_NT) {
      const int r = it / E, e = it - r * E;
      const int t = t0 + r;
      float ea = 0.f, eb = 0.f;
      if (r < rows) {
        const float qt = QK[e * TS + t];
        for (int j = 0; j <= t; ++j) {
          const float zb = (qt + CK[j * TS + t]) * s;
          ea += fmaxf(zb, 0.f); eb += fmaxf(-zb, 0.f);
        }
        ea *= nba[t]; eb *= nbb[t];
      }
      we[2 * it] = ea; we[2 * it + 1] = eb;
    }
    __syncthreads();
    // channel sums: thread = (channel c, 8 rows of the tile)
    constexpr int RG = 8;
    for (int it = tid; it < d * (TR / RG); it += SEQ_NT) {
      const int c = it % d, r0 = (it / d) * RG;
      if (r0 >= rows) continue;
      float oa[RG], ob[RG];
#pragma unroll
      for (int r = 0; r < RG; ++r) { oa[r] = 0.f; ob[r] = 0.f; }
      const int iend = min(tmax, t0 + r0 + RG - 1);
      for (int i = 0; i <= iend; ++i) {
        const float* li = lin + (long)i * p.ldlin + c;
        const float cj = li[0], va = li[2 * d], vb = li[3 * d];
        const float4* cf = coef + i * TR + r0;
#pragma unroll
        for (int r = 0; r < RG; ++r) {
          const float4 w = cf[r];
          oa[r] = fmaf(w.x, va, oa[r]); oa[r] = fmaf(w.z, cj, oa[r]);
          ob[r] = fmaf(w.y, vb, ob[r]); ob[r] = fmaf(w.w, cj, ob[r]);
          asm volatile("" : "+v"(oa[r]), "+v"(ob[r]));      // (kept scalar, as above)
        }
      }
      for (int e = 0; e < E; ++e) {
        const float be = p.bexp[(long)e * d + c];
#pragma unroll
        for (int r = 0; r < RG; ++r) {
          oa[r] = fmaf(we[2 * ((r0 + r) * E + e)], be, oa[r]);
          ob[r] = fmaf(we[2 * ((r0 + r) * E + e) + 1], be, ob[r]);
          asm volatile("" : "+v"(oa[r]), "+v"(ob[r]));
        }
      }
#pragma unroll
      for (int r = 0; r < RG; ++r) {
        const int t = t0 + r0 + r;
        if (r0 + r < rows) {
          const float sg = 1.0f / (1.0f + expf(-lin[(long)t * p.ldlin + 4 * d + c]));
          yout[(long)t * p.ldy + c] = yin[(long)t * p.ldyi + c] + sg * oa[r] + (1.0f - sg) * ob[r];
        }
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
// Scoring tail: one 256-thread block per logits row, two passes over the row (the second one hits the cache).
//   pass 1: maximum with its lowest index, pass 2: Σ exp(x - max) in fp32 and Σ (x - max) in fp64 (V terms of
//   magnitude ~10: an fp32 sum would carry an error of the size of one term's last bits times V)
// ---------------------------------------------------------------------------------------------
constexpr int TS_NT = 256;

__global__ __launch_bounds__(TS_NT) void token_stats_kernel(const float* __restrict__ logits, long ldl,
                                                            const long long* __restrict__ target,
                                                            float* __restrict__ logp_target, float* __restrict__ sum_logp,
                                                            int* __restrict__ argmax, float* __restrict__ max_logp,
                                                            int* __restrict__ status, int V) {
  __shared__ ArgmaxSlots<TS_NT / 64> s_m;
  __shared__ float s_e[TS_NT / 64];
  __shared__ double s_d[TS_NT / 64];
  const long row = blockIdx.x;
  const float* x = logits + row * ldl;
  const int tid = threadIdx.x;
  float m = -INFINITY; int mi = 0x7fffffff;
  for (int i = tid; i < V; i += TS_NT) {
    const float v = x[i];
    if (v > m || mi == 0x7fffffff) { m = v; mi = i; }   // (a thread's first element always: an all -inf or NaN row)
  }
  block_argmax<TS_NT / 64>(m, mi, s_m, 0);
  float se = 0.f; double sx = 0.0;
  for (int i = tid; i < V; i += TS_NT) {
    const float dv = x[i] - m;
    se += expf(dv); sx += (double)dv;
  }
  const float e = block_sum(se, s_e);
  const double dsum = block_sum(sx, s_d);     // wave 0 first, ascending: sum_logp keeps its bits
  if (tid == 0) {
    const float lg = logf(e);                 // logsumexp = m + lg
    sum_logp[row] = (float)(dsum - (double)V * (double)lg);
    argmax[row] = mi;
    max_logp[row] = -lg;
    if (target) {
      const long long tg = target[row];
      if (tg >= 0 && tg < V) logp_target[row] = (x[tg] - m) - lg;
      else { logp_target[row] = 0.f; atomicOr(status, 1); }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Cross-attention probabilities: one 256-thread block per (image, chunk of R query rows of that image), looping over the
// heads.  Per head
//   q       the nr x dk slice of the chunk's query rows → LDS
//   scores  thread = key: its dk-float K row is read ONCE (float4, as cross_attn_step_kernel reads it) into registers
//           and used for all nr rows (the q row comes from LDS as a broadcast); masked exactly as the step kernel
//   softmax wave w normalises rows w, w + 4, ...; lane l owns keys l, l + 64, ... of a row in every head, so the
//           head sum (acc[r][s], fixed head order) and the final store are by ONE thread per element: no atomics,
//           and nothing depends on the grid or on R
// LDS words: R·dk + 2·R·S + R;  R = 16 rows at S = 144, dk = 64 (the shipped decoder): 22.6 KB, so registers, not LDS,
// bound the blocks per CU; the host halves R until the block fits 64 KB (S = 576: R = 8, 39 KB — two blocks a CU).
// Products and sums that reach `out` are __fmul_rn / __fadd_rn: never contracted into an FMA, so accumulate = 1 adds
// exactly what accumulate = 0 would have stored.
// ---------------------------------------------------------------------------------------------
constexpr int AP_NT = 256;
constexpr int AP_MAX_R = 16;
constexpr size_t AP_MAX_LDS = 64 * 1024;

template <int DK>
__global__ __launch_bounds__(AP_NT) void cross_attn_probs_kernel(const float* __restrict__ q, long ldq,
                                                                 const float* __restrict__ kv, long ldkv, int koff,
                                                                 const int* __restrict__ enc_len,
                                                                 const int* __restrict__ row_valid, float* out,
                                                                 long ldo, int rows, int S, int heads, int R,
                                                                 int per_head, int accumulate, float scale) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* qs = sm;                                  // [R][DK]
  float* sc = qs + R * DK;                         // [R][S]  scores → exp of the current head
  float* acc = sc + R * S;                         // [R][S]  Σ_h p_h   (per_head = 0)
  int* vld = (int*)(acc + R * S);                  // [R]
  const int img = blockIdx.x, r0 = blockIdx.y * R;
  const int nr = min(R, rows - r0);                // rows handled here
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long n0 = (long)img * rows + r0;           // first query row of this block
  const int len = enc_len[img];
  const float inv = rsqrtf((float)DK);
  const float* kvb = kv + (long)img * S * ldkv + koff;
  if (tid < nr) vld[tid] = row_valid[n0 + tid];

  for (int h = 0; h < heads; ++h) {
    for (int e = tid; e < nr * DK; e += AP_NT) {
      const int r = e / DK, c = e - r * DK;
      qs[e] = q[(n0 + r) * ldq + h * DK + c];
    }
    __syncthreads();       // q (and vld) visible; every wave is through the previous head's softmax: sc may be rewritten
    for (int s = tid; s < S; s += AP_NT) {
      float4 k4[DK / 4];
      const float* kr = kvb + (long)s * ldkv + h * DK;
#pragma unroll
      for (int i = 0; i < DK / 4; ++i) k4[i] = *(const float4*)(kr + 4 * i);
      for (int r = 0; r < nr; ++r) {
        const float4* qr = (const float4*)(qs + r * DK);
        float a = 0.f;
#pragma unroll
        for (int i = 0; i < DK / 4; ++i) {
          const float4 qq = qr[i];
          a = fmaf(qq.x, k4[i].x, a); a = fmaf(qq.y, k4[i].y, a);
          a = fmaf(qq.z, k4[i].z, a); a = fmaf(qq.w, k4[i].w, a);
        }
        float v = a * inv;
        if (!vld[r] || s >= len) v = -1e4f;        // masked_fill(mask == 0, -1e4), layers.py:286
        sc[r * S + s] = v;
      }
    }
    __syncthreads();
    for (int r = wave; r < nr; r += AP_NT / 64) {
      float* row = sc + r * S;
      float m = -INFINITY;
      for (int s = lane; s < S; s += 64) m = fmaxf(m, row[s]);
      m = wave_max(m);
      float l = 0.f;
      for (int s = lane; s < S; s += 64) { const float e = expf(row[s] - m); row[s] = e; l += e; }
      l = wave_sum(l);
      for (int s = lane; s < S; s += 64) {
        const float p = row[s] / l;
        if (per_head) {
          float* o = out + (n0 + r) * ldo + (long)h * S + s;
          const float v = __fmul_rn(scale, p);
          *o = accumulate ? __fadd_rn(*o, v) : v;
        } else {
          acc[r * S + s] = h == 0 ? p : __fadd_rn(acc[r * S + s], p);
        }
      }
    }
  }
  if (!per_head)                                   // the thread that summed an element stores it
    for (int r = wave; r < nr; r += AP_NT / 64)
      for (int s = lane; s < S; s += 64) {
        float* o = out + (n0 + r) * ldo + s;
        const float v = __fmul_rn(scale, acc[r * S + s]);
        *o = accumulate ? __fadd_rn(*o, v) : v;
      }
}

}  // namespace

extern "C" int odic_dec_embed_seq(const int64_t* tokens, const float* embed, const float* pos_table,
                                  const int32_t* dec_len, int32_t* row_valid, float* y, int64_t ldy, int32_t N,
                                  int32_t T, int32_t d, int32_t vocab, int32_t pos_rows, float scale, void* stream) {
  if (!tokens || !embed || !pos_table || !y) return ODIC_ENULL;
  if (row_valid && !dec_len) return ODIC_ENULL;
  if (N <= 0 || T <= 0 || d <= 0 || vocab <= 0 || pos_rows <= 0 || T > pos_rows || ldy < d) return ODIC_EINVAL;
  if ((int64_t)N * T > 0x7fffffff) return ODIC_EINVAL;
  hipLaunchKernelGGL(dec_embed_seq_kernel, dim3((unsigned)(N * T)), dim3(256), 0, (hipStream_t)stream,
                     (const long long*)tokens, embed, pos_table, dec_len, row_valid, y, (long)ldy, T, d, vocab, scale);
  return odic_launch_status();
}

extern "C" int odic_dynexp_seq(const float* lin, int64_t ldlin, const float* qexp, const float* bexp,
                               const int32_t* dec_len, const float* y_in, int64_t ldy_in, float* y, int64_t ldy,
                               int32_t N, int32_t T, int32_t d, int32_t E, float eps, void* stream) {
  if (!lin || !qexp || !bexp || !dec_len || !y_in || !y) return ODIC_ENULL;
  if (N <= 0 || T <= 0 || T > SEQ_MAX_T || d <= 0 || d % 64) return ODIC_EINVAL;
  if (E != 4 && E != 8 && E != 16 && E != 32) return ODIC_EINVAL;
  if (ldlin < 5 * (int64_t)d || (ldlin & 3) || ldy_in < d || ldy < d || ((uintptr_t)lin & 15) || ((uintptr_t)qexp & 15))
    return ODIC_EINVAL;
  DynSeqParams p;
  p.lin = lin; p.ldlin = ldlin; p.qexp = qexp; p.bexp = bexp; p.dec_len = dec_len; p.y_in = y_in; p.ldyi = ldy_in;
  p.y = y; p.ldy = ldy; p.N = N; p.T = T; p.d = d; p.E = E; p.eps = eps;
  p.TS = T + ((5 - (T & 3)) & 3);           // T rounded up to 1 mod 4: odd row stride, 2-way conflicts at worst
  const size_t shmem = ((size_t)4 * SEQ_TR * T + 2 * SEQ_TR * E + (size_t)(3 * E + T) * p.TS + 2 * T) * sizeof(float);
  if (shmem > 160 * 1024) return ODIC_EINVAL;
  static bool raised = false;               // the first call is never inside a capture
  if (!raised) {
    (void)hipFuncSetAttribute((const void*)dynexp_seq_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    raised = true;
  }
  hipLaunchKernelGGL(dynexp_seq_kernel, dim3(N), dim3(SEQ_NT), shmem, (hipStream_t)stream, p);
  return odic_launch_status();
}

extern "C" int odic_token_stats(const float* logits, int64_t ldl, const int64_t* target, float* logp_target,
                                float* sum_logp, int32_t* argmax, float* max_logp, int32_t* status, int32_t R,
                                int32_t V, void* stream) {
  if (!logits || !sum_logp || !argmax || !max_logp) return ODIC_ENULL;
  if (target && (!logp_target || !status)) return ODIC_ENULL;
  if (R <= 0 || V <= 0 || ldl < V) return ODIC_EINVAL;
  hipLaunchKernelGGL(token_stats_kernel, dim3(R), dim3(TS_NT), 0, (hipStream_t)stream, logits, (long)ldl,
                     (const long long*)target, logp_target, sum_logp, argmax, max_logp, status, V);
  return odic_launch_status();
}

extern "C" int odic_cross_attn_probs(const float* q, int64_t ldq, const float* kv, int64_t ldkv, int32_t koff,
                                     const int32_t* enc_len, const int32_t* row_valid, float* out, int64_t ldo,
                                     int32_t N, int32_t n_img, int32_t S, int32_t d, int32_t heads, int32_t per_head,
                                     int32_t accumulate, float scale, void* stream) {
  if (!q || !kv || !enc_len || !row_valid || !out) return ODIC_ENULL;
  if (N < 1 || n_img < 1 || N % n_img || S < 1 || d < 1 || heads < 1 || d % heads) return ODIC_EINVAL;
  const int dk = d / heads;
  if (dk != 16 && dk != 32 && dk != 64) return ODIC_EINVAL;
  if ((ldq & 3) || (ldkv & 3) || (koff & 3) || koff < 0 || ((uintptr_t)q & 15) || ((uintptr_t)kv & 15)) return ODIC_EINVAL;
  if (ldq < d || ldkv < (int64_t)koff + d) return ODIC_EINVAL;
  if (ldo < (per_head ? (int64_t)heads * S : (int64_t)S)) return ODIC_EINVAL;
  const int rows = N / n_img;
  int R = rows < AP_MAX_R ? rows : AP_MAX_R;
  auto lds = [&](int r) { return ((size_t)r * dk + 2 * (size_t)r * S + r) * sizeof(float); };
  while (R > 1 && lds(R) > AP_MAX_LDS) R = (R + 1) / 2;
  if (lds(R) > AP_MAX_LDS) return ODIC_EINVAL;      // one row of scores + sums does not fit: S > 8159 at dk = 64
  const int chunks = (rows + R - 1) / R;
  if (chunks > 65535) return ODIC_EINVAL;
#define ODIC_APROBS(DK)                                                                                              \
  hipLaunchKernelGGL(cross_attn_probs_kernel<DK>, dim3(n_img, chunks), dim3(AP_NT), lds(R), (hipStream_t)stream, q,  \
                     (long)ldq, kv, (long)ldkv, koff, enc_len, row_valid, out, (long)ldo, rows, S, heads, R,         \
                     per_head ? 1 : 0, accumulate ? 1 : 0, scale)
  if (dk == 16) ODIC_APROBS(16);
  else if (dk == 32) ODIC_APROBS(32);
  else ODIC_APROBS(64);
#undef ODIC_APROBS
  return odic_launch_status();
}
