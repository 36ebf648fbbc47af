// Incremental decoder-step kernels for gfx950 (fp32) — SURVEY §8 rows A13-A19.
//
// The reference re-runs the whole prefix every step (O(T²)); its decoder is strictly causal, so we
// process ONE new position per step against per-position caches.  Beam re-ordering never moves a
// cache: `anc[n][j]` names the slot (sequence index at the time position j was processed) whose
// entry belongs to sequence n's history.  Every kernel reads the current position from device
// memory (`*pos`) so the same captured graph serves every step.
//
//   dec_embed_kernel         y = embed[tok]·sqrt(d) + pos_table[pos]
//   dynexp_step_kernel       DynamicExpansionBlock for the newest row (layers.py:152-204)
//   cross_attn_step_kernel   MultiHeadAttention against per-image cached K/V (layers.py:266-295)
//   logsoftmax_topk_kernel   log_softmax over the vocabulary + top-k (captioning_model.py:162-170); <false>: top-k alone
//   logsoftmax_sample_kernel log_softmax + k draws without replacement (Gumbel top-k)
//   ensemble_logprob_kernel  log of the mean of the models' softmaxes
//   beam_step_kernel         candidate masking, k·k selection, prefix/ancestor re-gather (:172-223)
//   group_beam_step_kernel   the same step for diverse (group) beam search: groups choose in turn, Hamming penalty
//   require_beam_step_kernel the same step for required words: 2^C banks of beams, one per set of words mentioned so far
//   beam_finalize_kernel     length-normalised ranking (:225-227)
// The row kernels (the three above that work on vocabulary rows) rank and reduce with row_select.h.
#include "row_sample.h"
#include "beam_step.h"

namespace {

constexpr int MAX_E = 32;      // max expansion vectors per position

// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dec_embed_kernel(const long long* __restrict__ tokens,
                                                        const float* __restrict__ embed,
                                                        const float* __restrict__ pos_table,
                                                        const int* __restrict__ pos, float* __restrict__ y,
                                                        long ldy, int N, int d, int pos_rows, float scale) {
  const int n = blockIdx.x;
  const long tok = tokens[n];
  const int p = *pos;
  if (p < 0 || p >= pos_rows) return;   // *pos is device memory no host check can see: a replay past the table's last
                                        // row (End_ExpansionNet_v2.py:105 caps the positions at max_seq_len) writes nothing
  for (int c = threadIdx.x; c < d; c += blockDim.x)
    y[n * ldy + c] = embed[tok * d + c] * scale + pos_table[(long)p * d + c];
}

// ---------------------------------------------------------------------------------------------
// Dynamic expansion for the newest position.  With t = *pos and slot(j) = (j < t ? anc[n][j] : n):
//   forward  z_fw[e][i] = (qexp[e] + cond_t)·key_i / sqrt(d)            i <= t
//            wfa_t[i][e] = relu(z_fw)/(Σ_i relu(z_fw) + eps),  wfb_t with -z        (CACHED: (t+1)·E scalars each)
//            class vectors of the reference:  afull_t[e] = Σ_i wfa_t[i][e]·va_i + bexp[e] + cond_t   (never formed)
//   backward z_bw[j][e] = (qexp[e] + cond_j)·key_t / sqrt(d)            j <= t
//            wba[j][e] = relu(z_bw)/(Σ_{j,e} relu(z_bw) + eps),  wbb with -z
//            out_a = Σ_{j,e} wba[j][e]·afull_j[e]
//                  = Σ_i ca[i]·va_i + Σ_e wea[e]·bexp[e] + Σ_j wja[j]·cond_j
//              with ca[i] = Σ_{j>=i} Σ_e wba[j][e]·wfa_j[i][e],  wea[e] = Σ_j wba[j][e],  wja[j] = Σ_e wba[j][e]
//   y_out = y_in + σ(sel)·out_a + (1-σ(sel))·out_b        (nothing is added on a padded row)
// The reference (layers.py:152-204) materialises the (t·E) x d class matrices every step; a cache of afull / bfull
// per position would be 2·E·d floats per position and sequence (64 KB at E = 16, d = 512: 100 MB read per step at
// t = 10 for 48 sequences x 3 layers, streamed beside the encoder's GEMMs).  Re-associating the double sum moves the
// cache to the forward WEIGHTS — (t+1)·E scalars per position — and the step to 3·(t+1) + E rows of d floats per
// sequence: 8x fewer bytes, same arithmetic up to summation order.
// The dot products split as qexp[e]·key + cond·key; qexp[e]·key_j is cached per position (qk_c).
// ---------------------------------------------------------------------------------------------
struct DynParams {
  const float* lin; long ldlin; const float* qexp; const float* bexp;
  float* cond_c; float* key_c; float* va_c; float* vb_c; float* wfa_c; float* wfb_c; float* qk_c;
  const int* anc; const int* row_valid; const int* pos; const float* y_in; long ldyi; float* y; long ldy;
  int N, T, d, E; float eps;
};

// One block per sequence, 1024 threads.  Phase 1: cache writes, the 2t+E+1 dot products (one per 16-lane group,
// 32 in flight per block, float4 loads), the normalised forward / backward weights, and the coefficients of
// the re-associated sum → LDS.  Phase 2 (two threads per channel): the sums over the cached value, condition and
// bias rows — (3·(t+1) + E) / 2 independent, coalesced loads per thread.
#ifndef ODIC_DYN_NT
#define ODIC_DYN_NT 1024
#endif
constexpr int DYN_NT = ODIC_DYN_NT;         // threads per sequence: the step is a chain of dependent load rounds, so the
                                     // block is as wide as it can be (64 dot-product groups, 2 x 512 channel threads)
__global__ __launch_bounds__(DYN_NT) void dynexp_step_kernel(DynParams p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  constexpr int NTD = DYN_NT;
  const int d = p.d, E = p.E, T = p.T, n = blockIdx.x, tid = threadIdx.x;
  const int t = *p.pos;
  if (t < 0 || t >= T) return;         // the caches hold T positions: a step replayed past the last one changes nothing
  float* cond_t = sm;                  // [d]
  float* key_t = cond_t + d;           // [d]
  float* dk = key_t + d;               // [T]  cond_t·key_j
  float* ck = dk + T;                  // [T]  cond_j·key_t
  float* qk_t = ck + T;                // [MAX_E]  qexp[e]·key_t
  float* nfw = qk_t + MAX_E;           // [2*MAX_E] 1/(Σ_j relu(±z_fw[e][·]) + eps)
  float* red = nfw + 2 * MAX_E;        // [16]
  int* slot = (int*)(red + 16);        // [T]
  float* qkh = (float*)(slot + T);     // [T*E]  qexp[e]·key_j history
  float* wba = qkh + T * E;            // [T*E]  backward weights of this step
  float* wbb = wba + T * E;            // [T*E]
  float* scr = wbb + T * E;            // ca[T] | cb[T] | wja[T] | wjb[T] | wea[E] | web[E]
  float* comb = scr + 4 * T + 2 * E;   // [NTD]  second half's partial sums of phase 2

  const float* lin = p.lin + (long)n * p.ldlin;
  const float inv_sqrt_d = rsqrtf((float)d);
  const long NT = (long)p.N;
  const int TE = T * E;

  for (int c = tid; c < d; c += NTD) {
    const float cv = lin[c], kv = lin[d + c];
    cond_t[c] = cv; key_t[c] = kv;
    const long o = ((long)t * NT + n) * d + c;
    p.cond_c[o] = cv; p.key_c[o] = kv; p.va_c[o] = lin[2 * d + c]; p.vb_c[o] = lin[3 * d + c];
  }
  for (int j = tid; j <= t; j += NTD) {
    const int sl = j < t ? p.anc[(long)n * T + j] : n;
    slot[j] = sl;
  }
  __syncthreads();
  for (int i = tid; i < t * E; i += NTD) {
    const int j = i / E, e = i - j * E;
    qkh[i] = p.qk_c[((long)j * NT + slot[j]) * E + e];
  }

  // dot products, one per 16-lane group (64 groups):
  //   items 0..E-1: qk_t[e];  E..E+t: dk[j] (j = 0..t);  E+t+1 .. E+2t: ck[j] (j = 0..t-1)
  const int nitems = E + (t + 1) + t;
  const int grp = tid >> 4, gl = tid & 15;
  for (int it = grp; it < nitems; it += NTD / 16) {
    const float* a; const float* b;
    if (it < E) { a = p.qexp + (long)it * d; b = key_t; }
    else if (it < E + t + 1) {
      const int j = it - E;
      a = cond_t; b = j < t ? p.key_c + ((long)j * NT + slot[j]) * d : key_t;
    } else {
      const int j = it - E - t - 1;
      a = p.cond_c + ((long)j * NT + slot[j]) * d; b = key_t;
    }
    float s = 0.f;
#pragma unroll 8
    for (int c = gl * 4; c < d; c += 64) {
      const float4 av = *(const float4*)(a + c);
      const float4 bv = *(const float4*)(b + c);
      s = fmaf(av.x, bv.x, s); s = fmaf(av.y, bv.y, s); s = fmaf(av.z, bv.z, s); s = fmaf(av.w, bv.w, s);
    }
    s += __shfl_xor(s, 8, 64); s += __shfl_xor(s, 4, 64); s += __shfl_xor(s, 2, 64); s += __shfl_xor(s, 1, 64);
    if (gl == 0) {
      if (it < E) { qk_t[it] = s; p.qk_c[((long)t * NT + n) * E + it] = s; }
      else if (it < E + t + 1) dk[it - E] = s;
      else ck[it - E - t - 1] = s;
    }
  }
  __syncthreads();
  if (tid == 0) ck[t] = dk[t];           // cond_t·key_t
  __syncthreads();

  // forward normalisers: 32 lanes per expansion query (E <= 32 → all of them in one pass), fixed shuffle order
  {
    const int e = tid >> 5, q = tid & 31;
    if (e < E) {
      float sp = 0.f, sn = 0.f;
      for (int j = q; j <= t; j += 32) {
        const float qq = j < t ? qkh[j * E + e] : qk_t[e];
        const float z = (qq + dk[j]) * inv_sqrt_d;
        sp += fmaxf(z, 0.f); sn += fmaxf(-z, 0.f);
      }
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) { sp += __shfl_xor(sp, o, 64); sn += __shfl_xor(sn, o, 64); }
      if (q == 0) { nfw[e] = 1.0f / (sp + p.eps); nfw[MAX_E + e] = 1.0f / (sn + p.eps); }
    }
  }
  float bp = 0.f, bn = 0.f;
  for (int i = tid; i < (t + 1) * E; i += NTD) {
    const int j = i / E, e = i - j * E;
    const float z = (qk_t[e] + ck[j]) * inv_sqrt_d;
    bp += fmaxf(z, 0.f); bn += fmaxf(-z, 0.f);
  }
  const float ibp = 1.0f / (block_sum(bp, red) + p.eps);
  const float ibn = 1.0f / (block_sum(bn, red) + p.eps);
  __syncthreads();
  // forward weights of THIS position → cache rows [t][n][i*E + e] (read by every later step of its descendants);
  // backward weights of this step → LDS
  float* wfa_t = p.wfa_c + ((long)t * NT + n) * TE;
  float* wfb_t = p.wfb_c + ((long)t * NT + n) * TE;
  for (int i = tid; i < (t + 1) * E; i += NTD) {
    const int j = i / E, e = i - j * E;
    const float q = j < t ? qkh[i] : qk_t[e];
    const float zf = (q + dk[j]) * inv_sqrt_d;
    const float zb = (qk_t[e] + ck[j]) * inv_sqrt_d;
    wfa_t[i] = fmaxf(zf, 0.f) * nfw[e];
    wfb_t[i] = fmaxf(-zf, 0.f) * nfw[MAX_E + e];
    wba[i] = fmaxf(zb, 0.f) * ibp;
    wbb[i] = fmaxf(-zb, 0.f) * ibn;
  }
  __syncthreads();                        // (also orders the block's own wfa_t / wfb_t stores before the reads below)
  // coefficients ca[i] = Σ_{j>=i} Σ_e wba[j][e]·wfa_j[i][e] (and cb): LP lanes per key position i (as many as the
  // block has for t+1 keys, 4..32), lane q takes j = i+q, i+q+LP, ...; fixed shuffle order → bit-identical run to run
  {
    int LP = 4;
    while (LP < 32 && (t + 1) * LP * 2 <= NTD) LP *= 2;
    const int i = tid / LP, q = tid - i * LP;
    if (i <= t) {
      float sa = 0.f, sb = 0.f;
      for (int j = i + q; j <= t; j += LP) {
        const long row = ((long)j * NT + slot[j]) * TE + (long)i * E;
        const float* fa = p.wfa_c + row;
        const float* fb = p.wfb_c + row;
        const float* ba = wba + j * E;
        const float* bb = wbb + j * E;
        for (int e = 0; e < E; e += 4) {
          const float4 x = *(const float4*)(fa + e), y = *(const float4*)(fb + e);
          sa = fmaf(ba[e], x.x, sa); sa = fmaf(ba[e + 1], x.y, sa); sa = fmaf(ba[e + 2], x.z, sa); sa = fmaf(ba[e + 3], x.w, sa);
          sb = fmaf(bb[e], y.x, sb); sb = fmaf(bb[e + 1], y.y, sb); sb = fmaf(bb[e + 2], y.z, sb); sb = fmaf(bb[e + 3], y.w, sb);
        }
      }
      for (int o = 1; o < LP; o <<= 1) { sa += __shfl_xor(sa, o, 64); sb += __shfl_xor(sb, o, 64); }
      if (q == 0) { scr[i] = sa; scr[T + i] = sb; }
    }
  }
  for (int j = tid; j <= t; j += NTD) {           // wja[j] = Σ_e wba[j][e]
    float sa = 0.f, sb = 0.f;
    for (int e = 0; e < E; ++e) { sa += wba[j * E + e]; sb += wbb[j * E + e]; }
    scr[2 * T + j] = sa; scr[3 * T + j] = sb;
  }
  {                                               // wea[e] = Σ_j wba[j][e]: 32 lanes per e
    const int e = tid >> 5, q = tid & 31;
    if (e < E) {
      float sa = 0.f, sb = 0.f;
      for (int j = q; j <= t; j += 32) { sa += wba[j * E + e]; sb += wbb[j * E + e]; }
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) { sa += __shfl_xor(sa, o, 64); sb += __shfl_xor(sb, o, 64); }
      if (q == 0) { scr[4 * T + e] = sa; scr[4 * T + E + e] = sb; }
    }
  }
  __syncthreads();

  // ---- phase 2: thread (half h, channel c): half 0 sums the earlier positions and the first E/2 bias rows, half 1
  //      the later ones; half 1's partial sums pass through LDS
  const float* ca = scr; const float* cb = scr + T;
  const float* wja = scr + 2 * T; const float* wjb = scr + 3 * T;
  const float* wea = scr + 4 * T; const float* web = wea + E;
  const bool valid = p.row_valid[n] != 0;
  constexpr int HALF = NTD / 2;
  const int h = tid / HALF, cl = tid - h * HALF;
  const int jm = (t + 1) / 2;
  const int j0 = h ? jm : 0, j1 = h ? t : jm;       // positions [j0, j1) from the caches; half 1 also takes position t
  const int e0 = h ? E / 2 : 0, e1 = h ? E : E / 2;
  for (int cb0 = 0; cb0 < d; cb0 += HALF) {
    const int c = cb0 + cl;
    float oa = 0.f, ob = 0.f;
    if (c < d) {
#pragma unroll 8
      for (int j = j0; j < j1; ++j) {
        const long o = ((long)j * NT + slot[j]) * d + c;
        const float va = p.va_c[o], vb = p.vb_c[o], cj = p.cond_c[o];
        oa = fmaf(ca[j], va, oa); oa = fmaf(wja[j], cj, oa);
        ob = fmaf(cb[j], vb, ob); ob = fmaf(wjb[j], cj, ob);
      }
      if (h) {
        oa = fmaf(ca[t], lin[2 * d + c], oa); oa = fmaf(wja[t], cond_t[c], oa);
        ob = fmaf(cb[t], lin[3 * d + c], ob); ob = fmaf(wjb[t], cond_t[c], ob);
      }
#pragma unroll 4
      for (int e = e0; e < e1; ++e) {
        const float be = p.bexp[(long)e * d + c];
        oa = fmaf(wea[e], be, oa);
        ob = fmaf(web[e], be, ob);
      }
    }
    if (h) { comb[cl] = oa; comb[HALF + cl] = ob; }
    __syncthreads();
    if (!h && c < d) {
      oa += comb[cl]; ob += comb[HALF + cl];
      float yv = p.y_in[(long)n * p.ldyi + c];
      if (valid) {
        const float sg = 1.0f / (1.0f + expf(-lin[4 * d + c]));
        yv += sg * oa + (1.0f - sg) * ob;
      }
      p.y[(long)n * p.ldy + c] = yv;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
// Cross attention: one block (4 waves) per (image, head, chunk of NB beams).  The k beams of an image
// attend to the SAME K/V, so every K/V element is loaded once per block and used for all NB queries
// (the one-wave-per-sequence form re-read 72 KB per beam and ran ~27 dependent load rounds):
//   scores : dk/16 lanes per key (16 floats each); the 4 waves sweep 4·64/(dk/16) keys at a time, all
//            sweeps of a wave in flight together; xor-shuffle reduce; NB dot products per loaded key
//   softmax: wave b normalises beam b (lanes stride over S), base e as the reference
//   P·V    : thread = (channel of the head, key group); coalesced dk·4-byte rows, 12 keys in flight,
//            NB accumulators; key groups combined through LDS.
// kv: [n_img, S, ldkv], K at koff, V at voff.
// ---------------------------------------------------------------------------------------------
template <int NB>
__global__ __launch_bounds__(256) void cross_attn_step_kernel(const float* __restrict__ q, long ldq,
                                                              const float* __restrict__ kv, long ldkv, int koff,
                                                              int voff, const int* __restrict__ enc_len,
                                                              const int* __restrict__ row_valid,
                                                              float* __restrict__ out, long ldo, int beams, int S,
                                                              int d, int heads) {
  extern __shared__ float smem[];        // sc[NB][S] | red[256 / dk][NB][dk] | lsum[NB]
  const int img = blockIdx.x, h = blockIdx.y, b0 = blockIdx.z * NB;
  const int nb = min(NB, beams - b0);    // beams handled here
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int dk = d / heads;
  const int lpk = dk >> 4;               // lanes per key (1, 2 or 4)
  const int kps = 64 / lpk;              // keys per wave-sweep
  const int len = enc_len[img];
  const float inv = rsqrtf((float)dk);
  const float* kvb = kv + (long)img * S * ldkv;
  const int part = lane % lpk, kslot = lane / lpk;
  float* sc = smem;
  float* red = smem + NB * S;
  float* lsum = red + 256 * NB;
  const long n0 = (long)img * beams + b0;   // first sequence row of this block

  float4 qv[NB][4];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const float* qp = q + (n0 + min(b, nb - 1)) * ldq + h * dk + part * 16;
#pragma unroll
    for (int i = 0; i < 4; ++i) qv[b][i] = *(const float4*)(qp + 4 * i);
  }
  int valid[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) valid[b] = row_valid[n0 + min(b, nb - 1)];

  // ---- scores: wave w takes sweeps w, w+4, ...; up to 3 sweeps of K loads in flight
  const int nsweep = (S + kps - 1) / kps;
  for (int sw0 = wave; sw0 < nsweep; sw0 += 12) {
    float4 k4[3][4];
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      const int s = min((sw0 + 4 * u) * kps + kslot, S - 1);
      const float* kr = kvb + (long)s * ldkv + koff + h * dk + part * 16;
#pragma unroll
      for (int i = 0; i < 4; ++i) k4[u][i] = *(const float4*)(kr + 4 * i);
    }
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      const int sw = sw0 + 4 * u;
      const int s = sw * kps + kslot;
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          acc = fmaf(qv[b][i].x, k4[u][i].x, acc); acc = fmaf(qv[b][i].y, k4[u][i].y, acc);
          acc = fmaf(qv[b][i].z, k4[u][i].z, acc); acc = fmaf(qv[b][i].w, k4[u][i].w, acc);
        }
        for (int o = 1; o < lpk; o <<= 1) acc += __shfl_xor(acc, o, 64);
        if (part == 0 && sw < nsweep && s < S) {
          float v = acc * inv;
          if (!valid[b] || s >= len) v = -1e4f;      // masked_fill(mask == 0, -1e4), layers.py:286
          sc[b * S + s] = v;
        }
      }
    }
  }
  __syncthreads();
  // ---- softmax: wave b → beam b, b + 4, ...
  for (int b = wave; b < nb; b += 4) {
    float m = -INFINITY;
    for (int s = lane; s < S; s += 64) m = fmaxf(m, sc[b * S + s]);
    m = wave_max(m);
    float l = 0.f;
    for (int s = lane; s < S; s += 64) { const float e = expf(sc[b * S + s] - m); sc[b * S + s] = e; l += e; }
    l = wave_sum(l);
    if (lane == 0) lsum[b] = l;
  }
  __syncthreads();
  // ---- P·V: thread = (channel c, key group g); groups take keys g, g + ng, ...
  const int c = tid % dk, g = tid / dk, ng = 256 / dk;
  float acc[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) acc[b] = 0.f;
  const float* vp = kvb + voff + h * dk + c;
  for (int s0 = g; s0 < S; s0 += 12 * ng) {
    float v[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) v[i] = vp[(long)min(s0 + i * ng, S - 1) * ldkv];
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      const int s = s0 + i * ng;
      if (s < S) {
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[b] = fmaf(sc[(b < nb ? b : 0) * S + s], v[i], acc[b]);
      }
    }
  }
#pragma unroll
  for (int b = 0; b < NB; ++b) red[(g * NB + b) * dk + c] = acc[b];
  __syncthreads();
  for (int e = tid; e < nb * dk; e += 256) {
    const int b = e / dk, cc = e - b * dk;
    float v = 0.f;
    for (int gg = 0; gg < ng; ++gg) v += red[(gg * NB + b) * dk + cc];
    out[(n0 + b) * ldo + h * dk + cc] = v / lsum[b];
  }
}

// ---------------------------------------------------------------------------------------------
// log-softmax + exact top-k (ties → lower index) of one row by one 512-thread block.  A thread holds a 20-value slice
// of the row in registers (V <= 10240; longer rows stream).  Selection by threshold instead of sorting:
//   1. wave maxima → LDS (their maximum is the row maximum the log-sum-exp needs anyway);
//   2. tau = the k-th largest of the 8 wave maxima: at least k elements are >= tau, so the k best all are;
//   3. in the Σexp pass every element >= tau (k .. a dozen of them) is appended to a candidate list in LDS;
//   4. wave 0 picks the k best of the candidates: k rounds of a wave arg-max over (value, lower index).
// That is ~60 VALU operations per thread and k+1 shuffle chains, against ~1000 for per-thread sorted lists.  A row
// whose candidate list would overflow (k > 8 wave maxima, or hundreds of equal values) takes block_ranked_topk
// (row_select.h) over a streaming scan instead — exact, just slower.
// `top_val` / `top_idx` ([k]); logp (optional): the full log-prob row.
// ---------------------------------------------------------------------------------------------
constexpr int TOPK_CAP = 128;          // candidates (two per lane of the selecting wave)
struct TopkShared {
  float red[16]; float red2[16]; int cnt; float cv[TOPK_CAP]; int ci[TOPK_CAP];
  ArgmaxSlots<8> win;                    // (512 threads)
};

template <int NTH, bool NORM>
__device__ __forceinline__ void row_logsoftmax_topk(const float* __restrict__ x, float* __restrict__ logp,
                                                    float* top_val, int* top_idx, int V, int k, TopkShared& sh) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int NPT = 10240 / NTH, NWV = NTH / 64;
  static_assert(NWV == 8, "TopkShared::win");
  const bool small = V <= NPT * NTH;
  float xv[NPT];
  float tm = -INFINITY;
  if (small) {                                       // all loads are in flight before the first use
#pragma unroll
    for (int u = 0; u < NPT; ++u) { const int i = tid + u * NTH; xv[u] = i < V ? x[i] : -INFINITY; }
  }
  if (small) {
#pragma unroll
    for (int u = 0; u < NPT; ++u) tm = fmaxf(tm, xv[u]);
  } else {
    for (int i = tid; i < V; i += NTH) tm = fmaxf(tm, x[i]);
  }
  tm = wave_max(tm);
  if (lane == 0) sh.red[wave] = tm;
  if (tid == 0) sh.cnt = 0;
  __syncthreads();
  float wm[NWV];
#pragma unroll
  for (int i = 0; i < NWV; ++i) wm[i] = sh.red[i];
  float mx = wm[0];
#pragma unroll
  for (int i = 1; i < NWV; ++i) mx = fmaxf(mx, wm[i]);
  float tau = -INFINITY;                             // k > NWV: every element is a candidate → the overflow path
  if (k <= NWV) {
#pragma unroll
    for (int i = 0; i < NWV; ++i) {                  // the element with exactly k-1 others ranked above it
      int above = 0;
#pragma unroll
      for (int j = 0; j < NWV; ++j) above += ranks_before(wm[j], j, wm[i], i) ? 1 : 0;
      if (above == k - 1) tau = wm[i];
    }
  }
  // Σ exp(x - max) and the candidates
  float sacc = 0.f;
  if (small) {
#pragma unroll
    for (int u = 0; u < NPT; ++u) {
      const float v = xv[u];
      if constexpr (NORM) sacc += expf(v - mx);
      if (v >= tau && tid + u * NTH < V) {
        const int pos = atomicAdd(&sh.cnt, 1);
        if (pos < TOPK_CAP) { sh.cv[pos] = v; sh.ci[pos] = tid + u * NTH; }
      }
    }
  } else {
    for (int i = tid; i < V; i += NTH) {
      const float v = x[i];
      if constexpr (NORM) sacc += expf(v - mx);
      if (v >= tau) {
        const int pos = atomicAdd(&sh.cnt, 1);
        if (pos < TOPK_CAP) { sh.cv[pos] = v; sh.ci[pos] = i; }
      }
    }
  }
  const float sm = wave_sum(sacc);
  if (lane == 0) sh.red2[wave] = sm;
  __syncthreads();
  float lse = 0.f;                                   // NORM = false: the row holds log-probs already
  if constexpr (NORM) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < NWV; ++i) t += sh.red2[i];
    lse = mx + logf(t);
  }
  if (logp)
    for (int i = tid; i < V; i += NTH) logp[i] = x[i] - lse;
  // selection: wave 0
  if (wave == 0) {
    const int n = sh.cnt;
    if (n <= TOPK_CAP) {
      float c0 = -INFINITY, c1 = -INFINITY; int i0 = 0x7fffffff, i1 = 0x7fffffff;
      if (lane < n) { c0 = sh.cv[lane]; i0 = sh.ci[lane]; }
      if (lane + 64 < n) { c1 = sh.cv[lane + 64]; i1 = sh.ci[lane + 64]; }
      for (int rd = 0; rd < k; ++rd) {
        const bool first = ranks_before(c0, i0, c1, i1);
        float best = first ? c0 : c1; int besti = first ? i0 : i1;
        wave_argmax(best, besti);
        if (lane == 0) { top_val[rd] = best - lse; top_idx[rd] = besti; }
        if (i0 == besti) { c0 = -INFINITY; i0 = 0x7fffffff; }
        if (i1 == besti) { c1 = -INFINITY; i1 = 0x7fffffff; }
      }
    }
  }
  // overflowed row (block-uniform)
  if (sh.cnt > TOPK_CAP) {
    block_ranked_topk<NTH>([&](float pv, int pi, float& best, int& besti) {
      for (int i = tid; i < V; i += NTH) {
        const float v = x[i];
        const bool after = ranks_after(v, i, pv, pi), before = ranks_before(v, i, best, besti);
        if (after & before) { best = v; besti = i; }
      }
    }, k, lse, top_val, top_idx, sh.win);
  }
}

template <bool NORM = true>
__global__ __launch_bounds__(512) void logsoftmax_topk_kernel(const float* __restrict__ logits, long ldl,
                                                              float* __restrict__ logp_out, long ldp,
                                                              float* __restrict__ top_val, int* __restrict__ top_idx,
                                                              int V, int k) {
  __shared__ TopkShared sh;
  const int n = blockIdx.x;
  row_logsoftmax_topk<512, NORM>(logits + (long)n * ldl, logp_out ? logp_out + (long)n * ldp : nullptr,
                                 top_val + (long)n * k, top_idx + (long)n * k, V, k, sh);
}


// ---------------------------------------------------------------------------------------------
// Sampling without replacement from softmax(x) — the `sample` branches of the reference search
// (captioning_model.py:128-131,166-168: exp(log_probs).multinomial(k, replacement=False)) and the ancestral
// sampling of :59-109 (k = 1) — as ONE pass over the row: the k largest of  x[v] + Gumbel(v)  are distributed
// exactly as k sequential draws without replacement (Gumbel-top-k / Plackett-Luce), so no renormalisation loop
// and no host round trip.  Noise: Philox4x32-10 keyed by `seed`, counter = (row, vocabulary index / 4, *pos, 0)
// → reproducible for a given seed whatever the launch geometry; the position read from device memory makes a
// captured step graph draw fresh numbers at every replay.  Outputs: the chosen words in draw order (descending
// perturbed score) and their log-probabilities x[v] − logsumexp(x); optionally the full log-prob row, and optionally
// (top_pert, odic_logsoftmax_sample_scored) the perturbed scores themselves, x[v] + Gumbel(v) − logsumexp(x).
// ---------------------------------------------------------------------------------------------
template <int KM>
__global__ __launch_bounds__(1024) void logsoftmax_sample_kernel(const float* __restrict__ logits, long ldl,
                                                                 float* __restrict__ logp_out, long ldp,
                                                                 float* __restrict__ top_val, int* __restrict__ top_idx,
                                                                 float* __restrict__ top_pert, int V, int k,
                                                                 unsigned long long seed, const int* __restrict__ pos) {
  __shared__ float red[16];
  __shared__ ArgmaxSlots<16> win;
  const int n = blockIdx.x, tid = threadIdx.x;
  const float* x = logits + (long)n * ldl;
  const unsigned step = pos ? (unsigned)*pos : 0u;
  DrawList<KM> l;
  l.clear();
  float mx = -INFINITY;
  // a thread owns groups of 4 consecutive words: one Philox call per group
  for (int g4 = tid; g4 * 4 < V; g4 += 1024) {
    unsigned r[4];
    philox4x32_10((unsigned)n, (unsigned)g4, step, 0u, (unsigned)seed, (unsigned)(seed >> 32), r);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int vi = g4 * 4 + e;
      if (vi < V) {
        const float xv = x[vi];
        mx = fmaxf(mx, xv);
        l.offer(xv + gumbel_from_bits(r[e]), vi);
      }
    }
  }
  const float m = block_max(mx, red);
  float s = 0.f;
  for (int i = tid; i < V; i += 1024) s += expf(x[i] - m);
  s = block_sum(s, red);
  const float lse = m + logf(s);
  if (logp_out)
    for (int i = tid; i < V; i += 1024) logp_out[(long)n * ldp + i] = x[i] - lse;
  block_draw_rounds<KM>(l, x, V, k, lse, top_val + (long)n * k, top_idx + (long)n * k,
                        top_pert ? top_pert + (long)n * k : nullptr, win);
}

// ---------------------------------------------------------------------------------------------
// Beam bookkeeping: one block per image (captioning_model.py:172-223).  Wave 0 does the k·k selection — one lane per
// candidate (four at k = 16), k rounds of wave_extract_best (below) in which the lowest flat index wins a tie (the scan
// order of the reference's topk over the flattened k x k scores) — then all threads permute the prefix / log-prob /
// ancestor rows IN PLACE (a thread owns whole columns j: it reads the k parent values of its column first, then
// writes the k new rows) and, when asked to, write the embedding of the chosen words for the next position
// (EmbeddingLayer, layers.py:118-121: what odic_dec_embed would do in its own launch).  The block that arrives last
// at `ctr` (low 16 bits = arrivals, high bits = images with a still-growing beam) advances *pos, raises *done when
// nothing grows any more, and re-arms the counter.  The state, the rows in LDS, wave_extract_best and the update half
// (beam_apply) live in beam_step.h, which stochastic_beam.hip shares.
// ---------------------------------------------------------------------------------------------
// the k best of the k x k candidates.  Key: the flat candidate index beam·k + rank (the scan order of the reference's
// topk over the flattened scores; drawn candidates are not sorted by word, and a finished row's rule is positional).
// A total of -inf is never ranked (a dead row, cumul = -inf; a candidate of value -inf; a NaN total compares false and
// goes the same way).  A slot for which no total above -inf is left (not found) becomes the EMPTY row of
// require_beam_select: parent = the slot itself, word = EOS, stored log-prob -inf.  A found key is a flat index that was
// put in below, so every index formed from a selection lies in [0, k) (s.parent) and [0, k·k) (s.ci), whatever the
// candidate values are.
__device__ __forceinline__ void beam_select(const BeamParams& p, BeamShared& s, int t) {
  if (threadIdx.x >= 64) return;
  const int lane = threadIdx.x, k = p.k;
  if (t == 0) {                         // seeding: the k best words of beam 0
    if (lane < k) { s.parent[lane] = 0; s.word[lane] = s.ci[lane]; s.lp[lane] = s.cv[lane]; }
    return;
  }
  float tot[BEAM_CPL], val[BEAM_CPL]; int key[BEAM_CPL];
#pragma unroll
  for (int u = 0; u < BEAM_CPL; ++u) {
    const int i = lane + 64 * u;
    tot[u] = -INFINITY; val[u] = 0.f; key[u] = NO_KEY<int>;
    if (i < k * k) {
      const int j = i / k, c = i - j * k;
      val[u] = s.eos[j] ? (c == 0 ? 0.0f : -999.0f) : s.cv[i];
      tot[u] = s.cu[j] + val[u];
      key[u] = i;
    }
  }
  for (int r = 0; r < k; ++r) {
    int bi; float bval;
    const bool found = wave_extract_best(tot, key, val, bi, bval);
    if (lane == 0) {
      if (found) { s.parent[r] = bi / k; s.word[r] = s.ci[bi]; s.lp[r] = bval; }
      else { s.parent[r] = r; s.word[r] = (int)p.eos; s.lp[r] = -INFINITY; }
    }
  }
}

__global__ __launch_bounds__(256) void beam_step_kernel(BeamParams p, EmbedArgs e) {
  __shared__ BeamShared s;
  const int b = blockIdx.x;
  const int t = *p.pos;                 // position just processed; prefix length is t+1
  if (t + 1 >= p.T) return;             // the prefix is full: a replay past the last step changes nothing
  beam_load_rows(p, s, b, t);
  beam_select(p, s, t);
  beam_apply(p, e, s, b, t);             // (four waves: the k·d embedding rows and the prefix re-gather are the bulk)
}

// ---------------------------------------------------------------------------------------------
// Diverse (group) beam search step: the R = G·kg rows of an image are G groups of kg beams, rows g·kg .. g·kg+kg-1 being
// group g.  Wave 0 walks the groups in order.  Group g ranks its kg·R candidates (beam j of the group x its R best
// words; four per lane at most) by   total = cumul_j + (logp_j(w) - penalty·count[w])   where count[w] is the number
// of picks of groups 0..g-1 at this step that appended w to a beam still growing; a finished beam keeps the rule of
// beam_select (rank 0 worth 0, the others -999, never penalised).  wave_extract_best with the key (beam in group, word)
// — unique within a group, a row's k words being distinct; at G = 1 (count = 0, a row's candidates sorted by value, then
// word) the order of beam_select's flat index — and the candidate's own, unpenalised value as the payload: that is what
// is stored (s.lp).  The three operations are rounded separately (__fmul_rn, __fsub_rn, __fadd_rn; the products go
// through a small LDS table so that nothing can be contracted), so that a float32 host model reproduces the order bit
// for bit.  The picks made so far ARE the penalty list: s.word[q] and grow[q] for q < g·kg (at most 15 entries), read
// back by the next group after a fence.  Seeding (t = 0): every row holds the same distribution; group g draws from its
// first row, against the seeds of the groups before it.
// A finished beam's candidates carry their rank in place of the word in the key (its -999 fillers tie, and beam_select
// takes them by flat index; lane 0 reads the word back from s.ci).  A slot for which no total above -inf is left becomes
// the EMPTY row of beam_select (parent = the slot's own row, word = EOS, stored log-prob -inf, grow = 0: never counted
// by a later group), so a group never holds one live caption twice.
// R candidates per row are enough: the penalised top-kg of a row lies inside its unpenalised top-(kg + P), P <= g·kg <=
// R - kg the number of penalised words.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void group_beam_select(const BeamParams& p, BeamShared& s, int* grow, const float* pen,
                                                  int t, int G, int kg) {
  if (threadIdx.x >= 64) return;
  const int lane = threadIdx.x, R = p.k;
  const int nc = (t == 0 ? 1 : kg) * R;                // candidates of a group (kg·R <= 256)
  for (int g = 0; g < G; ++g) {
    const int row0 = g * kg;                           // first row of the group = number of earlier picks
    float tot[BEAM_CPL], val[BEAM_CPL]; long long key[BEAM_CPL];
#pragma unroll
    for (int u = 0; u < BEAM_CPL; ++u) {
      const int i = lane + 64 * u;
      tot[u] = -INFINITY; val[u] = 0.f; key[u] = NO_KEY<long long>;
      if (i < nc) {
        const int j = i / R, c = i - j * R, row = row0 + j, fl = row * R + c;
        const int w = s.ci[fl];
        int low = w;
        float v;
        if (t > 0 && s.eos[row]) {
          v = val[u] = c == 0 ? 0.0f : -999.0f;
          low = c;                                       // the -999 fillers of a row tie: by rank, as in beam_select
        } else {
          int cnt = 0;
          for (int q = 0; q < row0; ++q) cnt += (grow[q] && s.word[q] == w) ? 1 : 0;
          val[u] = s.cv[fl];
          v = __fsub_rn(val[u], pen[cnt]);
        }
        tot[u] = t == 0 ? v : __fadd_rn(s.cu[row], v);
        key[u] = ((long long)j << 32) | (long long)(unsigned)low;
      }
    }
    for (int r = 0; r < kg; ++r) {
      long long bk; float bval;
      const bool found = wave_extract_best(tot, key, val, bk, bval);
      if (lane == 0) {
        const int q = row0 + r;
        if (found) {                                     // (a found key was put in above: row in the group, low < 2^31)
          const int row = row0 + (int)(bk >> 32), low = (int)(bk & 0xffffffffLL);
          const int fin = t > 0 && s.eos[row];
          s.parent[q] = row; s.word[q] = fin ? s.ci[row * R + low] : low; s.lp[q] = bval; grow[q] = fin ? 0 : 1;
        } else {                                         // no total above -inf is left: the EMPTY row of beam_select
          s.parent[q] = q; s.word[q] = (int)p.eos; s.lp[q] = -INFINITY; grow[q] = 0;
        }
      }
    }
    // lane 0's picks are read by every lane of this wave in the next group
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
}

__global__ __launch_bounds__(256) void group_beam_step_kernel(BeamParams p, EmbedArgs e, int G, int kg, float penalty) {
  __shared__ BeamShared s;
  __shared__ int grow[MAX_K];           // pick q of this step extends a beam that was still growing
  __shared__ float pen[MAX_K];          // penalty·count for count = 0 .. 15 (at most R - kg earlier picks)
  const int b = blockIdx.x;
  const int t = *p.pos;
  if (t + 1 >= p.T) return;
  // the product is rounded on its own here and only read back below: the build contracts a·b - c into one fma otherwise
  if (threadIdx.x < MAX_K) pen[threadIdx.x] = __fmul_rn(penalty, (float)threadIdx.x);
  beam_load_rows(p, s, b, t);
  group_beam_select(p, s, grow, pen, t, G, kg);
  beam_apply(p, e, s, b, t);
}

// ---------------------------------------------------------------------------------------------
// Required words (lexically constrained beam search): an image has C <= 4 required word ids (-1 = unused
// slot), and its R = 2^C·kb rows are 2^C banks of kb rows, bank m (a bit mask over the slots) being rows m·kb .. m·kb+kb-1:
// a row lives in bank m when its caption holds exactly the required words whose bits are set in m.  Wave 0 walks the
// target banks in order.  Bank m ranks kb·(R + C) candidates, four per lane at most:
//   stay   row j of bank m x its R best words, without the required words whose bit is clear in m (they lead elsewhere)
//          and without EOS unless m is the accepting bank (every used slot set); a finished row keeps the rule of
//          beam_select's rank 0 (worth 0) and offers nothing else;
//   enter  for every slot c set in m, row j of bank m ^ (1 << c) x the word required[c], at the value gathered from the
//          row's log-probs (rlp) — the word need not be among the row's R best.
// Only rows with cumul > -inf offer anything (t = 0: row 0 alone, total = v).  wave_extract_best with the key (source
// row, word), unique within a target bank, and the candidate's value as the payload.  A slot for which no finite total
// is left (not found) becomes an EMPTY row: parent = the slot itself (row 0 at t = 0), word = EOS, stored log-prob -inf —
// beam_apply then leaves it with cumul = -inf and has_eos = 1, and it never offers anything again.
// The banks read only the state of before the step, so nothing is handed from one bank to the next (no fence as between
// the groups of group_beam_select).  total is one __fadd_rn, as in the group kernel.
// ---------------------------------------------------------------------------------------------
constexpr int MAX_REQ = 4;
struct RequireArgs { const float* logp; long ldl; const long long* required; int C, kb, V; };

__device__ __forceinline__ void require_beam_select(const BeamParams& p, BeamShared& s, const int* req,
                                                    const float (*rlp)[MAX_REQ], int t, int C, int kb) {
  if (threadIdx.x >= 64) return;
  const int lane = threadIdx.x, R = p.k, eos = (int)p.eos;
  int accept = 0;
  for (int c = 0; c < C; ++c) accept |= req[c] >= 0 ? 1 << c : 0;
  const int n_stay = kb * R, nc = n_stay + C * kb;     // (kb·(R + C) <= 256)
  for (int m = 0; m < (1 << C); ++m) {
    float tot[BEAM_CPL], val[BEAM_CPL]; long long key[BEAM_CPL];
#pragma unroll
    for (int u = 0; u < BEAM_CPL; ++u) {
      const int i = lane + 64 * u;
      tot[u] = -INFINITY; val[u] = 0.f; key[u] = NO_KEY<long long>;
      if (i < nc) {
        int row, w; bool ok; float v = 0.f;
        if (i < n_stay) {
          const int j = i / R, c = i - j * R;
          row = m * kb + j;
          w = s.ci[row * R + c];
          if (t > 0 && s.eos[row]) {
            ok = c == 0;
          } else {
            v = s.cv[row * R + c];
            ok = !(w == eos && m != accept);
            for (int q = 0; q < C; ++q) ok = ok && !(w == req[q] && !((m >> q) & 1));
          }
        } else {
          const int en = i - n_stay, q = en / kb, j = en - q * kb;
          row = (m ^ (1 << q)) * kb + j;                 // (< R whatever the bit)
          w = req[q];
          ok = ((m >> q) & 1) && w >= 0 && !(t > 0 && s.eos[row]);
          if (ok) v = rlp[row][q];
        }
        ok = ok && (t == 0 ? row == 0 : s.cu[row] > -INFINITY);
        if (ok) {
          tot[u] = t == 0 ? v : __fadd_rn(s.cu[row], v);
          val[u] = v;
          key[u] = ((long long)row << 32) | (long long)(unsigned)w;
        }
      }
    }
    for (int r = 0; r < kb; ++r) {
      long long bk; float bval;
      const bool found = wave_extract_best(tot, key, val, bk, bval);
      if (lane == 0) {
        const int slot = m * kb + r;
        s.parent[slot] = found ? (int)(bk >> 32) : (t == 0 ? 0 : slot);
        s.word[slot] = found ? (int)(bk & 0xffffffffLL) : eos;
        s.lp[slot] = found ? bval : -INFINITY;
      }
    }
  }
}

__global__ __launch_bounds__(256) void require_beam_step_kernel(BeamParams p, EmbedArgs e, RequireArgs a) {
  __shared__ BeamShared s;
  __shared__ int req[MAX_REQ];          // the image's required ids; -1: unused slot, or an id outside the vocabulary
  __shared__ float rlp[MAX_K][MAX_REQ]; // log-prob of required word c in row r
  const int b = blockIdx.x, R = p.k, C = a.C;
  const int t = *p.pos;
  if (t + 1 >= p.T) return;
  for (int i = threadIdx.x; i < R * C; i += 256) {
    const int row = i / C, c = i - row * C;
    const long long w = a.required[(long)b * C + c];
    const bool used = w >= 0 && w < a.V;
    if (row == 0) req[c] = used ? (int)w : -1;
    rlp[row][c] = used ? a.logp[((long)b * R + row) * a.ldl + w] : -INFINITY;
  }
  beam_load_rows(p, s, b, t);
  require_beam_select(p, s, req, rlp, t, C, a.kb);
  beam_apply(p, e, s, b, t);
}

// score = cumul / n_elem of the k rows of image b, and their order: score descending, a tie (-inf against -inf included)
// to the lower row.  The rows already listed are remembered in a bit mask, their scores left alone, and every round takes
// the first row not yet listed unless a later one is strictly better: order is a permutation of 0..k-1 whatever the
// scores are (dead rows, score -inf, come last in row order).  Returns order[0].
__device__ __forceinline__ int beam_rank_rows(const float* cumul, const int* n_elem, int* order, float* score, int b,
                                              int k) {
  float sc[MAX_K];
  for (int j = 0; j < k; ++j) { sc[j] = cumul[b * k + j] / (float)n_elem[b * k + j]; score[b * k + j] = sc[j]; }
  unsigned taken = 0;
  int first = 0;
  for (int r = 0; r < k; ++r) {
    int bi = -1; float bv = 0.f;
    for (int j = 0; j < k; ++j)
      if (!((taken >> j) & 1u) && (bi < 0 || sc[j] > bv)) { bv = sc[j]; bi = j; }
    taken |= 1u << bi;
    order[b * k + r] = bi;
    if (r == 0) first = bi;
  }
  return first;
}

__global__ void beam_finalize_kernel(const float* cumul, const int* n_elem, int* order, float* score, int n_img,
                                     int k) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_img) return;
  beam_rank_rows(cumul, n_elem, order, score, b, k);
}

// odic_beam_finalize + emission of the best caption (EOS-padded int32 row + length): one 64-lane block per image
__global__ __launch_bounds__(64) void beam_finalize_best_kernel(const float* cumul, const int* n_elem,
                                                                const long long* tok, int* order, float* score,
                                                                int* out_tok, int* out_len, int k, int T, int pad) {
  __shared__ int s_best;
  const int b = blockIdx.x, lane = threadIdx.x;
  if (lane == 0) s_best = beam_rank_rows(cumul, n_elem, order, score, b, k);   // (row 0 when every row is dead)
  __syncthreads();
  const int best = s_best;
  const int len = n_elem[b * k + best];
  const long long* src = tok + ((long)b * k + best) * T;
  for (int j = lane; j < T; j += 64) out_tok[(long)b * T + j] = j < len ? (int)src[j] : pad;
  if (lane == 0) out_len[b] = len;
}

__global__ void beam_reset_kernel(long long* tok, float* lp, int* row_valid, long long* next_tok, int* pos,
                                  int* done, int* ctr, int N, int T, long long sos, EmbedArgs e) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) { tok[(long)i * T] = sos; lp[(long)i * T] = 0.f; row_valid[i] = 1; next_tok[i] = sos; }
  if (i == 0) { *pos = 0; *done = 0; *ctr = 0; }
  if (e.embed)                                          // input of position 0: the start token
    for (long q = i; q < (long)N * e.d; q += (long)gridDim.x * blockDim.x) {
      const long r = q / e.d; const int c = (int)(q - r * e.d);
      e.y[r * e.ldy + c] = e.embed[sos * e.d + c] * e.scale + e.pos_table[c];
    }
}

}  // namespace

extern "C" int odic_dec_embed(const int64_t* tokens, const float* embed, const float* pos_table,
                              const int32_t* pos, float* y, int64_t ldy, int32_t N, int32_t d, int32_t pos_rows,
                              float scale, void* stream) {
  if (!tokens || !embed || !pos_table || !pos || !y) return ODIC_ENULL;
  if (N <= 0 || d <= 0 || pos_rows <= 0) return ODIC_EINVAL;
  hipLaunchKernelGGL(dec_embed_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, (const long long*)tokens, embed,
                     pos_table, pos, y, (long)ldy, N, d, pos_rows, scale);
  return odic_launch_status();
}

extern "C" int odic_dynexp_step(const float* lin, int64_t ldlin, const float* qexp, const float* bexp,
                                float* cond_c, float* key_c, float* va_c, float* vb_c, float* wfa_c,
                                float* wfb_c, float* qk_c, const int32_t* anc, const int32_t* row_valid,
                                const int32_t* pos, const float* y_in, int64_t ldy_in, float* y, int64_t ldy,
                                int32_t N, int32_t T, int32_t d, int32_t E, float eps, void* stream) {
  if (!lin || !qexp || !bexp || !cond_c || !key_c || !va_c || !vb_c || !wfa_c || !wfb_c || !qk_c || !anc ||
      !row_valid || !pos || !y || !y_in)
    return ODIC_ENULL;
  if (N <= 0 || T <= 0 || T > MAX_T || d <= 0 || E <= 0 || E > MAX_E) return ODIC_EINVAL;
  if (E != 4 && E != 8 && E != 16 && E != 32) return ODIC_EUNSUPPORTED;
  if (d % 64) return ODIC_EINVAL;
  DynParams p;
  p.lin = lin; p.ldlin = ldlin; p.qexp = qexp; p.bexp = bexp; p.cond_c = cond_c; p.key_c = key_c; p.va_c = va_c;
  p.vb_c = vb_c; p.wfa_c = wfa_c; p.wfb_c = wfb_c; p.qk_c = qk_c; p.anc = anc; p.row_valid = row_valid;
  p.pos = pos; p.y_in = y_in; p.ldyi = ldy_in; p.y = y; p.ldy = ldy;
  p.N = N; p.T = T; p.d = d; p.E = E; p.eps = eps;
  const size_t shmem = (size_t)(2 * d + 2 * T + 3 * MAX_E + 16 + 3 * T * E + 4 * T + 2 * E + DYN_NT) * sizeof(float) +
                       (size_t)T * sizeof(int);
  if (shmem > 64 * 1024) return ODIC_EINVAL;
  hipLaunchKernelGGL(dynexp_step_kernel, dim3(N), dim3(DYN_NT), shmem, (hipStream_t)stream, p);
  return odic_launch_status();
}

extern "C" int odic_cross_attn_step(const float* q, int64_t ldq, const float* kv, int64_t ldkv, int32_t koff,
                                    int32_t voff, const int32_t* enc_len, const int32_t* row_valid, float* out,
                                    int64_t ldo, int32_t N, int32_t n_img, int32_t S, int32_t d, int32_t heads,
                                    void* stream) {
  if (!q || !kv || !enc_len || !row_valid || !out) return ODIC_ENULL;
  if (N <= 0 || n_img <= 0 || N % n_img || S <= 0 || d <= 0 || heads <= 0 || d % heads) return ODIC_EINVAL;
  const int dk = d / heads;
  if (dk != 16 && dk != 32 && dk != 64) return ODIC_EUNSUPPORTED;
  if ((ldq & 3) || (ldkv & 3) || (koff & 3) || ((uintptr_t)q & 15) || ((uintptr_t)kv & 15)) return ODIC_EINVAL;
  if (S > 2048) return ODIC_EINVAL;       // score rows of up to 5 beams live in LDS
  const int beams = N / n_img;
  hipStream_t st = (hipStream_t)stream;
#define ODIC_XATTN(NB)                                                                                              \
  hipLaunchKernelGGL(cross_attn_step_kernel<NB>, dim3(n_img, heads, (beams + NB - 1) / NB), dim3(256),              \
                     (size_t)(NB * S + 256 * NB + NB) * sizeof(float), st, q, (long)ldq, kv, (long)ldkv, koff, voff,  \
                     enc_len, row_valid, out, (long)ldo, beams, S, d, heads)
  if (heads > 65535) return ODIC_EINVAL;
  if (beams == 1) ODIC_XATTN(1);
  else if (beams == 2) ODIC_XATTN(2);
  else if (beams == 3) ODIC_XATTN(3);
  else if (beams == 5 || beams > 8) ODIC_XATTN(5);
  else ODIC_XATTN(4);
#undef ODIC_XATTN
  return odic_launch_status();
}

// Ensemble step distribution (ensemble_captioning_model.py:66-83): out[n][v] = log(mean_m softmax(logits_m[n])[v]).
// One block per row; per model the row max and Σexp, then one pass that averages the probabilities.
constexpr int MAX_MODELS = 8;
struct EnsembleParams { const float* logits[MAX_MODELS]; int M; long ldl; float* out; long ldo; int V; };

__global__ __launch_bounds__(1024) void ensemble_logprob_kernel(EnsembleParams p) {
  __shared__ float red[16];
  __shared__ float s_max[MAX_MODELS], s_inv[MAX_MODELS];
  const int n = blockIdx.x, tid = threadIdx.x;
  for (int m = 0; m < p.M; ++m) {
    const float* x = p.logits[m] + (long)n * p.ldl;
    float mx = -INFINITY;
    for (int i = tid; i < p.V; i += 1024) mx = fmaxf(mx, x[i]);
    mx = block_max(mx, red);
    float s = 0.f;
    for (int i = tid; i < p.V; i += 1024) s += expf(x[i] - mx);
    s = block_sum(s, red);
    if (tid == 0) { s_max[m] = mx; s_inv[m] = 1.0f / s; }
    __syncthreads();
  }
  const float inv_m = 1.0f / (float)p.M;
  for (int i = tid; i < p.V; i += 1024) {
    float acc = 0.f;
    for (int m = 0; m < p.M; ++m) acc += expf(p.logits[m][(long)n * p.ldl + i] - s_max[m]) * s_inv[m];
    p.out[(long)n * p.ldo + i] = logf(acc * inv_m);
  }
}

extern "C" int odic_ensemble_logprobs(const float* const* logits, int32_t M, int64_t ldl, float* out, int64_t ldo,
                                      int32_t N, int32_t V, void* stream) {
  if (!logits || !out) return ODIC_ENULL;
  if (M <= 0 || M > MAX_MODELS || N <= 0 || V <= 0) return ODIC_EINVAL;
  EnsembleParams p;
  for (int m = 0; m < MAX_MODELS; ++m) p.logits[m] = m < M ? logits[m] : nullptr;
  for (int m = 0; m < M; ++m) if (!p.logits[m]) return ODIC_ENULL;
  p.M = M; p.ldl = ldl; p.out = out; p.ldo = ldo; p.V = V;
  hipLaunchKernelGGL(ensemble_logprob_kernel, dim3(N), dim3(1024), 0, (hipStream_t)stream, p);
  return odic_launch_status();
}

extern "C" int odic_topk_rows(const float* logp, int64_t ldl, float* top_val, int32_t* top_idx, int32_t N, int32_t V,
                              int32_t k, void* stream) {
  if (!logp || !top_val || !top_idx) return ODIC_ENULL;
  if (N <= 0 || V <= 0 || k <= 0 || k > MAX_K || k > V) return ODIC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(logsoftmax_topk_kernel<false>, dim3(N), dim3(512), 0, s, logp, (long)ldl, (float*)nullptr, 0L, top_val, top_idx, V, k);
  return odic_launch_status();
}

extern "C" int odic_logsoftmax_topk(const float* logits, int64_t ldl, float* logp_out, int64_t ldp, float* top_val,
                                    int32_t* top_idx, int32_t N, int32_t V, int32_t k, void* stream) {
  if (!logits || !top_val || !top_idx) return ODIC_ENULL;
  if (N <= 0 || V <= 0 || k <= 0 || k > MAX_K || k > V) return ODIC_EINVAL;
  hipLaunchKernelGGL(logsoftmax_topk_kernel<true>, dim3(N), dim3(512), 0, (hipStream_t)stream, logits, (long)ldl, logp_out,
                     (long)ldp, top_val, top_idx, V, k);
  return odic_launch_status();
}

extern "C" int odic_beam_step(const float* cand_val, const int32_t* cand_idx, const odic_beam_state* st,
                              const odic_embed_args* emb, int32_t n_img, int32_t beams, int32_t T, int64_t eos_idx,
                              void* stream) {
  if (!cand_val || !cand_idx) return ODIC_ENULL;
  BeamParams p; EmbedArgs e;
  const int rc = beam_params(p, e, st, emb, n_img, beams, T, eos_idx);
  if (rc != 0) return rc;
  p.cand_val = cand_val; p.cand_idx = cand_idx;
  hipLaunchKernelGGL(beam_step_kernel, dim3(n_img), dim3(256), 0, (hipStream_t)stream, p, e);
  return odic_launch_status();
}

extern "C" int odic_group_beam_step(const float* cand_val, const int32_t* cand_idx, int32_t ncand,
                                    const odic_beam_state* st, const odic_embed_args* emb, int32_t n_img,
                                    int32_t groups, int32_t group_beams, int32_t T, int64_t eos_idx, float penalty,
                                    void* stream) {
  if (!cand_val || !cand_idx) return ODIC_ENULL;
  if (groups < 1 || group_beams < 1 || groups > MAX_K || group_beams > MAX_K) return ODIC_EINVAL;
  const int R = groups * group_beams;
  if (R > MAX_K || ncand != R) return ODIC_EINVAL;
  if (!(penalty >= 0.0f) || !(penalty <= 3.402823466e38f)) return ODIC_EINVAL;      // negative, infinite or NaN
  BeamParams p; EmbedArgs e;
  const int rc = beam_params(p, e, st, emb, n_img, R, T, eos_idx);
  if (rc != 0) return rc;
  p.cand_val = cand_val; p.cand_idx = cand_idx;
  hipLaunchKernelGGL(group_beam_step_kernel, dim3(n_img), dim3(256), 0, (hipStream_t)stream, p, e, (int)groups,
                     (int)group_beams, penalty);
  return odic_launch_status();
}

extern "C" int odic_require_beam_step(const float* cand_val, const int32_t* cand_idx, int32_t ncand, const float* logp,
                                      int64_t ldl, const int64_t* required, int32_t n_required,
                                      const odic_beam_state* st, const odic_embed_args* emb, int32_t n_img,
                                      int32_t bank_beams, int32_t T, int64_t eos_idx, int32_t V, void* stream) {
  if (!cand_val || !cand_idx) return ODIC_ENULL;
  if (n_required < 0 || n_required > MAX_REQ || bank_beams < 1 || bank_beams > MAX_K) return ODIC_EINVAL;
  const int R = bank_beams << n_required;
  if (R > MAX_K || ncand != R) return ODIC_EINVAL;
  if (n_required > 0 && R < bank_beams + n_required + 1) return ODIC_EINVAL;
  // eos: the word of an empty row, embedded like any other
  if (V < 1 || ldl < V || eos_idx < 0 || eos_idx >= V) return ODIC_EINVAL;
  if (n_required > 0 && (!logp || !required)) return ODIC_EINVAL;
  BeamParams p; EmbedArgs e;
  const int rc = beam_params(p, e, st, emb, n_img, R, T, eos_idx);
  if (rc != 0) return rc;
  p.cand_val = cand_val; p.cand_idx = cand_idx;
  RequireArgs a;
  a.logp = logp; a.ldl = (long)ldl; a.required = (const long long*)required; a.C = n_required; a.kb = bank_beams; a.V = V;
  hipLaunchKernelGGL(require_beam_step_kernel, dim3(n_img), dim3(256), 0, (hipStream_t)stream, p, e, a);
  return odic_launch_status();
}

extern "C" int odic_beam_finalize(const odic_beam_state* st, int32_t* order, float* score, int32_t n_img,
                                  int32_t beams, void* stream) {
  if (!st || !order || !score) return ODIC_ENULL;
  if (n_img <= 0 || beams <= 0 || beams > MAX_K) return ODIC_EINVAL;
  hipLaunchKernelGGL(beam_finalize_kernel, dim3((n_img + 63) / 64), dim3(64), 0, (hipStream_t)stream, st->cumul,
                     st->n_elem, order, score, n_img, beams);
  return odic_launch_status();
}

extern "C" int odic_beam_finalize_best(const odic_beam_state* st, int32_t* order, float* score, int32_t* out_tok,
                                       int32_t* out_len, int32_t n_img, int32_t beams, int32_t T, int32_t pad_idx,
                                       void* stream) {
  if (!st || !order || !score || !out_tok || !out_len) return ODIC_ENULL;
  if (!st->tokens || !st->cumul || !st->n_elem) return ODIC_ENULL;
  if (n_img <= 0 || beams <= 0 || beams > MAX_K || T <= 0) return ODIC_EINVAL;
  hipLaunchKernelGGL(beam_finalize_best_kernel, dim3(n_img), dim3(64), 0, (hipStream_t)stream, st->cumul, st->n_elem,
                     (const long long*)st->tokens, order, score, out_tok, out_len, beams, T, pad_idx);
  return odic_launch_status();
}

extern "C" int odic_beam_reset(const odic_beam_state* st, const odic_embed_args* emb, int32_t n_img, int32_t beams,
                               int32_t T, int64_t sos_idx, void* stream) {
  if (!st) return ODIC_ENULL;
  EmbedArgs e;
  const int rc = odic_embed_args_from(e, emb);
  if (rc != 0) return rc;
  if (!st->tokens || !st->logprobs || !st->row_valid || !st->next_tok || !st->pos || !st->done || !st->ctr)
    return ODIC_ENULL;
  if (n_img <= 0 || beams <= 0 || beams > MAX_K || T <= 0) return ODIC_EINVAL;
  const int N = n_img * beams;
  const int nblk = emb ? (int)(((long)N * e.d + 255) / 256 < 1024 ? ((long)N * e.d + 255) / 256 : 1024) : (N + 255) / 256;
  hipLaunchKernelGGL(beam_reset_kernel, dim3(nblk < (N + 255) / 256 ? (N + 255) / 256 : nblk), dim3(256), 0,
                     (hipStream_t)stream, (long long*)st->tokens, st->logprobs, st->row_valid,
                     (long long*)st->next_tok, st->pos, st->done, st->ctr, N, T, (long long)sos_idx, e);
  return odic_launch_status();
}

// the one launch behind odic_logsoftmax_sample (top_pert = nullptr) and odic_logsoftmax_sample_scored
static int launch_logsoftmax_sample(const float* logits, int64_t ldl, float* logp_out, int64_t ldp, float* top_val,
                                    int32_t* top_idx, float* top_pert, int32_t N, int32_t V, int32_t k, uint64_t seed,
                                    const int32_t* pos, void* stream) {
  if (!logits || !top_val || !top_idx) return ODIC_ENULL;
  if (N <= 0 || V <= 0 || k <= 0 || k > MAX_K || k > V) return ODIC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (k <= 4) hipLaunchKernelGGL(logsoftmax_sample_kernel<4>, dim3(N), dim3(1024), 0, s, logits, (long)ldl, logp_out, (long)ldp, top_val, top_idx, top_pert, V, k, (unsigned long long)seed, pos);
  else if (k <= 8) hipLaunchKernelGGL(logsoftmax_sample_kernel<8>, dim3(N), dim3(1024), 0, s, logits, (long)ldl, logp_out, (long)ldp, top_val, top_idx, top_pert, V, k, (unsigned long long)seed, pos);
  else hipLaunchKernelGGL(logsoftmax_sample_kernel<16>, dim3(N), dim3(1024), 0, s, logits, (long)ldl, logp_out, (long)ldp, top_val, top_idx, top_pert, V, k, (unsigned long long)seed, pos);
  return odic_launch_status();
}

extern "C" int odic_logsoftmax_sample(const float* logits, int64_t ldl, float* logp_out, int64_t ldp, float* top_val,
                                      int32_t* top_idx, int32_t N, int32_t V, int32_t k, uint64_t seed,
                                      const int32_t* pos, void* stream) {
  return launch_logsoftmax_sample(logits, ldl, logp_out, ldp, top_val, top_idx, nullptr, N, V, k, seed, pos, stream);
}

extern "C" int odic_logsoftmax_sample_scored(const float* logits, int64_t ldl, float* logp_out, int64_t ldp,
                                             float* top_val, int32_t* top_idx, float* top_pert, int32_t N, int32_t V,
                                             int32_t k, uint64_t seed, const int32_t* pos, void* stream) {
  if (!top_pert) return ODIC_ENULL;
  return launch_logsoftmax_sample(logits, ldl, logp_out, ldp, top_val, top_idx, top_pert, N, V, k, seed, pos, stream);
}
