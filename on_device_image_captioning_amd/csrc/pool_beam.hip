// Pooled beam search: the step that moves a hypothesis which takes EOS out of the beam into a per-image
// POOL of finished hypotheses scored by sum / len^alpha, so that the k rows of the beam stay live, and that closes an
// image once its pool cannot be improved — the sibling of beam_step_kernel on the same state (beam_step.h) — and the
// finalize that ranks the pool.
//
// A step at position t, one block per image.  Every live row (cumul > -inf; t = 0: row 0 alone) offers its k candidates
// — the k best admissible words OTHER than EOS, which the caller selects with EOS inadmissible — as slots 0..k-1 and EOS
// at the row's own log-prob for it (read from the log-prob rows the candidates came from) as slot k, the latter only at
// t >= min_words.  Wave 0 ranks the k·(k+1) <= 240 totals cumul + value with wave_extract_best, key = row·(k+1) + slot,
// and walks the ranking: a word becomes the next live row until k are chosen, an EOS met among the first k extractions
// is an offer to the pool, a later one is dropped; 2k extractions at most.  Threads 0..k-1 then re-sum the new rows'
// scores and threads 64.. the offers' (the order of beam_apply), thread 0 applies the offers to the pool one after the
// other and decides whether the image closes, all threads copy the accepted hypotheses' rows — read before beam_apply
// permutes them — and beam_apply does the rest.  A closed image's block only arrives at the counter.
//
// No powf on the device: len^alpha comes from a table the host builds in float64 and rounds once (scale[0..T]), and a
// score is one __fdiv_rn, so a float32 host model reproduces every pool field bit for bit (tests/pool_beam_model.py).
#include "beam_step.h"

namespace {

constexpr int POOL_MAX_K = 15;          // k·(k+1) candidates <= 256 = 64 lanes x BEAM_CPL

struct PoolParams {
  long long* tok; float* lp;            // [n_img, P, T]
  int* len; float* sum; float* score; int* serial;      // [n_img, P]
  int* count; int* closed;              // [n_img]
  const float* scale;                   // [T + 1]
  int min_words, early;
};

struct PoolShared {
  float psc[MAX_K]; int pser[MAX_K]; int cnt;           // the pool's scores and serials: the working copy of thread 0
  float elp[MAX_K];                                     // log-prob of EOS in every row
  int off_row[MAX_K]; float off_val[MAX_K]; float off_sum[MAX_K]; int off_len[MAX_K]; int off_slot[MAX_K]; int n_off;
  float ncu[MAX_K];                                     // cumul of the new rows
  int closing;
};

// One offer to the pool of P slots (one thread, on the working copy): appended while the pool is not full, else in place
// of the worst entry — lowest score, a tie to the highest serial — when strictly better.  → the slot, or -1.  The serial
// is one above the largest in the pool: later than every hypothesis the pool holds.
__device__ __forceinline__ int pool_worst(const PoolShared& x) {
  int w = 0;
  for (int i = 1; i < x.cnt; ++i)
    if ((x.psc[i] < x.psc[w]) | ((x.psc[i] == x.psc[w]) & (x.pser[i] > x.pser[w]))) w = i;
  return w;
}
__device__ __forceinline__ int pool_offer(PoolShared& x, int P, float sc) {
  int ser = 0;
  for (int i = 0; i < x.cnt; ++i) ser = max(ser, x.pser[i] + 1);
  int slot;
  if (x.cnt < P) {
    slot = x.cnt++;
  } else {
    slot = pool_worst(x);
    if (!(sc > x.psc[slot])) return -1;
  }
  x.psc[slot] = sc; x.pser[slot] = ser;
  return slot;
}

__device__ __forceinline__ void pool_load(const PoolParams& q, PoolShared& x, int b, int P) {
  const int tid = threadIdx.x;
  const int cnt = min(max(q.count[b], 0), P);
  if (tid == 0) x.cnt = cnt;
  if (tid < cnt) { x.psc[tid] = q.score[b * P + tid]; x.pser[tid] = q.serial[b * P + tid]; }
}

__device__ __forceinline__ void pool_store_entry(const PoolParams& q, const PoolShared& x, int b, int P, int i, int slot) {
  q.len[b * P + slot] = x.off_len[i]; q.sum[b * P + slot] = x.off_sum[i];
  q.score[b * P + slot] = x.psc[slot]; q.serial[b * P + slot] = x.pser[slot];
}

__device__ __forceinline__ float pool_score(const PoolParams& q, float sum, int len, int T) {
  return __fdiv_rn(sum, q.scale[min(max(len, 0), T)]);
}

// the selection and the walk (wave 0): s.parent / s.word / s.lp of the k rows, x.off_row / x.off_val / x.n_off
__device__ __forceinline__ void pool_beam_select(const BeamParams& p, BeamShared& s, PoolShared& x, int min_words, int t) {
  if (threadIdx.x >= 64) return;
  const int lane = threadIdx.x, k = p.k, k1 = k + 1;
  float tot[BEAM_CPL], val[BEAM_CPL]; int key[BEAM_CPL];
#pragma unroll
  for (int u = 0; u < BEAM_CPL; ++u) {
    const int i = lane + 64 * u;
    tot[u] = -INFINITY; val[u] = 0.f; key[u] = NO_KEY<int>;
    if (i < k * k1) {
      const int j = i / k1, c = i - j * k1;
      const bool is_eos = c == k;
      const bool live = t == 0 ? j == 0 : s.cu[j] > -INFINITY;
      const float v = is_eos ? x.elp[j] : s.cv[j * k + c];
      const float tt = t == 0 ? v : __fadd_rn(s.cu[j], v);
      if (live && (!is_eos || t >= min_words) && tt > -INFINITY) { tot[u] = tt; val[u] = v; key[u] = i; }
    }
  }
  int n_live = 0, n_off = 0;                             // (wave uniform)
  for (int ex = 0; ex < 2 * k && n_live < k; ++ex) {
    int bi; float bval;
    if (!wave_extract_best(tot, key, val, bi, bval)) break;
    const int j = bi / k1, c = bi - j * k1;              // a found key was put in above: j < k, c <= k
    if (c == k) {
      if (ex < k) {
        if (lane == 0) { x.off_row[n_off] = j; x.off_val[n_off] = bval; }
        ++n_off;
      }
    } else {
      if (lane == 0) { s.parent[n_live] = j; s.word[n_live] = s.ci[j * k + c]; s.lp[n_live] = bval; }
      ++n_live;
    }
  }
  if (lane == 0) {
    for (int r = n_live; r < k; ++r) { s.parent[r] = t == 0 ? 0 : r; s.word[r] = (int)p.eos; s.lp[r] = -INFINITY; }
    x.n_off = n_off;
  }
}

// the parent's per-token log-probs re-summed in position order, then + value: the order of beam_apply
__device__ __forceinline__ float resum(const BeamShared& s, int row, int t, float v) {
  const float* src = s.lpm[row];
  float cs = 0.f;
  for (int j = 0; j <= t; ++j) cs += src[j];
  return cs + v;
}

__global__ __launch_bounds__(256) void pool_beam_step_kernel(BeamParams p, EmbedArgs e, PoolParams q,
                                                             const float* __restrict__ logp, long ldl) {
  __shared__ BeamShared s;
  __shared__ PoolShared x;
  const int b = blockIdx.x, k = p.k, P = p.k, T = p.T, tid = threadIdx.x;
  const int t = *p.pos;
  if (t + 1 >= T) return;
  if (q.closed[b] != 0) {                                // (block uniform) a closed image only arrives
    if (tid == 0) beam_arrive(p, 0, t);
    return;
  }
  if (tid < k) x.elp[tid] = logp[((long)b * k + tid) * ldl + p.eos];
  pool_load(q, x, b, P);
  beam_load_rows(p, s, b, t);
  pool_beam_select(p, s, x, q.min_words, t);
  __syncthreads();
  if (tid < k) x.ncu[tid] = resum(s, s.parent[tid], t, s.lp[tid]);
  if (tid >= 64 && tid - 64 < x.n_off) {
    const int i = tid - 64, row = x.off_row[i];
    x.off_sum[i] = resum(s, row, t, x.off_val[i]);
    x.off_len[i] = (t == 0 ? 1 : s.ne[row]) + 1;
  }
  __syncthreads();
  if (tid == 0) {
    for (int i = 0; i < x.n_off; ++i) {
      const int slot = pool_offer(x, P, pool_score(q, x.off_sum[i], x.off_len[i], T));
      x.off_slot[i] = slot;
      if (slot >= 0) pool_store_entry(q, x, b, P, i, slot);
    }
    q.count[b] = x.cnt;
    int closing = 0;
    if (x.cnt == P) {
      float best = -INFINITY;
      for (int r = 0; r < k; ++r) best = x.ncu[r] > best ? x.ncu[r] : best;
      closing = (q.early != 0) | (x.psc[pool_worst(x)] >= __fdiv_rn(best, q.scale[T]));
    }
    x.closing = closing;
    if (closing) q.closed[b] = 1;
  }
  __syncthreads();
  // the accepted hypotheses: the parent's row as it stands before beam_apply permutes it, plus EOS; zero behind it.
  // (A thread writes the same columns for every offer, in walk order: a slot taken twice in one step keeps the last.)
  for (int i = 0; i < x.n_off; ++i) {
    const int slot = x.off_slot[i];
    if (slot < 0) continue;
    const long src = ((long)b * k + x.off_row[i]) * T, dst = ((long)b * P + slot) * T;
    for (int j = tid; j < T; j += BEAM_NT) {
      q.tok[dst + j] = j <= t ? p.tok[src + j] : (j == t + 1 ? p.eos : 0LL);
      q.lp[dst + j] = j <= t ? p.lp[src + j] : (j == t + 1 ? x.off_val[i] : 0.f);
    }
  }
  beam_apply(p, e, s, b, t, x.closing != 0);
}

// One block per image.  Thread 0: an image still open offers its live rows that have not ended (sum = cumul, len =
// n_elem, no EOS) in row order, then ranks the pool — score descending, a tie to the lower serial; all threads copy the
// accepted rows.  closed[b] gains bit 1, so a second call offers nothing again.
__global__ __launch_bounds__(256) void pool_beam_finalize_kernel(BeamParams p, PoolParams q, int* __restrict__ order,
                                                                 float* __restrict__ oscore) {
  __shared__ PoolShared x;
  const int b = blockIdx.x, k = p.k, P = p.k, T = p.T, tid = threadIdx.x;
  pool_load(q, x, b, P);
  __syncthreads();
  if (tid == 0) {
    int n_off = 0;
    if (q.closed[b] == 0) {
      for (int r = 0; r < k; ++r) {
        const float cu = p.cumul[b * k + r];
        if (!(cu > -INFINITY) || p.has_eos[b * k + r] != 0) continue;
        const int i = n_off++;
        x.off_row[i] = r; x.off_sum[i] = cu; x.off_len[i] = p.n_elem[b * k + r];
        const int slot = pool_offer(x, P, pool_score(q, cu, x.off_len[i], T));
        x.off_slot[i] = slot;
        if (slot >= 0) pool_store_entry(q, x, b, P, i, slot);
      }
    }
    x.n_off = n_off;
    q.count[b] = x.cnt;
    q.closed[b] |= 2;
    unsigned taken = 0;
    for (int r = 0; r < P; ++r) {
      int bi = -1;
      for (int j = 0; j < x.cnt; ++j)
        if (!((taken >> j) & 1u) &&
            (bi < 0 || x.psc[j] > x.psc[bi] || (x.psc[j] == x.psc[bi] && x.pser[j] < x.pser[bi]))) bi = j;
      if (bi >= 0) taken |= 1u << bi;
      order[b * P + r] = bi;
      oscore[b * P + r] = bi >= 0 ? x.psc[bi] : -INFINITY;
    }
  }
  __syncthreads();
  for (int i = 0; i < x.n_off; ++i) {
    const int slot = x.off_slot[i];
    if (slot < 0) continue;
    const int len = min(max(x.off_len[i], 0), T);
    const long src = ((long)b * k + x.off_row[i]) * T, dst = ((long)b * P + slot) * T;
    for (int j = tid; j < T; j += BEAM_NT) {
      q.tok[dst + j] = j < len ? p.tok[src + j] : 0LL;
      q.lp[dst + j] = j < len ? p.lp[src + j] : 0.f;
    }
  }
}

__global__ void pool_reset_kernel(int* count, int* closed, int n_img) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_img) { count[i] = 0; closed[i] = 0; }
}

int pool_params(PoolParams& q, const odic_pool_args* a, int32_t beams) {
  if (!a || beams < 1 || beams > POOL_MAX_K) return ODIC_EINVAL;
  if (!a->tokens || !a->logprobs || !a->len || !a->sum || !a->score || !a->serial || !a->count || !a->closed || !a->scale)
    return ODIC_EINVAL;
  if (a->min_words < 0) return ODIC_EINVAL;
  q.tok = (long long*)a->tokens; q.lp = a->logprobs; q.len = a->len; q.sum = a->sum; q.score = a->score;
  q.serial = a->serial; q.count = a->count; q.closed = a->closed; q.scale = a->scale;
  q.min_words = a->min_words; q.early = a->early_stopping;
  return 0;
}

}  // namespace

extern "C" int odic_pool_reset(const odic_pool_args* pool, int32_t n_img, void* stream) {
  if (!pool || !pool->count || !pool->closed || n_img <= 0 || n_img > 32767) return ODIC_EINVAL;
  hipLaunchKernelGGL(pool_reset_kernel, dim3((n_img + 255) / 256), dim3(256), 0, (hipStream_t)stream, pool->count,
                     pool->closed, n_img);
  return odic_launch_status();
}

extern "C" int odic_pool_beam_step(const float* cand_val, const int32_t* cand_idx, const float* logp, int64_t ldl,
                                   const odic_pool_args* pool, const odic_beam_state* st, const odic_embed_args* emb,
                                   int32_t n_img, int32_t beams, int32_t T, int64_t eos_idx, int32_t V, void* stream) {
  // one refusal code for this entry point
  if (!cand_val || !cand_idx || !logp || V < 1 || ldl < V || eos_idx < 0 || eos_idx >= V) return ODIC_EINVAL;
  BeamParams p; EmbedArgs e; PoolParams q;
  if (pool_params(q, pool, beams) != 0 || beam_params(p, e, st, emb, n_img, beams, T, eos_idx) != 0) return ODIC_EINVAL;
  p.cand_val = cand_val; p.cand_idx = cand_idx;
  hipLaunchKernelGGL(pool_beam_step_kernel, dim3(n_img), dim3(BEAM_NT), 0, (hipStream_t)stream, p, e, q, logp, (long)ldl);
  return odic_launch_status();
}

extern "C" int odic_pool_beam_finalize(const odic_pool_args* pool, const odic_beam_state* st, int32_t* order, float* score,
                                       int32_t n_img, int32_t beams, int32_t T, void* stream) {
  if (!order || !score) return ODIC_EINVAL;
  BeamParams p; EmbedArgs e; PoolParams q;
  if (pool_params(q, pool, beams) != 0 || beam_params(p, e, st, nullptr, n_img, beams, T, 0) != 0) return ODIC_EINVAL;
  hipLaunchKernelGGL(pool_beam_finalize_kernel, dim3(n_img), dim3(BEAM_NT), 0, (hipStream_t)stream, p, q, order, score);
  return odic_launch_status();
}
