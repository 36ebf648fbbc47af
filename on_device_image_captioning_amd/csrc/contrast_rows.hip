// odic_contrast_topk: the candidates of a contrastive (emitter–suppressor) search step, one block of 512 threads per row
// (include/odic_hip.h has the contract, DESIGN.md §4.22 the reasoning).  The row of the target image and the rows of up
// to seven distractor images become  out[v] = lp_t[v] − w·max(log mean_d p_d[v], floor)  over the plausible words of the
// target, and the k best of them, in one launch:
//   1. the target row's maximum and log-sum-exp, formed as row_logsoftmax_topk (decoder_ops.hip) forms them — 512 threads,
//      thread t owns words t, t + 512, ..., the same wave and block order — so that a row with nothing to suppress gives
//      that kernel's numbers bit for bit.  That ownership is why the rows are read with 4-byte loads (a wave reads 256
//      contiguous bytes per instruction): a 16-byte load would hand a thread four neighbours and reorder the sum;
//   2. the plausible words are counted; a row with fewer than min_keep of them is cut at its min_keep-th ranked word
//      instead, found without a sort by the bisection of row_bisect.h (sample_filter.hip's);
//   3. every active distractor row's log-sum-exp (one pass each, the row in registers), then per word the log of the mean
//      probability in the log domain (the distractor words come back from L2: a row is 40 KB);
//   4. block_ranked_topk (row_select.h) over the scores, which a thread keeps in registers for V <= 10240; longer rows
//      stream and form a word's score again in every round — exact, just slower.
#include "row_bisect.h"

namespace {

constexpr int NTH = 512, NWV = NTH / 64;
constexpr int NPT = 10240 / NTH;               // words a thread holds in registers (row_logsoftmax_topk's slice)
constexpr int MAX_M = 8;                       // target + distractors

struct ContrastParams {
  const float* logits[MAX_M];
  const int* count;
  float* score_out; float* top_val; int* top_idx; int* kept;
  long ldl, lds;
  int M, V, k, min_keep;
  float w, log_alpha, floor;
};

// The maximum (mx) and max + log Σ exp(x − max) of row x in row_logsoftmax_topk's order of operations; REG: the thread's
// words stay in xr, -inf behind the row's end.
template <bool REG>
__device__ __forceinline__ float row_lse(const float* __restrict__ x, int V, float (&xr)[REG ? NPT : 1], float& mx,
                                         float* red) {
  const int tid = threadIdx.x;
  float tm = -INFINITY;
  if constexpr (REG) {
#pragma unroll
    for (int u = 0; u < NPT; ++u) { const int i = tid + u * NTH; xr[u] = i < V ? x[i] : -INFINITY; }
#pragma unroll
    for (int u = 0; u < NPT; ++u) tm = fmaxf(tm, xr[u]);
  } else {
    for (int i = tid; i < V; i += NTH) tm = fmaxf(tm, x[i]);
  }
  mx = block_max(tm, red);
  float s = 0.f;
  if constexpr (REG) {
#pragma unroll
    for (int u = 0; u < NPT; ++u) s += expf(xr[u] - mx);
  } else {
    for (int i = tid; i < V; i += NTH) s += expf(x[i] - mx);
  }
  return mx + logf(block_sum(s, red));
}

template <bool REG>
__global__ __launch_bounds__(NTH) void contrast_topk_kernel(ContrastParams p) {
  __shared__ float red[NWV];
  __shared__ float lse_d[MAX_M];
  __shared__ ArgmaxSlots<NWV> win;
  __shared__ CountMassSlots<NWV> cms;
  const int n = blockIdx.x, tid = threadIdx.x, V = p.V;
  const float* xt = p.logits[0] + (long)n * p.ldl;
  const int c = p.count ? min(max(p.count[n], 0), p.M - 1) : 0;      // active distractors: rows 1 .. c
  const bool on = (c > 0) & (p.w != 0.f);                            // (block-uniform) else the distractors are not read

  float xr[REG ? NPT : 1];
  float mx;
  const float lse = row_lse<REG>(xt, V, xr, mx, red);
  auto each_x = [&](auto f) {                                        // the thread's words of the target row
    if constexpr (REG) {
#pragma unroll
      for (int u = 0; u < NPT; ++u)
        if (tid + u * NTH < V) f(xr[u], tid + u * NTH);
    } else {
      for (int i = tid; i < V; i += NTH) f(xt[i], i);
    }
  };

  // plausibility: m words lie within log_alpha of the best; fewer than min_keep → the first min_keep in rank order,
  // up to and including word (ts, is)
  int rd = 0;
  double none = 0.0;
  auto count_if = [&](auto pred) {
    int cn = 0;
    each_x([&](float x, int i) { cn += pred(rank_key(x), i) ? 1 : 0; });
    block_count_mass<false>(cn, none, cms, rd);
    return cn;
  };
  int m = 0;
  each_x([&](float x, int) { m += __fsub_rn(x, mx) >= p.log_alpha ? 1 : 0; });
  block_count_mass<false>(m, none, cms, rd);
  if (p.kept && tid == 0) p.kept[n] = m;
  const bool byrank = m < p.min_keep;
  unsigned ts = 0; int is = V - 1;
  if (byrank) {
    const int nth = p.min_keep;
    ts = bisect_max(32, [&](unsigned t) { return count_if([&](unsigned ky, int) { return ky >= t; }) >= nth; });
    const int gt = count_if([&](unsigned ky, int) { return ky > ts; });
    const int eq = count_if([&](unsigned ky, int) { return ky == ts; });
    const int in = nth - gt;                                         // of the eq words of value ts
    if (in < eq)                                                     // the in-th of them: `in - 1` lie before it
      is = (int)bisect_max(V > 1 ? 32 - __clz(V - 1) : 0, [&](unsigned j) {
        return count_if([&](unsigned ky, int i) { return (ky == ts) & (i < (int)j); }) < in;
      });
  }
  auto admissible = [&](float x, int i) {
    const unsigned ky = rank_key(x);
    return byrank ? (ky > ts) | ((ky == ts) & (i <= is)) : __fsub_rn(x, mx) >= p.log_alpha;
  };

  // the suppressor: log of the mean probability of word i under the c active distractors, in the log domain
  if (on) {
    for (int d = 1; d <= c; ++d) {
      float xd[REG ? NPT : 1];
      float mxd;
      const float l = row_lse<REG>(p.logits[d] + (long)n * p.ldl, V, xd, mxd, red);
      if (tid == 0) lse_d[d] = l;
    }
    __syncthreads();
  }
  const float log_c = logf((float)c);
  auto suppress = [&](int i) {
    const long at = (long)n * p.ldl + i;
    if (c == 1) return p.logits[1][at] - lse_d[1];
    float mm = -INFINITY;
    for (int d = 1; d <= c; ++d) mm = fmaxf(mm, p.logits[d][at] - lse_d[d]);
    float acc = 0.f;
    for (int d = 1; d <= c; ++d) acc += expf((p.logits[d][at] - lse_d[d]) - mm);
    return mm > -INFINITY ? (mm + logf(acc)) - log_c : -INFINITY;    // (masked by every active distractor)
  };
  auto score = [&](float x, int i) {
    float o = x - lse;
    if (on) o = __fsub_rn(o, __fmul_rn(p.w, fmaxf(suppress(i), p.floor)));
    return admissible(x, i) ? o : -INFINITY;
  };
  // What the k rounds rank by.  A row with nothing to suppress ranks by its logits and reports x − lse, exactly as
  // row_logsoftmax_topk does (two logits may round to one log-prob; that kernel keeps the order of the logits).
  const float sub = on ? 0.f : lse;
  auto rank_value = [&](float x, int i) { return on ? score(x, i) : (admissible(x, i) ? x : -INFINITY); };

  float* so = p.score_out ? p.score_out + (long)n * p.lds : nullptr;
  if constexpr (REG) {
#pragma unroll
    for (int u = 0; u < NPT; ++u) {
      const int i = tid + u * NTH;
      if (i < V) {
        const float r = rank_value(xr[u], i);
        xr[u] = r;
        if (so) so[i] = r - sub;
      }
    }
  } else if (so) {
    for (int i = tid; i < V; i += NTH) so[i] = rank_value(xt[i], i) - sub;
  }
  block_ranked_topk<NTH>([&](float pv, int pi, float& best, int& besti) {
    if constexpr (REG) {
#pragma unroll
      for (int u = 0; u < NPT; ++u) {
        const float v = xr[u];
        const int i = tid + u * NTH;
        const bool after = ranks_after(v, i, pv, pi), before = ranks_before(v, i, best, besti);
        if ((i < V) & after & before) { best = v; besti = i; }
      }
    } else {
      for (int i = tid; i < V; i += NTH) {
        const float v = rank_value(xt[i], i);
        const bool after = ranks_after(v, i, pv, pi), before = ranks_before(v, i, best, besti);
        if (after & before) { best = v; besti = i; }
      }
    }
  }, p.k, sub, p.top_val + (long)n * p.k, p.top_idx + (long)n * p.k, win);
}

}  // namespace

extern "C" int odic_contrast_topk(const float* const* logits, int32_t M, int64_t ldl, const int32_t* count,
                                  const odic_contrast_args* a, float* score_out, int64_t lds, float* top_val,
                                  int32_t* top_idx, int32_t* kept, int32_t N, int32_t V, int32_t k, void* stream) {
  if (!logits || !a || !top_val || !top_idx) return ODIC_ENULL;
  if (M < 1 || M > MAX_M) return ODIC_EINVAL;
  for (int m = 0; m < M; ++m) if (!logits[m]) return ODIC_ENULL;
  if (M > 1 && !count) return ODIC_ENULL;
  if (N < 1 || k < 1 || k > 16 || k > V || V > 262144) return ODIC_EINVAL;
  if (ldl < V || (score_out && lds < V)) return ODIC_EINVAL;
  if (a->min_keep < k || a->min_keep > V) return ODIC_EINVAL;
  if (!(a->weight >= 0.f) || !(a->weight < INFINITY)) return ODIC_EINVAL;
  if (!(a->log_alpha <= 0.f)) return ODIC_EINVAL;                    // (> 0 or NaN; -inf = no cut)
  if (!(a->floor <= 0.f) || !(a->floor > -INFINITY)) return ODIC_EINVAL;
  ContrastParams p;
  for (int m = 0; m < MAX_M; ++m) p.logits[m] = m < M ? logits[m] : nullptr;
  p.count = M > 1 ? count : nullptr;
  p.score_out = score_out; p.top_val = top_val; p.top_idx = top_idx; p.kept = kept;
  p.ldl = (long)ldl; p.lds = (long)lds;
  p.M = M; p.V = V; p.k = k; p.min_keep = a->min_keep;
  p.w = a->weight; p.log_alpha = a->log_alpha; p.floor = a->floor;
  if (V <= NPT * NTH)
    hipLaunchKernelGGL(contrast_topk_kernel<true>, dim3(N), dim3(NTH), 0, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(contrast_topk_kernel<false>, dim3(N), dim3(NTH), 0, (hipStream_t)stream, p);
  return odic_launch_status();
}
