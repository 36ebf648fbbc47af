// odic_logsoftmax_sample_filtered: the draws of odic_logsoftmax_sample (decoder_ops.hip) restricted to a temperature-
// scaled top-k / nucleus set, one block of 1024 threads per row (include/odic_hip.h has the contract, DESIGN.md §4.17 the
// reasoning).  No sort: the set is the rank-prefix up to one threshold word (value, index), found by bisection on the
// order-preserving integer key of z = x·inv_temperature — 32 rounds of a block-wide count (top-k) or mass sum (nucleus) —
// and, where the threshold value is shared by several words, a bisection on the index among them (the key, the block
// count and the bisection: row_bisect.h).  The model's own log-sum-exp, the noise and the draw rounds are
// odic_logsoftmax_sample's (row_sample.h), in its order of operations.
#include "row_sample.h"
#include "row_bisect.h"

namespace {

constexpr int NTH = 1024, NWV = NTH / 64;
constexpr int NPT = 16;                        // words a thread holds in registers: rows up to NPT·NTH = 16384 words

// #{ j in [0, cap) : before + j·w < P }: how many of `cap` equal words, each of mass w, start below P
__device__ __forceinline__ int ties_below(double before, double w, double P, int cap) {
  if (!(w > 0.0)) return cap;
  const double e = floor((P - before) / w);
  int n = e >= (double)cap ? cap : e > 0.0 ? (int)e : 0;
  while (n < cap && before + n * w < P) ++n;
  while (n > 0 && !(before + (n - 1) * w < P)) --n;
  return n;
}

template <int KM, bool REG>
__global__ __launch_bounds__(NTH) void sample_filter_kernel(const float* __restrict__ logits, long ldl,
                                                            float* __restrict__ logp_out, long ldp,
                                                            float* __restrict__ top_val, int* __restrict__ top_idx,
                                                            int* __restrict__ kept, int V, int k, float inv_t, int top_k,
                                                            float top_p, unsigned long long seed,
                                                            const int* __restrict__ pos) {
  __shared__ float red[NWV];
  __shared__ ArgmaxSlots<NWV> win;
  __shared__ CountMassSlots<NWV> cms;
  const int n = blockIdx.x, tid = threadIdx.x;
  const float* x = logits + (long)n * ldl;
  const unsigned step = pos ? (unsigned)*pos : 0u;

  // the model's own log-sum-exp and log-probs: unscaled, unfiltered, summed as odic_logsoftmax_sample sums them
  float xr[REG ? NPT : 1];
  float mx = -INFINITY;
  if constexpr (REG) {
#pragma unroll
    for (int u = 0; u < NPT; ++u) {
      const int i = tid + u * NTH;
      xr[u] = i < V ? x[i] : -INFINITY;
      mx = fmaxf(mx, xr[u]);
    }
  } else {
    for (int i = tid; i < V; i += NTH) mx = fmaxf(mx, x[i]);
  }
  const float m = block_max(mx, red);
  float s = 0.f;
  if constexpr (REG) {
#pragma unroll
    for (int u = 0; u < NPT; ++u)
      if (tid + u * NTH < V) s += expf(xr[u] - m);
  } else {
    for (int i = tid; i < V; i += NTH) s += expf(x[i] - m);
  }
  s = block_sum(s, red);
  const float lse = m + logf(s);
  if (logp_out) {
    if constexpr (REG) {
#pragma unroll
      for (int u = 0; u < NPT; ++u)
        if (tid + u * NTH < V) logp_out[(long)n * ldp + tid + u * NTH] = xr[u] - lse;
    } else {
      for (int i = tid; i < V; i += NTH) logp_out[(long)n * ldp + i] = x[i] - lse;
    }
  }

  // the thread's words as (key of z, mass exp(z - max z), index): held in registers, or re-read from the row
  const float zmax = __fmul_rn(m, inv_t);
  unsigned key[REG ? NPT : 1]; float wt[REG ? NPT : 1];
  if constexpr (REG) {
#pragma unroll
    for (int u = 0; u < NPT; ++u) {
      const float z = __fmul_rn(xr[u], inv_t);
      key[u] = rank_key(z); wt[u] = expf(z - zmax);
    }
  }
  auto each_key = [&](auto f) {
    if constexpr (REG) {
#pragma unroll
      for (int u = 0; u < NPT; ++u)
        if (tid + u * NTH < V) f(key[u], tid + u * NTH);
    } else {
      for (int i = tid; i < V; i += NTH) f(rank_key(__fmul_rn(x[i], inv_t)), i);
    }
  };
  auto each_mass = [&](auto f) {
    if constexpr (REG) {
#pragma unroll
      for (int u = 0; u < NPT; ++u)
        if (tid + u * NTH < V) f(key[u], wt[u]);
    } else {
      for (int i = tid; i < V; i += NTH) { const float z = __fmul_rn(x[i], inv_t); f(rank_key(z), expf(z - zmax)); }
    }
  };
  int rd = 0;
  double none = 0.0;
  auto count_ge = [&](unsigned t) {
    int c = 0;
    each_key([&](unsigned ky, int) { c += ky >= t ? 1 : 0; });
    block_count_mass<false>(c, none, cms, rd);
    return c;
  };
  auto mass_ge = [&](unsigned t) {
    int c = 0; double ms = 0.0;
    each_mass([&](unsigned ky, float w) { ms += ky >= t ? (double)w : 0.0; });
    block_count_mass<true>(c, ms, cms, rd);
    return ms;
  };
  // the words of value t and before it: gt = how many rank before that value, their mass, eq = how many share it
  auto tier = [&](unsigned t, int& gt, int& eq, double& mass_gt) {
    gt = 0; eq = 0; mass_gt = 0.0;
    each_mass([&](unsigned ky, float w) { gt += ky > t ? 1 : 0; mass_gt += ky > t ? (double)w : 0.0; });
    block_count_mass<true>(gt, mass_gt, cms, rd);
    each_key([&](unsigned ky, int) { eq += ky == t ? 1 : 0; });
    block_count_mass<false>(eq, none, cms, rd);
  };

  // K: the first kk words in rank order end inside value tK, with `in` of its eq words
  const int kk = (top_k == 0 || top_k >= V) ? V : top_k;
  unsigned ts = 0;
  if (kk < V) ts = bisect_max(32, [&](unsigned t) { return count_ge(t) >= kk; });
  int gt, eq; double mass_gt;
  tier(ts, gt, eq, mass_gt);                              // (kk == V: ts = 0 lies below every key, gt = V, eq = 0)
  int in = kk - gt, m_kept = kk;
  if (top_p < 1.f) {
    // nucleus: the words of K whose predecessors in K weigh less than P.  tq = the lowest value whose first word does
    const double massK = mass_gt + (in > 0 ? in * (double)expf(key_value(ts) - zmax) : 0.0);
    const double P = (double)top_p * massK;
    const unsigned tq = bisect_max(32, [&](unsigned t) { return mass_ge(t) >= P; });
    if (tq > ts) { ts = tq; tier(ts, gt, eq, mass_gt); in = eq; }          // else the nucleus ends inside value tK
    in = max(1, ties_below(mass_gt, (double)expf(key_value(ts) - zmax), P, in));
    m_kept = min(gt + in, kk);
  }
  if (kept && tid == 0) kept[n] = m_kept;
  // S: the first max(m, k) words in rank order, up to and including word (ts, is)
  if (m_kept < k) {
    ts = bisect_max(32, [&](unsigned t) { return count_ge(t) >= k; });
    tier(ts, gt, eq, mass_gt);
    in = k - gt;
  }
  int is = V - 1;
  if (in < eq) {                                          // the in-th word of value ts: `in - 1` of them lie before it
    is = (int)bisect_max(V > 1 ? 32 - __clz(V - 1) : 0, [&](unsigned j) {
      int c = 0;
      each_key([&](unsigned ky, int i) { c += ((ky == ts) & (i < (int)j)) ? 1 : 0; });
      block_count_mass<false>(c, none, cms, rd);
      return c < in;
    });
  }

  // the draws: odic_logsoftmax_sample's, on z, over S
  DrawList<KM> l;
  l.clear();
  for (int g4 = tid; g4 * 4 < V; g4 += NTH) {
    unsigned r[4];
    philox4x32_10((unsigned)n, (unsigned)g4, step, 0u, (unsigned)seed, (unsigned)(seed >> 32), r);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int vi = g4 * 4 + e;
      if (vi < V) {
        const float z = __fmul_rn(x[vi], inv_t);
        const unsigned ky = rank_key(z);
        if ((ky > ts) | ((ky == ts) & (vi <= is))) l.offer(z + gumbel_from_bits(r[e]), vi);
      }
    }
  }
  block_draw_rounds<KM>(l, x, V, k, lse, top_val + (long)n * k, top_idx + (long)n * k, nullptr, win);
}

template <int KM>
void launch(const float* logits, long ldl, float* logp_out, long ldp, float* top_val, int* top_idx, int* kept, int N, int V,
            int k, const odic_sample_filter& f, unsigned long long seed, const int* pos, hipStream_t s) {
  if (V <= NPT * NTH)
    hipLaunchKernelGGL((sample_filter_kernel<KM, true>), dim3(N), dim3(NTH), 0, s, logits, ldl, logp_out, ldp, top_val,
                       top_idx, kept, V, k, f.inv_temperature, f.top_k, f.top_p, seed, pos);
  else
    hipLaunchKernelGGL((sample_filter_kernel<KM, false>), dim3(N), dim3(NTH), 0, s, logits, ldl, logp_out, ldp, top_val,
                       top_idx, kept, V, k, f.inv_temperature, f.top_k, f.top_p, seed, pos);
}

}  // namespace

extern "C" int odic_logsoftmax_sample_filtered(const float* logits, int64_t ldl, float* logp_out, int64_t ldp,
                                               float* top_val, int32_t* top_idx, int32_t* kept, int32_t N, int32_t V,
                                               int32_t k, const odic_sample_filter* f, uint64_t seed, const int32_t* pos,
                                               void* stream) {
  if (!f || !logits || !top_val || !top_idx) return ODIC_EINVAL;
  if (!(f->inv_temperature > 0.f) || !(f->inv_temperature < INFINITY) || f->top_k < 0) return ODIC_EINVAL;
  if (!(f->top_p > 0.f) || !(f->top_p <= 1.f)) return ODIC_EINVAL;
  if (N < 1 || k < 1 || k > 16 || V < k || V > 262144) return ODIC_EINVAL;
  if (ldl < V || (logp_out && ldp < V)) return ODIC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (k <= 4) launch<4>(logits, ldl, logp_out, ldp, top_val, top_idx, kept, N, V, k, *f, seed, pos, s);
  else if (k <= 8) launch<8>(logits, ldl, logp_out, ldp, top_val, top_idx, kept, N, V, k, *f, seed, pos, s);
  else launch<16>(logits, ldl, logp_out, ldp, top_val, top_idx, kept, N, V, k, *f, seed, pos, s);
  return odic_launch_status();
}
