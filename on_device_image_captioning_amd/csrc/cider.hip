// CIDEr-D on token ids (include/odic_hip.h has the contract, DESIGN.md §4.19 the reasoning): odic_cider_vectorize turns
// every caption into its sorted TF-IDF n-gram vector, one block per caption with the caption's 512 key slots in LDS for
// the whole sort; odic_cider_pairs takes the clipped cosine of a hypothesis and one reference per wave.  Integer keys,
// fp64 weights, fixed reduction trees, no atomics: two runs give the same bits.
#include "cider_row.h"

namespace {

constexpr int VT = NK / 2, VW = VT / 64;       // vectorize: one thread per compare-exchange of the bitonic network
constexpr int PW = 4;                          // pairs: waves (= pairs) per block
constexpr unsigned long long NOKEY = ~0ull;    // sorts behind every key (a field holds id + 1 <= 65534, never 0xFFFF)

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(VT) void cider_vectorize_kernel(const int* __restrict__ tokens, long ld,
                                                             const int* __restrict__ lengths, int max_len, int max_id,
                                                             const unsigned long long* __restrict__ df_keys,
                                                             const double* __restrict__ df_idf, int n_table,
                                                             double default_idf, unsigned long long* __restrict__ ws,
                                                             long ldw) {
  __shared__ unsigned long long key[NK];
  __shared__ int tok[MAXLEN];
  __shared__ int start[NK + 1];                // first sorted position of every unique key; start[U] = n
  __shared__ int wave_heads[VW];
  __shared__ double wave_sq[VW][4];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int L = min(max(lengths[r], 0), max_len);
  if (tid < L) tok[tid] = min(max(tokens[(long)r * ld + tid], 0), max_id) + 1;
  __syncthreads();

  // the n-grams, order after order: order k has L - k + 1 of them (none once k > L)
  const int n1 = L, n2 = max(L - 1, 0), n3 = max(L - 2, 0), n4 = max(L - 3, 0);
  const int n = n1 + n2 + n3 + n4;
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int i = tid + e * VT;
    unsigned long long k = NOKEY;
    if (i < n) {
      int p = i, ord = 1;
      if (p >= n1) { p -= n1; ord = 2; if (p >= n2) { p -= n2; ord = 3; if (p >= n3) { p -= n3; ord = 4; } } }
      k = 0;
      for (int j = 0; j < ord; ++j) k |= (unsigned long long)tok[p + j] << (16 * j);
    }
    key[i] = k;
  }
  __syncthreads();

  // bitonic sort of the NK slots, ascending as unsigned values
  for (int k = 2; k <= NK; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      const int lo = ((tid & ~(j - 1)) << 1) | (tid & (j - 1)), hi = lo | j;
      const unsigned long long a = key[lo], b = key[hi];
      if ((a > b) == ((lo & k) == 0)) { key[lo] = b; key[hi] = a; }
      __syncthreads();
    }
  }

  // run heads: thread t owns positions 2t and 2t + 1; an exclusive scan of the head flags numbers the unique keys
  const int p0 = 2 * tid, p1 = p0 + 1;
  const bool h0 = p0 < n && (p0 == 0 || key[p0] != key[p0 - 1]);
  const bool h1 = p1 < n && key[p1] != key[p0];
  const int mine = (int)h0 + (int)h1;
  int incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  if (lane == 63) wave_heads[wv] = incl;
  __syncthreads();
  int before = incl - mine, U = 0;
#pragma unroll
  for (int w = 0; w < VW; ++w) { if (w < wv) before += wave_heads[w]; U += wave_heads[w]; }
  if (h0) start[before] = p0;
  if (h1) start[before + (int)h0] = p1;
  if (tid == 0) start[U] = n;
  __syncthreads();

  Row row(ws + (long)r * ldw);
  double sq[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int u = tid + e * VT;
    if (u < U) {
      const unsigned long long k = key[start[u]];
      double idf = default_idf;
      if (n_table > 0) {
        const int at = find_key(df_keys, n_table, k);
        if (at >= 0) idf = df_idf[at];
      }
      const double w = (double)(start[u + 1] - start[u]) * idf;
      row.keys[u] = k;
      row.w[u] = w;
      const int ord = key_order(k);
#pragma unroll
      for (int o = 0; o < 4; ++o) sq[o] += o == ord ? w * w : 0.0;
    }
  }
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    const double s = wave_sum_f64(sq[o]);
    if (lane == 0) wave_sq[wv][o] = s;
  }
  __syncthreads();
  if (tid < 4) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < VW; ++w) s += wave_sq[w][tid];
    row.norms[tid] = sqrt(s);
  }
  if (tid == 0) { row.meta[0] = U; row.meta[1] = n2; }   // the penalty's "length": the number of bigram tokens
}

__global__ __launch_bounds__(PW * 64) void cider_pairs_kernel(const unsigned long long* __restrict__ ws, long ldw, int R,
                                                              const int* __restrict__ ref_begin,
                                                              const int* __restrict__ ref_end, int H, int max_refs,
                                                              double* __restrict__ sim, long lds) {
  const int lane = threadIdx.x & 63;
  const long p = (long)blockIdx.x * PW + (threadIdx.x >> 6);
  if (p >= (long)H * max_refs) return;
  const int h = (int)(p / max_refs), s = (int)(p % max_refs);
  const long j = (long)ref_begin[h] + s;
  double out = 0.0;
  if (j >= 0 && j < R && j < ref_end[h]) {           // (wave-uniform)
    const Row a(const_cast<unsigned long long*>(ws) + (long)h * ldw), b(const_cast<unsigned long long*>(ws) + j * ldw);
    const int na = min(max(a.meta[0], 0), NK), nb = min(max(b.meta[0], 0), NK);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int g = lane; g < na; g += 64) {
      const unsigned long long k = a.keys[g];
      const int at = find_key(b.keys, nb, k);
      if (at >= 0) {
        const double wr = b.w[at], v = fmin(a.w[g], wr) * wr;
        const int ord = key_order(k);
#pragma unroll
        for (int o = 0; o < 4; ++o) acc[o] += o == ord ? v : 0.0;
      }
    }
    double total = 0.0;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      double v = wave_sum_f64(acc[o]);
      const double nh = a.norms[o], nr = b.norms[o];
      if (nh != 0.0 && nr != 0.0) v /= nh * nr;
      total += v;
    }
    const double delta = (double)(a.meta[1] - b.meta[1]);
    out = total * exp(-(delta * delta) / (2.0 * ODIC_CIDER_SIGMA * ODIC_CIDER_SIGMA)) * 0.25 * 10.0;
  }
  if (lane == 0) sim[(long)h * lds + s] = out;
}

}  // namespace

extern "C" int odic_cider_vectorize(const int32_t* tokens, int64_t ld, const int32_t* lengths, int32_t R, int32_t max_len,
                                    int32_t max_id, const uint64_t* df_keys, const double* df_idf, int32_t n_table,
                                    double default_idf, uint64_t* ws, int64_t ldw, void* stream) {
  if (!tokens || !lengths || !ws) return ODIC_ENULL;
  if (n_table > 0 && (!df_keys || !df_idf)) return ODIC_ENULL;
  if (R <= 0 || n_table < 0) return ODIC_EINVAL;
  if (max_len < 0 || max_len > MAXLEN || ld < max_len) return ODIC_EINVAL;
  if (max_id < 0 || max_id > ODIC_CIDER_MAX_ID) return ODIC_EINVAL;
  if (ldw < ROW) return ODIC_EINVAL;
  if (!(default_idf == default_idf)) return ODIC_EINVAL;
  hipLaunchKernelGGL(cider_vectorize_kernel, dim3(R), dim3(VT), 0, (hipStream_t)stream, tokens, (long)ld, lengths, max_len,
                     max_id, (const unsigned long long*)df_keys, df_idf, n_table, default_idf, (unsigned long long*)ws,
                     (long)ldw);
  return odic_launch_status();
}

extern "C" int odic_cider_pairs(const uint64_t* ws, int64_t ldw, int32_t R, const int32_t* ref_begin, const int32_t* ref_end,
                                int32_t H, int32_t max_refs, double* sim, int64_t lds, void* stream) {
  if (!ws || !ref_begin || !ref_end || !sim) return ODIC_ENULL;
  if (R <= 0 || H <= 0 || H > R || max_refs <= 0) return ODIC_EINVAL;
  if (ldw < ROW || lds < max_refs) return ODIC_EINVAL;
  const long pairs = (long)H * max_refs;
  if ((pairs + PW - 1) / PW > 0x7FFFFFFFL) return ODIC_EINVAL;
  hipLaunchKernelGGL(cider_pairs_kernel, dim3((unsigned)((pairs + PW - 1) / PW)), dim3(PW * 64), 0, (hipStream_t)stream,
                     (const unsigned long long*)ws, (long)ldw, R, ref_begin, ref_end, H, max_refs, sim, (long)lds);
  return odic_launch_status();
}
