// BLEU and ROUGE-L on token ids (include/odic_hip.h has the contracts, DESIGN.md §4.20 the reasoning): odic_bleu_stats
// counts the clipped n-gram matches of a hypothesis against a range of references on the term-frequency rows
// odic_cider_vectorize writes, one wave per query; odic_lcs_pairs takes the longest common subsequence of a hypothesis and
// one reference per wave, bit-parallel on two ballots per hypothesis token.  Integer results, integer reductions in a fixed
// tree, no atomics: two runs give the same bits.
#include "cider_row.h"

namespace {

constexpr int QW = 4;                          // waves (= queries, = pairs) per block
constexpr int SW = ODIC_BLEU_STAT_WORDS;

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ int clamp_len(int l, int max_len) { return min(max(l, 0), max_len); }

__global__ __launch_bounds__(QW * 64) void bleu_stats_kernel(const unsigned long long* __restrict__ ws, long ldw,
                                                             const int* __restrict__ lengths, int R, int max_len,
                                                             const int* __restrict__ hyp_row,
                                                             const int* __restrict__ ref_begin,
                                                             const int* __restrict__ ref_end, int Q, int* __restrict__ stats,
                                                             long lds) {
  const int lane = threadIdx.x & 63;
  const long q = (long)blockIdx.x * QW + (threadIdx.x >> 6);
  if (q >= Q) return;
  const int h = hyp_row[q];
  int out = 0;                                                 // lane i < SW holds word i of the query's row
  if (h >= 0 && h < R) {                                       // (wave-uniform)
    unsigned long long* base = const_cast<unsigned long long*>(ws);
    const int L = clamp_len(lengths[h], max_len);
    const int b = max(ref_begin[q], 0), e = min(ref_end[q], R);      // rows outside [0, R) are skipped
    int closest = 0, gap = 0, shortest = 0;
    unsigned total = 0;
    for (int j = b; j < e; ++j) {                              // the same few loads in every lane
      const int l = clamp_len(lengths[j], max_len), d = abs(l - L);
      if (j == b || d < gap || (d == gap && l < closest)) { gap = d; closest = l; }
      shortest = j == b ? l : min(shortest, l);
      total += (unsigned)l;
    }
    const Row a(base + (long)h * ldw);
    const int na = min(max(a.meta[0], 0), NK);
    int acc[4] = {0, 0, 0, 0};
    for (int g = lane; g < na; g += 64) {
      const unsigned long long k = a.keys[g];
      int most = 0;                                            // the largest count of this n-gram in one reference
      for (int j = b; j < e; ++j) {
        const Row r(base + (long)j * ldw);
        const int at = find_key(r.keys, min(max(r.meta[0], 0), NK), k);
        if (at >= 0) most = max(most, (int)r.w[at]);
      }
      const int c = min((int)a.w[g], most), ord = key_order(k);
#pragma unroll
      for (int o = 0; o < 4; ++o) acc[o] += o == ord ? c : 0;
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const int c = wave_sum_i32(acc[o]);
      if (lane == o) out = c;
    }
    if (lane >= 4 && lane < 8) out = max(0, L - (lane - 4));
    if (lane == 8) out = L;
    if (lane == 9) out = closest;
    if (lane == 10) out = shortest;
    if (lane == 11) out = (int)total;
  }
  if (lane < SW) stats[q * lds + lane] = out;
}

__device__ __forceinline__ unsigned long long low_bits(int n) { return n >= 64 ? ~0ull : (1ull << n) - 1ull; }

__global__ __launch_bounds__(QW * 64) void lcs_pairs_kernel(const int* __restrict__ tokens, long ld,
                                                            const int* __restrict__ lengths, int R, int max_len,
                                                            const int* __restrict__ ref_begin,
                                                            const int* __restrict__ ref_end, int H, int max_refs,
                                                            int* __restrict__ lcs, long ldl) {
  const int lane = threadIdx.x & 63;
  const long p = (long)blockIdx.x * QW + (threadIdx.x >> 6);
  if (p >= (long)H * max_refs) return;
  const int h = (int)(p / max_refs), s = (int)(p % max_refs);
  const long j = (long)ref_begin[h] + s;
  int out = 0;
  if (j >= 0 && j < R && j < ref_end[h]) {                     // (wave-uniform)
    const int Lh = clamp_len(lengths[h], max_len), Lr = clamp_len(lengths[j], max_len);
    // lane i holds tokens i and i + 64 of both rows; a slot behind the row's length is never loaded and never matches
    const bool r0 = lane < Lr, r1 = lane + 64 < Lr;
    const int ref0 = r0 ? tokens[j * ld + lane] : 0, ref1 = r1 ? tokens[j * ld + 64 + lane] : 0;
    const int hyp0 = lane < Lh ? tokens[(long)h * ld + lane] : 0;
    const int hyp1 = lane + 64 < Lh ? tokens[(long)h * ld + 64 + lane] : 0;
    // Hyyrö's bit-vector LCS: bit i of V is 0 where row i of the DP column grew; V' = (V + (V & M)) | (V & ~M) on 128 bits
    unsigned long long v0 = ~0ull, v1 = ~0ull;
    for (int i = 0; i < Lh; ++i) {
      const int t = i < 64 ? __shfl(hyp0, i, 64) : __shfl(hyp1, i - 64, 64);
      const unsigned long long m0 = __ballot(r0 && ref0 == t), m1 = __ballot(r1 && ref1 == t);
      const unsigned long long u0 = v0 & m0, u1 = v1 & m1;
      const unsigned long long s0 = v0 + u0, carry = s0 < v0 ? 1ull : 0ull;
      v1 = (v1 + u1 + carry) | (v1 & ~m1);
      v0 = s0 | (v0 & ~m0);
    }
    out = Lr - __popcll(v0 & low_bits(min(Lr, 64))) - __popcll(v1 & low_bits(max(Lr - 64, 0)));
  }
  if (lane == 0) lcs[(long)h * ldl + s] = out;
}

}  // namespace

extern "C" int odic_bleu_stats(const uint64_t* ws, int64_t ldw, const int32_t* lengths, int32_t R, int32_t max_len,
                               const int32_t* hyp_row, const int32_t* ref_begin, const int32_t* ref_end, int32_t Q,
                               int32_t* stats, int64_t lds, void* stream) {
  if (!ws || !lengths || !hyp_row || !ref_begin || !ref_end || !stats) return ODIC_ENULL;
  if (Q <= 0 || R <= 0) return ODIC_EINVAL;
  if (max_len < 0 || max_len > MAXLEN) return ODIC_EINVAL;
  if (ldw < ROW || lds < SW) return ODIC_EINVAL;
  hipLaunchKernelGGL(bleu_stats_kernel, dim3((unsigned)(((long)Q + QW - 1) / QW)), dim3(QW * 64), 0, (hipStream_t)stream,
                     (const unsigned long long*)ws, (long)ldw, lengths, R, max_len, hyp_row, ref_begin, ref_end, Q, stats,
                     (long)lds);
  return odic_launch_status();
}

extern "C" int odic_lcs_pairs(const int32_t* tokens, int64_t ld, const int32_t* lengths, int32_t R, int32_t max_len,
                              const int32_t* ref_begin, const int32_t* ref_end, int32_t H, int32_t max_refs, int32_t* lcs,
                              int64_t ldl, void* stream) {
  if (!tokens || !lengths || !ref_begin || !ref_end || !lcs) return ODIC_ENULL;
  if (R <= 0 || H <= 0 || H > R || max_refs <= 0) return ODIC_EINVAL;
  if (max_len < 0 || max_len > MAXLEN || ld < max_len || ldl < max_refs) return ODIC_EINVAL;
  const long pairs = (long)H * max_refs;
  if ((pairs + QW - 1) / QW > 0x7FFFFFFFL) return ODIC_EINVAL;
  hipLaunchKernelGGL(lcs_pairs_kernel, dim3((unsigned)((pairs + QW - 1) / QW)), dim3(QW * 64), 0, (hipStream_t)stream, tokens,
                     (long)ld, lengths, R, max_len, ref_begin, ref_end, H, max_refs, lcs, (long)ldl);
  return odic_launch_status();
}
