// The (L + E) x L dot products of a sequence's dynamic expansion, shared by dynexp_seq_kernel (decoder_seq.hip) and
// dynexp_fill_caches_kernel (decoder_prefill.hip): rows a < L are cond_a, rows L..L+E-1 are qexp; columns are key_b.
//   CK[a][b] = cond_a·key_b   (row stride TS)        QK[e][b] = qexp[e]·key_b   (row stride TS)
// 4 x 4 register tiles of length-d dot products, float4 loads from the lin rows (cond at column 0, key at column d);
// every accumulator is one chain of fmaf in channel order, so the result does not depend on who calls this.
#pragma once

template <int NT>
__device__ __forceinline__ void dynexp_qk_ck_tiles(const float* lin, long ldlin, const float* qexp, int d, int E, int L,
                                                   int TS, float* QK, float* CK, int tid) {
  const int na = (L + E + 3) >> 2, nb = (L + 3) >> 2;
  for (int it = tid; it < na * nb; it += NT) {
    const int a0 = (it / nb) * 4, b0 = (it % nb) * 4;
    const float* ar[4]; const float* br[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int a = min(a0 + u, L + E - 1), b = min(b0 + u, L - 1);
      ar[u] = a < L ? lin + (long)a * ldlin : qexp + (long)(a - L) * d;
      br[u] = lin + (long)b * ldlin + d;
    }
    float acc[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int v = 0; v < 4; ++v) acc[u][v] = 0.f;
    for (int c = 0; c < d; c += 4) {
      float4 av[4], bv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { av[u] = *(const float4*)(ar[u] + c); bv[u] = *(const float4*)(br[u] + c); }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          float r = acc[u][v];
          r = fmaf(av[u].x, bv[v].x, r); r = fmaf(av[u].y, bv[v].y, r);
          r = fmaf(av[u].z, bv[v].z, r); r = fmaf(av[u].w, bv[v].w, r);
          asm volatile("" : "+v"(r));     // scalar FMAs: hipcc's SLP pass pairs neighbouring accumulators into packed fp32
                                          // ops with `op_sel` source selection otherwise (tests/test_isa_lint.py)
          acc[u][v] = r;
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int a = a0 + u, b = b0 + v;
        if (a < L + E && b < L) {
          if (a < L) CK[a * TS + b] = acc[u][v];
          else QK[(a - L) * TS + b] = acc[u][v];
        }
      }
  }
}
