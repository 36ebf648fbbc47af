// bf16 NT GEMM with fused epilogue for gfx950:  out = act(alpha·A·Wᵀ + bias) + residual
//
//   A [M,K], W [N,K] bf16 row-major (K contiguous — the nn.Linear layout, so both MFMA operands are
//   read as 16-byte K-runs and nothing is ever transposed), fp32 accumulation.
//
// Structure (cdna_hip_programming.md §5):
//   * block tile BM x BN x 64 with NWM x NWN waves, each wave a (16·MI) x (16·NI) patch of
//     v_mfma_f32_16x16x32_bf16 tiles.  Three instantiations:
//        256x256 (2x4 waves of 128x64)  arithmetic intensity 128 FLOP per LDS-filled byte — the
//                                       large stage-2/3 products (73 % of all Swin FLOPs)
//        128x128 (2x2 waves of 64x64)   small N / tail-friendly
//        128x64  (2x2 waves of 64x32)   N = 192 style panels
//   * global → LDS by global_load_lds_dwordx4 (LDS-DMA, 1 KiB per wave-instruction, no VGPR round
//     trip).  The LDS image is lane-linear, so the bank-conflict XOR swizzle (16-byte chunk index
//     ^ (row & 7) inside each 128-byte row) is applied to the per-lane SOURCE address and again on
//     the ds_read_b128 fragment reads (rule 21: both sides or neither).
//   * two LDS stages: the DMA of K-tile t+1 is in flight while tile t feeds the MFMAs; one
//     s_waitcnt vmcnt(0) + barrier per K-tile.
//   * operands are SWAPPED in the MFMA (A-slot = W fragment, B-slot = activation fragment): the
//     accumulator tile is then Cᵀ, i.e. each lane holds 4 CONSECUTIVE OUTPUT COLUMNS of one output
//     row, so bias / activation / fp32 residual / output move as 16-byte (fp32) or 8-byte (bf16)
//     per-lane vectors straight from the accumulator registers — no LDS staging, no shuffles.
//   * XCD-aware 2-D tile partition: blocks b, b+8, ... share an XCD (and its 4 MiB L2); each XCD
//     owns a PM x PN rectangle of the tile grid chosen so that its W sub-panel stays L2-resident
//     while its A panels stream through once (PMC: L2 hit rate 70 % → see profiles/).
//   * rows/cols beyond M/N are clamped on load (valid memory, discarded on store).
// The swizzle, the W row permutation, the tile grid and the host's launch helpers are gemm_tile.h's, shared with
// gemm_x3.hip and gemm_lowp.hip (which repeat this kernel's rectangle walk, staging and counted wait as text).
#include "gemm_tile.h"
#include <stdio.h>
#include <stdlib.h>
#include <type_traits>

namespace {

struct Params {
  const bf16_raw* A; const bf16_raw* W; const float* bias; const float* residual; void* out;
  int M, N, K;
  long lda, ldw, ldr, ldc;
  long strideA, strideW, strideBias, strideR, strideC;
  float alpha; int act; int bias_axis;
  TileGrid grid;       // tile counts and XCD partition (gemm_tile.h)
  const float* a_ln; long ld_aln; float ln_eps;   // A-resident kernels: fp32 rows whose LayerNorm (no affine) is the A operand
};

// (second launch bound: the 4-wave blocks with 128 accumulator registers per lane must stay within 256 registers
//  so that two of them share a CU — left alone hipcc takes 158 + 128)
// KS = 2: TWO groups of NWM x NWN waves share the tile and its LDS stages; group g takes the 32-deep half g of every 64-deep
// K-tile (half the MFMAs each), group 1 hands its accumulators to group 0 through LDS after the loop (a fixed order of
// additions: deterministic, but not the summation order of the KS = 1 form).  For the tiles whose wave count does not fill
// four SIMDs evenly — 144 x 192 is six waves, the exact-round tile of the 9216 x 768 products — this gives every SIMD three
// waves.  Only group 0 stages (its vmcnt waits precede the barrier both groups meet at) and only group 0 stores.
template <int NWM, int NWN, int MI, int NI, int NSTAGE, int BK, typename OutT, int KS = 1>
__global__ __launch_bounds__(64 * NWM * NWN * KS, (NWM * NWN * KS == 4 && MI * NI == 32) ? 2 : 1) void gemm_bf16_nt_kernel(Params p) {
  static_assert(KS == 1 || (KS == 2 && BK == 64), "the K-split form is two groups on 64-deep K-tiles");
  constexpr int NW = NWM * NWN;
  constexpr int ROWB = BK * 2;                 // bytes per LDS row
  constexpr int RPI = 1024 / ROWB;             // rows per 1-KiB DMA instruction
  constexpr int CPR = ROWB / 16;               // 16-byte chunks per row
  constexpr int BM = NWM * MI * 16, BN = NWN * NI * 16;
  constexpr int A_BYTES = BM * BK * 2, W_BYTES = BN * BK * 2, STAGE = A_BYTES + W_BYTES;
  constexpr int A_INSTR = BM / RPI / NW, W_INSTR = BN / RPI / NW;  // 1-KiB DMA instructions per wave
  static_assert(BM % (RPI * NW) == 0 && BN % (RPI * NW) == 0, "tile rows must split evenly over the waves");
  constexpr int G = A_INSTR + W_INSTR;                                 // LDS-DMA instructions per wave per K-tile
  static_assert(NI % 2 == 0, "the epilogue pairs MFMA column tiles");
  constexpr int D = NSTAGE - 1;                                        // prefetch distance in K-tiles
  extern __shared__ __attribute__((aligned(16))) char lds[];          // stage0 {A,W} | stage1 {A,W}

  const int tid = threadIdx.x, lane = tid & 63;
  const int kg = KS == 1 ? 0 : __builtin_amdgcn_readfirstlane((tid >> 6) / NW);      // K group of this wave
  const int wave = KS == 1 ? (tid >> 6) : __builtin_amdgcn_readfirstlane((tid >> 6) % NW);
  const int wm = wave / NWN, wn = wave % NWN;
  ODIC_ENCODE_PRIO();

  // XCD x = blockIdx % 8 owns tile rows [r0,r1) x cols [c0,c1); inside the rectangle tiles run N-fastest
  int tm, tn;
  {
    const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    const int xm = xcd / p.grid.pn, xn = xcd - xm * p.grid.pn;
    const int r0 = xm * p.grid.tiles_m / p.grid.pm, r1 = (xm + 1) * p.grid.tiles_m / p.grid.pm;
    const int c0 = xn * p.grid.tiles_n / p.grid.pn, c1 = (xn + 1) * p.grid.tiles_n / p.grid.pn;
    const int w = c1 - c0;
    if (idx >= (r1 - r0) * w) return;             // rectangles differ by at most one row/col of tiles
    const int lr = idx / w;
    tm = r0 + lr; tn = c0 + (idx - lr * w);
  }
  const int m0 = tm * BM, n0 = tn * BN;
  const long bz = blockIdx.z;
  const bf16_raw* A = p.A + bz * p.strideA;
  const bf16_raw* W = p.W + bz * p.strideW;

  // ---- LDS-DMA source addresses: instruction i of this wave fills rows (i*NW+wave)*RPI .. +RPI-1
  const int srow = lane / CPR;
  const int schunk = swz<ROWB>(lane % CPR, srow);  // logical 16-byte chunk this lane must fetch
  const bf16_raw* a_src[A_INSTR];
  const bf16_raw* w_src[W_INSTR];
#pragma unroll
  for (int i = 0; i < A_INSTR; ++i) {
    const int row = (i * NW + wave) * RPI + srow;
    a_src[i] = A + (long)min(m0 + row, p.M - 1) * p.lda + schunk * 8;
  }
#pragma unroll
  for (int i = 0; i < W_INSTR; ++i) {
    const int row = (i * NW + wave) * RPI + srow;
    w_src[i] = W + (long)min(n0 + wperm(row), p.N - 1) * p.ldw + schunk * 8;
  }

  auto stage = [&](int buf, int kt) {
    if (KS == 2 && kg != 0) return;
    char* la = lds + buf * STAGE;
    char* lw = la + A_BYTES;
#pragma unroll
    for (int i = 0; i < A_INSTR; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(a_src[i] + (long)kt * BK), (lptr_t)(la + (i * NW + wave) * 1024), 16, 0, 0);
#pragma unroll
    for (int i = 0; i < W_INSTR; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(w_src[i] + (long)kt * BK), (lptr_t)(lw + (i * NW + wave) * 1024), 16, 0, 0);
  };

  f32x4_t acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int nk = p.K / BK;
  const int frow = lane & 15, fq = lane >> 4;

  // Pipeline: tiles kt+1 .. kt+D-1 stay in flight across the barrier (counted vmcnt: the wave's own
  // DMA groups retire in order, G instructions per tile; the raw s_barrier carries no implicit
  // vmcnt(0) drain).  After the barrier every wave's share of tile kt has landed AND every wave has
  // finished reading tile kt-1, whose buffer the prefetch of tile kt+D then overwrites.
#pragma unroll
  for (int t = 0; t < D; ++t)
    if (t < nk) stage(t, t);

  for (int kt = 0; kt < nk; ++kt) {
    const int ahead = min(D - 1, nk - 1 - kt);
    if (ahead >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * G) : "memory");
    else if (ahead == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(G) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (kt + D < nk) stage((kt + D) % NSTAGE, kt + D);

    const int cur = kt % NSTAGE;
    const char* la = lds + cur * STAGE + (wm * MI * 16 + frow) * ROWB;
    const char* lw = lds + cur * STAGE + A_BYTES + (wn * NI * 16 + frow) * ROWB;
#pragma unroll
    for (int kq = 0; kq < BK / 32 / KS; ++kq) {
      const int kk = KS == 1 ? kq : kg;
      bf16x8_t af[MI], wf[NI];
      const int chunk = swz<ROWB>(kk * 4 + fq, frow) << 4;
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) af[mi] = *(const bf16x8_t*)(la + mi * 16 * ROWB + chunk);
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) wf[ni] = *(const bf16x8_t*)(lw + ni * 16 * ROWB + chunk);
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[ni], af[mi], acc[mi][ni], 0, 0, 0);
    }
  }
  if constexpr (KS == 2) {
    // group 1 → LDS → group 0 (the stages are free: every wave is past its last fragment read at the barrier)
    f32x4_t* red = (f32x4_t*)lds + (long)wave * MI * NI * 64 + lane;
    __builtin_amdgcn_s_barrier();
    if (kg == 1) {
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) red[(i * NI + j) * 64] = acc[i][j];
    }
    __syncthreads();
    if (kg == 1) return;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NI; ++j) acc[i][j] += red[(i * NI + j) * 64];
  }
  // ---- epilogue.  With the operands swapped the 16x16 accumulator is Cᵀ: lane (frow, fq) register j
  //      holds output row frow, W-slot 4·fq + j.  The W rows were staged permuted (wperm above), so
  //      the slot pair (2q, 2q+1) of a lane covers 8 CONSECUTIVE output columns 32q + 8·fq .. +7:
  //      one 16-byte bf16 store (or two adjacent float4) per lane, 64/128 contiguous bytes per row.
  const float* bias = p.bias ? p.bias + bz * p.strideBias : nullptr;
  const float* resid = p.residual ? p.residual + bz * p.strideR : nullptr;
  OutT* out = (OutT*)p.out + bz * p.strideC;
  const bool ld_ok = ((p.ldc & 7) == 0) && (!resid || (p.ldr & 3) == 0) &&
                     ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
  if constexpr (sizeof(OutT) == 2 && NI % 4 == 0) {
    // bf16 output in WHOLE 128-byte lines.  A lane's 8 columns are 16 bytes, the four fq lanes of a row 64 contiguous
    // bytes: half a line per row and store instruction, and half-line stores run at 4 TB/s where whole lines run at
    // 6.8 (tools/smallk_probe.py).  The line's other half is the same lanes' NEXT column group: the two groups are
    // exchanged between lanes frow and frow ^ 8 (one DPP row rotation per dword), so that the low eight lanes of each
    // 16 hold both rows' first halves and the high eight both second halves — 8 rows x 128 bytes per store.
    if (ld_ok && (p.N & 63) == 0) {
      typedef __attribute__((ext_vector_type(4))) int i32x4_t;
      const bool lo = frow < 8;
#pragma unroll
      for (int q2 = 0; q2 < NI / 4; ++q2) {
        const int cbase = n0 + wn * NI * 16 + q2 * 64;            // wave-uniform
        if (cbase >= p.N) continue;
        f32x4_t bc[2][2];
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
          for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int e = 0; e < 4; ++e)
              bc[g][h][e] = (bias && !p.bias_axis) ? bias[cbase + g * 32 + fq * 8 + 4 * h + e] : 0.f;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
          const int r16 = m0 + (wm * MI + mi) * 16;
          const float brow = (bias && p.bias_axis) ? bias[min(r16 + frow, p.M - 1)] : 0.f;
          i32x4_t own[2];
#pragma unroll
          for (int g = 0; g < 2; ++g) {
            bf16x8_t pk;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              f32x4_t pre = acc[mi][4 * q2 + 2 * g + h] * p.alpha + bc[g][h] + brow;
              if (p.act == ODIC_ACT_GELU) {
                pre = gelu_poly4(pre);
              } else if (p.act != ODIC_ACT_NONE) {
#pragma unroll
                for (int e = 0; e < 4; ++e) pre[e] = apply_act<true>(pre[e], p.act);
              }
              if (resid) {
                const f32x4_t rr = *(const f32x4_t*)(resid + (long)min(r16 + frow, p.M - 1) * p.ldr + cbase + g * 32 + fq * 8 + 4 * h);
                pre += rr;
              }
#pragma unroll
              for (int e = 0; e < 4; ++e) pk[4 * h + e] = (short)f32_to_bf16(pre[e]);
            }
            own[g] = __builtin_bit_cast(i32x4_t, pk);
          }
          const i32x4_t send = lo ? own[1] : own[0];
          i32x4_t recv;
#pragma unroll
          for (int e = 0; e < 4; ++e) recv[e] = __builtin_amdgcn_update_dpp(0, send[e], 0x128, 0xf, 0xf, false);   // row_ror:8
          const int ra = r16 + (frow & 7);
          bf16_raw* dst = (bf16_raw*)out + (long)ra * p.ldc + cbase + (lo ? 0 : 32) + fq * 8;
          if (ra < p.M) *(i32x4_t*)dst = lo ? own[0] : recv;
          if (ra + 8 < p.M) *(i32x4_t*)(dst + 8 * p.ldc) = lo ? recv : own[1];
        }
      }
      return;
    }
  }
  if constexpr (!(sizeof(OutT) == 2 && NI % 4 == 0)) {   // (bf16 with NI % 4 == 0: whole-line path above, or the plain loop below)
    // The general vector path.  vmcnt retires in order and counts stores, so ANY load between two groups of stores
    // waits for every store before it: a bias or residual load per column group turned the epilogue into a chain of
    // memory round trips (9 per 144 x 192 tile; the "+16-20 us for the fp32 residual form" of DESIGN.md §4.1).  Here
    // every bias value is requested before the first store, and the residual rows of column group g + 1 are requested
    // BEFORE the stores of group g (they are then older than those stores, and waiting for them waits for nothing else).
    if (ld_ok && (p.N & 7) == 0) {
      constexpr int NG = NI / 2;
      // residual prefetch depth: 2 = pipelined as above (4- and 6-wave blocks: the registers are there), 1 = a group's
      // rows requested together (12-wave blocks), 0 = row by row (8-wave blocks: 32 more registers would cost them
      // their second resident block)
      constexpr int RD = sizeof(OutT) == 4 ? (NW <= 6 ? 2 : (NW >= 12 ? 1 : 0)) : 0;
      const int cw = n0 + wn * NI * 16 + fq * 8;
      f32x4_t bc[NG][2];
      float brow[MI];
#pragma unroll
      for (int nq = 0; nq < NG; ++nq) bc[nq][0] = bc[nq][1] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) brow[mi] = 0.f;
      if (bias && !p.bias_axis) {                       // (uniform branches around whole groups of loads)
        if ((reinterpret_cast<uintptr_t>(bias) & 15) == 0) {
#pragma unroll
          for (int nq = 0; nq < NG; ++nq) {
            const f32x4_t* bp = (const f32x4_t*)(bias + min(cw + nq * 32, p.N - 8));
            bc[nq][0] = bp[0]; bc[nq][1] = bp[1];
          }
        } else {
#pragma unroll
          for (int nq = 0; nq < NG; ++nq) {
            const float* bp = bias + min(cw + nq * 32, p.N - 8);
#pragma unroll
            for (int e = 0; e < 4; ++e) { bc[nq][0][e] = bp[e]; bc[nq][1][e] = bp[4 + e]; }
          }
        }
      } else if (bias) {
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) brow[mi] = bias[min(m0 + (wm * MI + mi) * 16 + frow, p.M - 1)];
      }
      // (two copies of the store loop, with and without a residual, so that the residual loads are unconditional:
      //  a load under a lane-dependent branch makes hipcc's wait insertion fall back to vmcnt(0))
      auto store_groups = [&](auto has_res) {
        constexpr bool HR = decltype(has_res)::value;
        f32x4_t rv[RD == 2 ? 2 : 1][(HR && RD) ? MI : 1][2];
        auto loadg = [&](int nq, int slot) {
          if constexpr (HR && RD > 0) {
            const int colc = min(cw + nq * 32, p.N - 8);
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
              const f32x4_t* rp = (const f32x4_t*)(resid + (long)min(m0 + (wm * MI + mi) * 16 + frow, p.M - 1) * p.ldr + colc);
              rv[slot][mi][0] = rp[0]; rv[slot][mi][1] = rp[1];
            }
          }
        };
        if constexpr (RD == 2) loadg(0, 0);
#pragma unroll
        for (int nq = 0; nq < NG; ++nq) {
          if constexpr (RD == 2) { if (nq + 1 < NG) loadg(nq + 1, (nq + 1) & 1); }
          if constexpr (RD == 1) loadg(nq, 0);
          const int col = cw + nq * 32;
#pragma unroll
          for (int mi = 0; mi < MI; ++mi) {
            const int row = m0 + (wm * MI + mi) * 16 + frow;
            f32x4_t v[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              f32x4_t pre = acc[mi][2 * nq + h] * p.alpha + bc[nq][h] + brow[mi];
              if (p.act == ODIC_ACT_GELU) {
                pre = gelu_poly4(pre);
              } else if (p.act != ODIC_ACT_NONE) {
#pragma unroll
                for (int e = 0; e < 4; ++e) pre[e] = apply_act<true>(pre[e], p.act);
              }
              v[h] = pre;
            }
            if constexpr (HR) {
              if constexpr (RD == 0) {
                const f32x4_t* rp = (const f32x4_t*)(resid + (long)min(row, p.M - 1) * p.ldr + min(col, p.N - 8));
                v[0] += rp[0]; v[1] += rp[1];
              } else {
                v[0] += rv[RD == 2 ? (nq & 1) : 0][mi][0]; v[1] += rv[RD == 2 ? (nq & 1) : 0][mi][1];
              }
            }
            if (row < p.M && col < p.N) {
              OutT* dst = out + (long)row * p.ldc + col;
              if constexpr (sizeof(OutT) == 4) {
                ((f32x4_t*)dst)[0] = v[0]; ((f32x4_t*)dst)[1] = v[1];
              } else {
                bf16x8_t pk;
#pragma unroll
                for (int e = 0; e < 4; ++e) { pk[e] = (short)f32_to_bf16(v[0][e]); pk[4 + e] = (short)f32_to_bf16(v[1][e]); }
                *(bf16x8_t*)dst = pk;
              }
            }
          }
        }
      };
      if (resid) store_groups(std::true_type{});
      else store_groups(std::false_type{});
      return;
    }
  }
#pragma unroll
  for (int nq = 0; nq < NI / 2; ++nq) {
    const int col = n0 + wn * NI * 16 + nq * 32 + fq * 8;
    if (col >= p.N) continue;
    float bc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) bc[e] = (bias && !p.bias_axis && col + e < p.N) ? bias[col + e] : 0.f;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      const int row = m0 + (wm * MI + mi) * 16 + frow;
      if (row >= p.M) continue;
      const float brow = (bias && p.bias_axis) ? bias[row] : 0.f;
      f32x4_t v[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        f32x4_t pre = acc[mi][2 * nq + h] * p.alpha + f32x4_t{bc[4 * h], bc[4 * h + 1], bc[4 * h + 2], bc[4 * h + 3]} + brow;
        if (p.act == ODIC_ACT_GELU) {
          pre = gelu_poly4(pre);
        } else if (p.act != ODIC_ACT_NONE) {
#pragma unroll
          for (int e = 0; e < 4; ++e) pre[e] = apply_act<true>(pre[e], p.act);
        }
        v[h] = pre;
      }
      if (ld_ok && col + 7 < p.N) {
        if (resid) {
          const f32x4_t* rp = (const f32x4_t*)(resid + (long)row * p.ldr + col);
          v[0] += rp[0]; v[1] += rp[1];
        }
        OutT* dst = out + (long)row * p.ldc + col;
        if constexpr (sizeof(OutT) == 4) {
          ((f32x4_t*)dst)[0] = v[0]; ((f32x4_t*)dst)[1] = v[1];
        } else {
          bf16x8_t pk;
#pragma unroll
          for (int e = 0; e < 4; ++e) { pk[e] = (short)f32_to_bf16(v[0][e]); pk[4 + e] = (short)f32_to_bf16(v[1][e]); }
          *(bf16x8_t*)dst = pk;
        }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          if (col + e < p.N) {
            float x = v[e >> 2][e & 3];
            if (resid) x += resid[(long)row * p.ldr + col + e];
            store_from_f32<OutT>(out + (long)row * p.ldc + col + e, x);
          }
        }
      }
    }
  }
}

// =================================================================================================
// A-resident streaming form for the K = 192 / 384 products of Swin stages 0-1 (tile_cfg 50-53).
//
// Those products (147456 x {576,192,768} x 192, 36864 x {1152,384,1536} x 384 at B = 16) are output-bandwidth-bound —
// 227-283 MB of traffic for 33-44 GFLOP — and the tiled kernel above spends 1.5-3x the time of a copy of the same
// bytes on them (tools/smallk_probe.py: fc1 of stage 0 145 us against 84 us for a device copy of twice its bytes):
// a K-loop of 3-6 steps is all pipeline fill, every tile re-stages its A rows once per column tile, and the stores of a
// round of tiles leave together.  Here nothing is re-staged and the stores never stop:
//   * a wave keeps its 16·MI rows of A over the WHOLE K extent in registers (MI · K/32 fragments, read once, straight
//     from global memory in MFMA operand layout — A never touches LDS);
//   * the block's four waves walk the output columns in chunks of 16·NI; a chunk of W (16·NI rows x K, 24 KiB) comes in
//     by LDS-DMA one chunk ahead into the other of two buffers, in the generic kernel's swizzled sub-tile images;
//   * one barrier per chunk; the counted wait in front of it lets the previous chunk's stores stay in flight
//     (vmcnt retires in order: the chunk's DMA was issued BEFORE those stores, so `vmcnt(stores per chunk)` proves it
//     landed) — the store stream of a wave overlaps its own next MFMA block, and the resident blocks of a CU
//     overlap each other's epilogue arithmetic.  (Tried and dropped: a fifth wave that only issues the DMA, so that
//     the compute waves never wait on vmcnt at all — 10 % slower; the store stream is not what the counted wait holds
//     back, the same kernel with MFMA and DMA switched off stores no faster.);
//   * whole tiles only (M % 64·MI == 0, N % 16·NI == 0, vector-store alignment): every wave issues exactly the counted
//     number of stores; anything else is refused and the caller's tuner falls back to the tiled kernel.
// Grid: row panels x `nsplit` column ranges; the ranges of one panel run on one XCD (its A rows come from that L2).
// =================================================================================================
template <int MI, int NI, int KT, int KH, typename OutT, bool RES, bool LNA = false>
__global__ __launch_bounds__(256, 2) void gemm_bf16_apanel_kernel(Params p, int nsplit) {
  constexpr int NW = 4;
  constexpr int BM = NW * MI * 16, BNC = NI * 16;
  constexpr int SUB = BNC * 128;                         // one 64-deep W sub-tile: BNC rows x 128 B
  // a chunk of W arrives in KH pieces along K (KH = 2 for K = 384: a 24-KiB buffer then holds half the K extent of 64
  // columns, so that the wave's column groups still pair into whole 128-byte output lines); one pipeline step per piece
  static_assert(KH == 1 || KH == 2, "one or two K pieces per chunk");
  constexpr int KTS = KT / KH;                           // 64-deep sub-tiles per step
  constexpr int CHUNK = KTS * SUB;                       // bytes per buffer
  static_assert(CHUNK % (1024 * NW) == 0, "a chunk must split into whole DMA instructions per wave");
  constexpr int INSTR = CHUNK / 1024 / NW;               // 1-KiB LDS-DMA instructions per wave per chunk
  constexpr int RG = BNC / 8;                            // 8-row DMA groups per sub-tile
  constexpr int NST = MI * (NI / 2) * (sizeof(OutT) == 4 ? 2 : 1);     // stores per wave per chunk
  static_assert(NI % 2 == 0 && NST <= 48, "store count must fit the vmcnt field with the DMA group on top");
  extern __shared__ __attribute__((aligned(16))) char lds[];          // W chunk buffers 0 | 1 | the block's bias values

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  ODIC_ENCODE_PRIO();
  const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
  const int split = idx % nsplit, panel = (idx / nsplit) * 8 + xcd;
  if (panel >= p.M / BM) return;
  const int nchunks = p.N / BNC;
  const int c0 = split * nchunks / nsplit, c1 = (split + 1) * nchunks / nsplit;
  if (c0 >= c1) return;
  const int m0 = panel * BM;
  const int frow = lane & 15, fq = lane >> 4;

  // ---- this wave's rows of A, whole K, as MFMA B-operand fragments: lane (frow, fq) holds A[row frow][32k + 8fq ..]
  bf16x8_t af[2 * KT][MI];
  if constexpr (LNA) {
    // LayerNorm while reading: the row's K fp32 values are spread over the four fq lanes (8 per 32-deep step each);
    // mean and centred variance in two passes over the registers, reduced across lanes frow, frow + 16, + 32, + 48,
    // then (x - mean)·rstd is rounded to bf16 straight into the fragments (gamma / beta are folded into W / bias).
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      const float* xr = p.a_ln + (long)(m0 + (wave * MI + mi) * 16 + frow) * p.ld_aln + fq * 8;
      if constexpr (KT > 3) {
        // K = 384: 96 fp32 values per lane and row would cost the kernel a resident block — moments in ONE pass over the
        // loads (shifted by the row's first element, which keeps E[(x-c)²] − E[x-c]² well conditioned), then the row is
        // read again (L1 / L2) and normalised into the fragments
        f32x4_t a0 = *(const f32x4_t*)xr;
        const float c = __shfl(a0[0], frow, 64);                         // x[row][0] (lane fq = 0 holds it)
        f32x4_t s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 2 * KT; ++k) {
          const f32x4_t u0 = *(const f32x4_t*)(xr + k * 32) - c, u1 = *(const f32x4_t*)(xr + k * 32 + 4) - c;
          s1 += u0 + u1;
          s2 += u0 * u0 + u1 * u1;
          if (k % 4 == 3) __builtin_amdgcn_sched_barrier(0);             // (at most 8 row loads in flight: registers)
        }
        float t1 = (s1[0] + s1[1]) + (s1[2] + s1[3]), t2 = (s2[0] + s2[1]) + (s2[2] + s2[3]);
        t1 += __shfl_xor(t1, 16, 64); t2 += __shfl_xor(t2, 16, 64);
        t1 += __shfl_xor(t1, 32, 64); t2 += __shfl_xor(t2, 32, 64);
        const float m1 = t1 * (1.0f / (64 * KT));
        const float mean = c + m1;
        const float rstd = rsqrtf(fmaxf(t2 * (1.0f / (64 * KT)) - m1 * m1, 0.f) + p.ln_eps);
#pragma unroll
        for (int k = 0; k < 2 * KT; ++k) {
          const f32x4_t u0 = (*(const f32x4_t*)(xr + k * 32) - mean) * rstd, u1 = (*(const f32x4_t*)(xr + k * 32 + 4) - mean) * rstd;
          bf16x8_t f;
#pragma unroll
          for (int e = 0; e < 4; ++e) { f[e] = (short)f32_to_bf16(u0[e]); f[4 + e] = (short)f32_to_bf16(u1[e]); }
          af[k][mi] = f;
          if (k % 4 == 3) __builtin_amdgcn_sched_barrier(0);
        }
        continue;
      }
      f32x4_t xv[2 * KT][2];
#pragma unroll
      for (int k = 0; k < 2 * KT; ++k) { xv[k][0] = *(const f32x4_t*)(xr + k * 32); xv[k][1] = *(const f32x4_t*)(xr + k * 32 + 4); }
      f32x4_t s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < 2 * KT; ++k) s4 += xv[k][0] + xv[k][1];
      float sum = (s4[0] + s4[1]) + (s4[2] + s4[3]);
      sum += __shfl_xor(sum, 16, 64);
      sum += __shfl_xor(sum, 32, 64);
      const float mean = sum / (float)(64 * KT);       // (a true division: a constant row then normalises to exactly 0)
      f32x4_t q4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < 2 * KT; ++k) {
        xv[k][0] -= mean; xv[k][1] -= mean;
        q4 += xv[k][0] * xv[k][0] + xv[k][1] * xv[k][1];
      }
      float ssq = (q4[0] + q4[1]) + (q4[2] + q4[3]);
      ssq += __shfl_xor(ssq, 16, 64);
      ssq += __shfl_xor(ssq, 32, 64);
      const float rstd = rsqrtf(ssq / (float)(64 * KT) + p.ln_eps);
#pragma unroll
      for (int k = 0; k < 2 * KT; ++k) {
        bf16x8_t f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          f[e] = (short)f32_to_bf16(xv[k][0][e] * rstd);
          f[4 + e] = (short)f32_to_bf16(xv[k][1][e] * rstd);
        }
        af[k][mi] = f;
      }
    }
  } else {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      const bf16_raw* ar = p.A + (long)(m0 + (wave * MI + mi) * 16 + frow) * p.lda + fq * 8;
#pragma unroll
      for (int k = 0; k < 2 * KT; ++k) af[k][mi] = *(const bf16x8_t*)(ar + k * 32);
    }
  }

  // ---- W chunk DMA: instruction i of this wave fills 1 KiB = rows 8·rg .. +7 of sub-tile kt, j = i·NW + wave
  int w_off[INSTR];                                       // element offsets inside a chunk (< 2^31: host-checked)
#pragma unroll
  for (int i = 0; i < INSTR; ++i) {
    const int j = i * NW + wave, kt = j / RG, rg = j - kt * RG;
    const int srow = lane >> 3, r = rg * 8 + srow;
    w_off[i] = wperm(r) * (int)p.ldw + kt * 64 + swz<128>(lane & 7, srow) * 8;
  }
  auto issue = [&](int c, int h, int buf) {
    const bf16_raw* wb = p.W + (long)c * BNC * p.ldw + h * KTS * 64;
    char* lb = lds + buf * CHUNK;
#pragma unroll
    for (int i = 0; i < INSTR; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(wb + w_off[i]), (lptr_t)(lb + (i * NW + wave) * 1024), 16, 0, 0);
  };

  const float* resid = p.residual;
  OutT* out = (OutT*)p.out;

  issue(c0, 0, 0);
  // the block's bias values go through LDS: a global load inside the chunk loop would be younger than the next
  // piece's DMA, and waiting for it (vmcnt retires in order) would wait for that DMA and every store before it
  float* sbias = (float*)(lds + 2 * CHUNK);
  for (int t = tid; t < (c1 - c0) * BNC; t += 256) sbias[t] = p.bias ? p.bias[c0 * BNC + t] : 0.f;
  // A fragments, first piece and bias staging complete.  (The builtin, not inline asm: hipcc's own wait insertion
  // must SEE that the A fragments have arrived, or it waits for vmcnt(0) at their first use in every iteration.)
  __builtin_amdgcn_s_waitcnt(0x0070);                                  // vmcnt(0) lgkmcnt(0)
  for (int c = c0; c < c1; ++c) {
    f32x4_t acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NI; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int h = 0; h < KH; ++h) {
      // this piece has landed: its DMA is older than the previous chunk's NST stores, which may stay in flight when
      // they are the only younger operations (h == 0); a second piece has nothing younger than itself ...
      if (h == 0) { if (c != c0) __builtin_amdgcn_s_waitcnt(0x0F70 | (NST & 15) | ((NST >> 4) << 14)); }   // vmcnt(NST)
      else __builtin_amdgcn_s_waitcnt(0x0F70);                                                             // vmcnt(0)
      // ... for every wave, and every wave is done reading the other buffer (the previous piece)
      __builtin_amdgcn_s_barrier();
      const int buf = KH == 2 ? h : ((c - c0) & 1);
      if (h + 1 < KH) issue(c, h + 1, buf ^ 1);
      else if (c + 1 < c1) issue(c + 1, 0, buf ^ 1);
      const char* lw = lds + buf * CHUNK + frow * 128;
#pragma unroll
      for (int kt = 0; kt < KTS; ++kt) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          bf16x8_t wf[NI];
          const int chunk = swz<128>(kk * 4 + fq, frow) << 4;
#pragma unroll
          for (int ni = 0; ni < NI; ++ni) wf[ni] = *(const bf16x8_t*)(lw + kt * SUB + ni * 16 * 128 + chunk);
#pragma unroll
          for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
              acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[ni], af[2 * (h * KTS + kt) + kk][mi], acc[mi][ni], 0, 0, 0);
        }
      }
    }

    // ---- epilogue of the chunk (lane → 8 adjacent columns as in the generic kernel; no bounds: whole tiles only)
    // the eight finished values of accumulator pair (mi, nq): alpha, bias, activation, residual
    auto finish = [&](int mi, int nq, f32x4_t* v) {
      const int col = c * BNC + nq * 32 + fq * 8;
      const f32x4_t* sb = (const f32x4_t*)(sbias + (c - c0) * BNC + nq * 32 + fq * 8);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        f32x4_t pre = acc[mi][2 * nq + h] * p.alpha + sb[h];
        if (p.act == ODIC_ACT_GELU) {
          pre = gelu_poly4(pre);
        } else if (p.act != ODIC_ACT_NONE) {
#pragma unroll
          for (int e = 0; e < 4; ++e) pre[e] = apply_act<true>(pre[e], p.act);
        }
        v[h] = pre;
      }
      if constexpr (RES) {
        const f32x4_t* rp = (const f32x4_t*)(resid + (long)(m0 + (wave * MI + mi) * 16 + frow) * p.ldr + col);
        v[0] += rp[0]; v[1] += rp[1];
      }
    };
    if constexpr (sizeof(OutT) == 2 && NI % 4 == 0) {
      // bf16 output, WHOLE 128-byte lines per store instruction.  A lane's 8 columns are 16 bytes and the four fq lanes
      // of a row make 64 contiguous bytes — half a cache line per row, and half-line stores run at 4 TB/s where whole
      // lines run at 6.8 (tools/smallk_probe.py).  The other half of the line is the same lanes' NEXT column group, so
      // the two groups are exchanged between lanes frow and frow ^ 8 (one DPP row rotation by 8 per dword): the low
      // eight lanes of each 16 then hold both rows' first halves, the high eight both rows' second halves, and each
      // store instruction writes 8 rows x 128 bytes.
      typedef __attribute__((ext_vector_type(4))) int i32x4_t;
      const bool lo = frow < 8;
#pragma unroll
      for (int q2 = 0; q2 < NI / 4; ++q2) {
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
          f32x4_t v0[2], v1[2];
          finish(mi, 2 * q2, v0);
          finish(mi, 2 * q2 + 1, v1);
          bf16x8_t p0, p1;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            p0[e] = (short)f32_to_bf16(v0[0][e]); p0[4 + e] = (short)f32_to_bf16(v0[1][e]);
            p1[e] = (short)f32_to_bf16(v1[0][e]); p1[4 + e] = (short)f32_to_bf16(v1[1][e]);
          }
          const i32x4_t own0 = __builtin_bit_cast(i32x4_t, p0), own1 = __builtin_bit_cast(i32x4_t, p1);
          const i32x4_t send = lo ? own1 : own0;
          i32x4_t recv;
#pragma unroll
          for (int e = 0; e < 4; ++e) recv[e] = __builtin_amdgcn_update_dpp(0, send[e], 0x128, 0xf, 0xf, false);   // row_ror:8
          // first store: rows 0-7 of the 16 (low lanes: own first half; high lanes: row frow - 8's second half)
          const long rbase = (long)(m0 + (wave * MI + mi) * 16 + (frow & 7)) * p.ldc + c * BNC + q2 * 64 + (lo ? 0 : 32) + fq * 8;
          *(i32x4_t*)(out + rbase) = lo ? own0 : recv;
          *(i32x4_t*)(out + rbase + 8 * p.ldc) = lo ? recv : own1;
        }
      }
    } else {
#pragma unroll
      for (int nq = 0; nq < NI / 2; ++nq) {
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
          f32x4_t v[2];
          finish(mi, nq, v);
          OutT* dst = out + (long)(m0 + (wave * MI + mi) * 16 + frow) * p.ldc + c * BNC + nq * 32 + fq * 8;
          if constexpr (sizeof(OutT) == 4) {
            ((f32x4_t*)dst)[0] = v[0]; ((f32x4_t*)dst)[1] = v[1];
          } else {
            bf16x8_t pk;
#pragma unroll
            for (int e = 0; e < 4; ++e) { pk[e] = (short)f32_to_bf16(v[0][e]); pk[4 + e] = (short)f32_to_bf16(v[1][e]); }
            *(bf16x8_t*)dst = pk;
          }
        }
      }
    }
  }
}

template <int MI, int NI, int KT, int KH = 1>
int launch_apanel(Params& p, int out_dtype, int batch, hipStream_t stream) {
  constexpr int BM = 4 * MI * 16, BNC = NI * 16;
  if (batch != 1 || p.K != KT * 64 || p.M % BM != 0 || p.N % BNC != 0 || p.bias_axis != 0)
    return ODIC_EUNSUPPORTED;
  if ((long)BNC * p.ldw >= (1L << 30) || (p.residual && MI > 2))       // (the residual form of the 64-row waves would spill)
    return ODIC_EUNSUPPORTED;
  if ((p.ldc & 7) || ((uintptr_t)p.out & 15) || (p.residual && ((p.ldr & 3) || ((uintptr_t)p.residual & 15))))
    return ODIC_EUNSUPPORTED;
  const int panels = p.M / BM, nchunks = p.N / BNC;
  // column ranges per panel: the smallest divisor of the chunk count that gives the chip >= `want` blocks (3 rounds of 2
  // per CU) — a block should keep its A rows for as many chunks as the grid size allows
  static const int want = getenv("ODIC_APANEL_BLOCKS") ? atoi(getenv("ODIC_APANEL_BLOCKS")) : 1536;
  const int nsplit = panel_split(panels, nchunks, want);
  dim3 grid(8 * ((panels + 7) / 8) * nsplit), block(256);
  const int SHMEM = 2 * (KT / KH) * BNC * 128 + (nchunks + nsplit - 1) / nsplit * BNC * 4;     // W buffers + the block's bias values
  if (SHMEM > 64 * 1024) return ODIC_EUNSUPPORTED;
  if (p.a_ln) {                       // LayerNorm-while-reading form: bf16 / fp32 output, no residual
    if (p.residual || (p.ld_aln & 3) || ((uintptr_t)p.a_ln & 15)) return ODIC_EUNSUPPORTED;
    if (out_dtype == ODIC_BF16) hipLaunchKernelGGL((gemm_bf16_apanel_kernel<MI, NI, KT, KH, bf16_raw, false, true>), grid, block, SHMEM, stream, p, nsplit);
    else hipLaunchKernelGGL((gemm_bf16_apanel_kernel<MI, NI, KT, KH, float, false, true>), grid, block, SHMEM, stream, p, nsplit);
    return odic_launch_status();
  }
  if constexpr (MI <= 2) {
    if (p.residual) {
      if (out_dtype == ODIC_BF16) hipLaunchKernelGGL((gemm_bf16_apanel_kernel<MI, NI, KT, KH, bf16_raw, true>), grid, block, SHMEM, stream, p, nsplit);
      else hipLaunchKernelGGL((gemm_bf16_apanel_kernel<MI, NI, KT, KH, float, true>), grid, block, SHMEM, stream, p, nsplit);
      return odic_launch_status();
    }
  }
  if (out_dtype == ODIC_BF16) hipLaunchKernelGGL((gemm_bf16_apanel_kernel<MI, NI, KT, KH, bf16_raw, false>), grid, block, SHMEM, stream, p, nsplit);
  else hipLaunchKernelGGL((gemm_bf16_apanel_kernel<MI, NI, KT, KH, float, false>), grid, block, SHMEM, stream, p, nsplit);
  return odic_launch_status();
}

// =================================================================================================
// The MLP of a Swin block of width C = 64·KT in ONE launch:  out = x + fc2(GELU(fc1(LN0(x))))  (odic_swin_mlp).
//
// As two launches (the LNA form above, then the tiled kernel) the bf16 hidden tensor [M, 4C] is written once and read
// once — 2 x 226 MB per stage-0 block at B = 16, two thirds of the pair's traffic — and nothing else reads it.  Here it
// never leaves the registers.  What makes that free is the swapped-operand accumulator layout: a lane's finished pair
// (2q, 2q+1) of fc1 tiles is row frow, hidden columns 32q + 8·fq .. +7 (the epilogue note of the tiled kernel), which is
// the B-operand fragment of v_mfma_f32_16x16x32_bf16 for the 32-deep K step q.  After bias, GELU and rounding to bf16 a
// wave's 64-column fc1 chunk IS its fc2 activation fragment pair: no LDS, no shuffle, no store.
//   * a wave keeps its 16·MI rows as LayerNorm-ed fragments over the whole K = C (the LNA prologue, the same bits) and
//     MI x C/16 fp32 output accumulators for the whole launch;
//   * the block walks the hidden dimension in chunks of 64: phase A = fc1 of the chunk (W1 rows 64c .. +63, 24 KiB at
//     C = 192) → hidden fragments; phase B = two 32-deep K steps of fc2 (W2 columns 64c .. +63 of all C rows, through
//     wperm, 24 KiB) into the output accumulators;
//   * one LDS buffer per operand: W2(c) is requested after the barrier in front of phase A, W1(c+1) after the barrier in
//     front of phase B, so each phase computes under the other operand's DMA; two barriers per chunk.  The DMA group is
//     the only outstanding vector-memory operation inside the loop, so its wait is vmcnt(0);
//   * epilogue once per block: alpha2, bias, the residual rows re-read from x (L2 / Infinity Cache hits), float4 pairs.
// Every output element is one accumulator chain over ascending 32-deep steps, as in the tiled kernel, and both epilogue
// expressions are the ones of the kernels this replaces: the result is bit-identical to the two launches.
// `out` may be `x` itself: a lane re-reads exactly the elements it then writes, and a row belongs to one wave.
// =================================================================================================
struct MlpParams {
  const float* x; float* out; const bf16_raw* W1; const float* b1; const bf16_raw* W2; const float* b2;
  long ldx, ldo; int M;
  float alpha1, alpha2, ln_eps;
};

template <int MI, int KT>
__global__ __launch_bounds__(256, 2) void swin_mlp_kernel(MlpParams p) {
  constexpr int NW = 4;
  constexpr int C = KT * 64, H = 4 * C, BM = NW * MI * 16;
  constexpr int NO = C / 16;                             // fc2 output tiles per 16 rows
  constexpr int SUB = 64 * 128;                          // one 64-deep sub-tile of the W1 chunk: 64 rows x 128 B
  constexpr int W1B = KT * SUB, W2B = C * 128;           // bytes per buffer (equal: 64·C bf16 each)
  constexpr int I1 = W1B / 1024 / NW, I2 = W2B / 1024 / NW;            // 1-KiB LDS-DMA instructions per wave per chunk
  static_assert(W1B % (1024 * NW) == 0 && W2B % (1024 * NW) == 0, "a chunk must split into whole DMA instructions per wave");
  extern __shared__ __attribute__((aligned(16))) char lds[];          // W1 chunk | W2 chunk | fc1 bias [H] | fc2 bias [C]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  ODIC_ENCODE_PRIO();
  const int m0 = blockIdx.x * BM;                        // (blocks b, b + 8, ... share an XCD: consecutive panels spread over all eight)
  // (the two alphas live in VGPRs: a packed multiply by one scalar of an SGPR pair is the `op_sel` source-selection form
  //  the ISA lint forbids — DESIGN.md §5)
  float alpha1_v = p.alpha1, alpha2_v = p.alpha2;
  asm volatile("" : "+v"(alpha1_v), "+v"(alpha2_v));
  const int frow = lane & 15, fq = lane >> 4;

  // ---- W chunk DMA (element offsets inside a chunk).  W1: sub-tile kt, rows 8·rg .. +7 as in the A-resident kernel;
  //      W2: C rows of 128 B, rows 8·j .. +7
  int w1_off[I1], w2_off[I2];
  {
    const int srow = lane >> 3, sch = swz<128>(lane & 7, srow) * 8;
#pragma unroll
    for (int i = 0; i < I1; ++i) {
      const int j = i * NW + wave, kt = j / 8, rg = j - kt * 8;
      w1_off[i] = wperm(rg * 8 + srow) * C + kt * 64 + sch;
    }
#pragma unroll
    for (int i = 0; i < I2; ++i) w2_off[i] = wperm((i * NW + wave) * 8 + srow) * H + sch;
  }
  char* const l1 = lds;
  char* const l2 = lds + W1B;
  auto issue1 = [&](int c) {
    const bf16_raw* wb = p.W1 + (long)c * 64 * C;
#pragma unroll
    for (int i = 0; i < I1; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(wb + w1_off[i]), (lptr_t)(l1 + (i * NW + wave) * 1024), 16, 0, 0);
  };
  auto issue2 = [&](int c) {
    const bf16_raw* wb = p.W2 + c * 64;
#pragma unroll
    for (int i = 0; i < I2; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(wb + w2_off[i]), (lptr_t)(l2 + (i * NW + wave) * 1024), 16, 0, 0);
  };
  issue1(0);
  float* sb1 = (float*)(lds + W1B + W2B);
  float* sb2 = sb1 + H;
  for (int t = tid; t < H; t += 256) sb1[t] = p.b1[t];
  for (int t = tid; t < C; t += 256) sb2[t] = p.b2[t];

  // ---- this wave's rows, LayerNorm-ed while read, as MFMA B-operand fragments (gemm_bf16_apanel_kernel's LNA prologue,
  //      KT <= 3 form, statement for statement: the fragments are the same bits)
  bf16x8_t af[2 * KT][MI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const float* xr = p.x + (long)(m0 + (wave * MI + mi) * 16 + frow) * p.ldx + fq * 8;
    f32x4_t xv[2 * KT][2];
#pragma unroll
    for (int k = 0; k < 2 * KT; ++k) { xv[k][0] = *(const f32x4_t*)(xr + k * 32); xv[k][1] = *(const f32x4_t*)(xr + k * 32 + 4); }
    f32x4_t s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 2 * KT; ++k) s4 += xv[k][0] + xv[k][1];
    float sum = (s4[0] + s4[1]) + (s4[2] + s4[3]);
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float mean = sum / (float)(64 * KT);       // (a true division: a constant row then normalises to exactly 0)
    f32x4_t q4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 2 * KT; ++k) {
      xv[k][0] -= mean; xv[k][1] -= mean;
      q4 += xv[k][0] * xv[k][0] + xv[k][1] * xv[k][1];
    }
    float ssq = (q4[0] + q4[1]) + (q4[2] + q4[3]);
    ssq += __shfl_xor(ssq, 16, 64);
    ssq += __shfl_xor(ssq, 32, 64);
    const float rstd = rsqrtf(ssq / (float)(64 * KT) + p.ln_eps);
#pragma unroll
    for (int k = 0; k < 2 * KT; ++k) {
      bf16x8_t f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        f[e] = (short)f32_to_bf16(xv[k][0][e] * rstd);
        f[4 + e] = (short)f32_to_bf16(xv[k][1][e] * rstd);
      }
      af[k][mi] = f;
    }
  }

  f32x4_t acc2[MI][NO];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NO; ++j) acc2[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // rows, first W1 chunk and bias staging complete (the builtin: hipcc's wait insertion must see the rows arrive)
  __builtin_amdgcn_s_waitcnt(0x0070);                                  // vmcnt(0) lgkmcnt(0)
  const char* lw1 = l1 + frow * 128;
  const char* lw2 = l2 + frow * 128;
  for (int c = 0; c < H / 64; ++c) {
    // W1(c) has landed for every wave, and every wave is done with W2(c-1)
    __builtin_amdgcn_s_waitcnt(0x0F70);                                // vmcnt(0)
    __builtin_amdgcn_s_barrier();
    issue2(c);
    // ---- phase A: 64 hidden columns of fc1
    f32x4_t acc1[MI][4];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc1[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        bf16x8_t wf[4];
        const int chunk = swz<128>(kk * 4 + fq, frow) << 4;
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) wf[ni] = *(const bf16x8_t*)(lw1 + kt * SUB + ni * 16 * 128 + chunk);
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int ni = 0; ni < 4; ++ni)
            acc1[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[ni], af[2 * kt + kk][mi], acc1[mi][ni], 0, 0, 0);
      }
    }
    // the chunk's epilogue as the A-resident kernel writes it (alpha, bias, GELU, bf16): pair q → fragment of K step q
    bf16x8_t hf[2][MI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const f32x4_t* sb = (const f32x4_t*)(sb1 + c * 64 + q * 32 + fq * 8);
        bf16x8_t f;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          f32x4_t pre = acc1[mi][2 * q + h] * alpha1_v + sb[h];
          pre = gelu_poly4(pre);
#pragma unroll
          for (int e = 0; e < 4; ++e) f[4 * h + e] = (short)f32_to_bf16(pre[e]);
        }
        hf[q][mi] = f;
      }
    }
    // W2(c) has landed for every wave, and every wave is done with W1(c)
    __builtin_amdgcn_s_waitcnt(0x0F70);                                // vmcnt(0)
    __builtin_amdgcn_s_barrier();
    if (c + 1 < H / 64) issue1(c + 1);
    // ---- phase B: two 32-deep K steps of fc2, four output tiles at a time
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int chunk = swz<128>(kk * 4 + fq, frow) << 4;
#pragma unroll
      for (int n4 = 0; n4 < NO / 4; ++n4) {
        bf16x8_t wf[4];
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) wf[ni] = *(const bf16x8_t*)(lw2 + (n4 * 4 + ni) * 16 * 128 + chunk);
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int ni = 0; ni < 4; ++ni)
            acc2[mi][n4 * 4 + ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[ni], hf[kk][mi], acc2[mi][n4 * 4 + ni], 0, 0, 0);
      }
    }
  }

  // ---- epilogue (the tiled kernel's fp32 vector path with a residual: the rows of column group q + 1 are requested
  //      before the stores of group q; no bounds: whole panels only)
  constexpr int NG = NO / 2;
  const float brow = 0.f;                                // (the tiled kernel's row-bias term, absent here, kept in the expression)
  f32x4_t rv[2][MI][2];
  auto loadg = [&](int q, int slot) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      const f32x4_t* rp = (const f32x4_t*)(p.x + (long)(m0 + (wave * MI + mi) * 16 + frow) * p.ldx + q * 32 + fq * 8);
      rv[slot][mi][0] = rp[0]; rv[slot][mi][1] = rp[1];
    }
  };
  loadg(0, 0);
#pragma unroll
  for (int q = 0; q < NG; ++q) {
    if (q + 1 < NG) loadg(q + 1, (q + 1) & 1);
    const f32x4_t* sb = (const f32x4_t*)(sb2 + q * 32 + fq * 8);
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      f32x4_t v[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) v[h] = acc2[mi][2 * q + h] * alpha2_v + sb[h] + brow;
      v[0] += rv[q & 1][mi][0]; v[1] += rv[q & 1][mi][1];
      float* dst = p.out + (long)(m0 + (wave * MI + mi) * 16 + frow) * p.ldo + q * 32 + fq * 8;
      ((f32x4_t*)dst)[0] = v[0]; ((f32x4_t*)dst)[1] = v[1];
    }
  }
}

template <int NWM, int NWN, int MI, int NI, int NSTAGE, int BK = 64, int KS = 1>
int launch_cfg(Params& p, int out_dtype, int batch, hipStream_t stream) {
  constexpr int BM = NWM * MI * 16, BN = NWN * NI * 16;
  // (+ BM * 8: a tail no kernel reads any more — it held a row's (mean, rstd) for the retired LayerNorm fold.  It stays
  //  because it is part of the footprint every tile was measured and tuned with: without it a fifth 64 x 64 x 2-stage
  //  block fits a CU's 160 KiB of LDS, and a change of residency is one to measure, not to slip in.)
  constexpr int SH_STAGES = NSTAGE * (BM + BN) * BK * 2 + BM * 8;
  constexpr int SH_RED = KS == 2 ? NWM * NWN * MI * NI * 1024 : 0;     // K-split: one group's accumulators
  constexpr int SHMEM = SH_STAGES > SH_RED ? SH_STAGES : SH_RED;
  if (p.K % BK != 0) return ODIC_EINVAL;
  const int max_rect = tile_grid(p.grid, p.M, p.N, BM, BN, (double)p.M * p.K * 2.0, (double)p.N * p.K * 2.0,
                                 32 * (NWM * NWN * KS <= 4 ? 2 : 1));
  dim3 grid(8 * max_rect, 1, batch), block(64 * NWM * NWN * KS);
  constexpr auto kb = gemm_bf16_nt_kernel<NWM, NWN, MI, NI, NSTAGE, BK, bf16_raw, KS>;
  constexpr auto kf = gemm_bf16_nt_kernel<NWM, NWN, MI, NI, NSTAGE, BK, float, KS>;
  tile_allow_lds<SHMEM, kb, kf>();
  if (out_dtype == ODIC_BF16) hipLaunchKernelGGL(kb, grid, block, SHMEM, stream, p);
  else hipLaunchKernelGGL(kf, grid, block, SHMEM, stream, p);
  return odic_launch_status();
}

// This file carries the tile configurations the host's tuner chooses from (0, 1, 7, 10, 40-42, 50-53), the one the
// built-in model falls back to (2) and the variants kept beside them (43-49).  Everything else that was built and
// measured on the way — more stages, 16-wave and 4-wave 256-wide tiles, out-of-phase residents, the persistent and
// the 256x256 phase-pipelined kernels, the LayerNorm fold across two products — lost every comparison and is gone;
// DESIGN.md §4.1 / §4.4 / §5 keep the measurements and name the last commit that has the code.

}  // namespace

int odic_gemm_bf16_launch(const odic_gemm_args* a, hipStream_t stream) {
  if (a->ln_colsum) return ODIC_EUNSUPPORTED;                          // (the in-kernel moments form is fp32 skinny only)
  if (a->K % 64 != 0 || (a->A && a->lda % 8 != 0) || a->ldw % 8 != 0) return ODIC_EINVAL;
  if (((uintptr_t)a->A & 15) || ((uintptr_t)a->W & 15)) return ODIC_EINVAL;
  if (a->a_ln && (a->tile_cfg < 50 || a->tile_cfg > 53)) return ODIC_EUNSUPPORTED;   // (A-resident kernels only)
  if (!a->a_ln && !a->A) return ODIC_EINVAL;
  if ((a->strideA % 8) || (a->strideW % 8)) return ODIC_EINVAL;
  Params p;
  p.A = (const bf16_raw*)a->A; p.W = (const bf16_raw*)a->W; p.bias = a->bias; p.residual = a->residual;
  p.out = a->out; p.M = a->M; p.N = a->N; p.K = a->K;
  p.lda = a->lda; p.ldw = a->ldw; p.ldr = a->ldr; p.ldc = a->ldc;
  p.strideA = a->strideA; p.strideW = a->strideW; p.strideBias = a->strideBias;
  p.strideR = a->strideR; p.strideC = a->strideC;
  p.alpha = a->alpha; p.act = a->act; p.bias_axis = a->bias_axis;
  p.a_ln = a->a_ln; p.ld_aln = a->ld_aln; p.ln_eps = a->ln_eps;
  // Tile choice = fewest "rounds x per-tile cost": a launch runs in ceil(tiles / resident slots)
  // rounds (256 CUs x 3 / 2 / 1 blocks for the 128x64 / 128x128 / 256x256 tiles, set by their LDS
  // footprints); relative per-tile costs 1 : 1.38 : 2.6 were measured on MI355X over the Swin-L
  // shapes (tools/gemm_tune.py; profiles/r01_gemm_tile_sweep.txt).
  int cfg = a->tile_cfg;
  if (cfg < 0) {
    const double c0 = tile_rounds(a->M, a->N, a->batch, 128, 64, 768) * 1.0;
    const double c1 = tile_rounds(a->M, a->N, a->batch, 128, 128, 512) * 1.38;
    const double c2 = a->N % 256 == 0 ? tile_rounds(a->M, a->N, a->batch, 256, 256, 256) * 2.6 : 1e30;
    cfg = (c0 <= c1 && c0 <= c2) ? 0 : (c1 <= c2 ? 1 : 2);
  }
  switch (cfg) {
    case 0: return launch_cfg<2, 2, 4, 2, 2>(p, a->out_dtype, a->batch, stream);     // 128 x 64, 2 stages
    case 1: return launch_cfg<2, 2, 4, 4, 2>(p, a->out_dtype, a->batch, stream);     // 128 x 128
    case 2: return launch_cfg<2, 4, 8, 4, 2>(p, a->out_dtype, a->batch, stream);     // 256 x 256
    case 7: return launch_cfg<4, 2, 4, 4, 2, 32>(p, a->out_dtype, a->batch, stream); // 256 x 128 x 32 (48 KiB)
    case 10: return launch_cfg<4, 2, 4, 4, 3, 32>(p, a->out_dtype, a->batch, stream); // 256 x 128 x 32, 3 stages (72 KiB)
    // 144- / 288-row tiles of 48 x 96 wave patches (MI = 3, NI = 6): the Swin-L token counts carry factors of 9
    // (9216 = 32·288, 2304 = 16·144), so these tile grids are exact multiples of the 256 compute units where the
    // power-of-two tiles leave a ragged last round (9216 x 3072: 512 tiles of 288 x 192 = two full rounds of one
    // 12-wave block per CU, against 1.69 rounds of 256 x 128).  One block per CU; the fill traffic per MFMA is a
    // quarter below the 256 x 128 tile's.
    case 40: return launch_cfg<6, 2, 3, 6, 2, 64>(p, a->out_dtype, a->batch, stream);  // 288 x 192, 12 waves (120 KiB)
    case 41: return launch_cfg<3, 3, 3, 6, 2, 64>(p, a->out_dtype, a->batch, stream);  // 144 x 288,  9 waves (108 KiB)
    case 42: return launch_cfg<3, 2, 3, 6, 2, 64>(p, a->out_dtype, a->batch, stream);  // 144 x 192,  6 waves, 2 stages (84 KiB)
    case 43: return launch_cfg<3, 2, 3, 6, 3, 64>(p, a->out_dtype, a->batch, stream);  // 144 x 192,  6 waves, 3 stages (126 KiB)
    case 44: return launch_cfg<3, 1, 3, 6, 2, 64>(p, a->out_dtype, a->batch, stream);  // 144 x 96,   3 waves, 2 stages (60 KiB)
    case 45: return launch_cfg<3, 3, 3, 6, 3, 32>(p, a->out_dtype, a->batch, stream);  // 144 x 288 x 32, 9 waves, 3 stages (81 KiB)
    case 46: return launch_cfg<3, 1, 3, 6, 3, 64>(p, a->out_dtype, a->batch, stream);  // 144 x 96,   3 waves, 3 stages (90 KiB)
    case 47: return launch_cfg<3, 2, 3, 6, 2, 64, 2>(p, a->out_dtype, a->batch, stream);  // 144 x 192, TWO K groups of 6 waves (108 KiB)
    // 64 x 64 tiles (4 waves of 32 x 32): the expansion encoder's products are 2304 rows (or 16 batches of 144) by 512 columns —
    // 72 tiles of 128 x 128 leave 184 of the 256 CUs idle while each tile walks a K of 512 ... 2048 alone
    case 48: return launch_cfg<2, 2, 2, 2, 3, 64>(p, a->out_dtype, a->batch, stream);  // 64 x 64, 3 stages (48 KiB)
    case 49: return launch_cfg<2, 2, 2, 2, 2, 64>(p, a->out_dtype, a->batch, stream);  // 64 x 64, 2 stages (32 KiB)
    // A-resident streaming kernels for K = 192 / 384 (whole tiles only; see gemm_bf16_apanel_kernel)
    case 50: return launch_apanel<4, 4, 3>(p, a->out_dtype, a->batch, stream);  // K = 192: 256-row panels, 64-column chunks
    case 51: return launch_apanel<2, 2, 6>(p, a->out_dtype, a->batch, stream);  // K = 384: 128-row panels, 32-column chunks
    case 52: return launch_apanel<2, 4, 3>(p, a->out_dtype, a->batch, stream);  // K = 192: 128-row panels, 64-column chunks
    case 53: return launch_apanel<2, 4, 6, 2>(p, a->out_dtype, a->batch, stream);  // K = 384: 128-row panels, 64-column chunks in two K pieces
    default: return ODIC_EINVAL;
  }
}

/* x + fc2(GELU(fc1(LN0(x)))) of one Swin block in one launch (stage width 192; see swin_mlp_kernel). */
extern "C" int odic_swin_mlp(const float* x, int64_t ldx, const void* w1_folded, const float* b1_folded, const void* w2,
                             const float* b2, float alpha2, float* out, int64_t ldo, int32_t M, int32_t C, float ln_eps,
                             void* stream) {
  if (!x || !w1_folded || !b1_folded || !w2 || !b2 || !out) return ODIC_ENULL;
  constexpr int MI = 2, BM = 4 * MI * 16;
  if (C != 192 || M <= 0 || M % BM != 0) return ODIC_EINVAL;
  if (ldx < C || ldo < C || (ldx & 3) || (ldo & 3)) return ODIC_EINVAL;
  if (((uintptr_t)x & 15) || ((uintptr_t)out & 15) || ((uintptr_t)w1_folded & 15) || ((uintptr_t)w2 & 15)) return ODIC_EINVAL;
  MlpParams p;
  p.x = x; p.out = out; p.W1 = (const bf16_raw*)w1_folded; p.b1 = b1_folded; p.W2 = (const bf16_raw*)w2; p.b2 = b2;
  p.ldx = ldx; p.ldo = ldo; p.M = M;
  p.alpha1 = 1.0f; p.alpha2 = alpha2; p.ln_eps = ln_eps;
  const int SHMEM = 2 * 64 * C * 2 + 5 * C * 4;          // W1 chunk + W2 chunk + the two bias vectors
  hipLaunchKernelGGL((swin_mlp_kernel<MI, 3>), dim3(M / BM), dim3(256), SHMEM, (hipStream_t)stream, p);
  return odic_launch_status();
}
