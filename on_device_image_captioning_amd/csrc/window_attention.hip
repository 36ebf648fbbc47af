// Swin (shifted-)window attention core for gfx950 — SURVEY §8 row A4.
//
// One workgroup per (window, head): softmax(q·kᵀ·scale + rel_pos_bias + sw_mask)·v for the N = ws²
// (= 144) tokens of one window and one 32-wide head.  The cyclic shift, window_partition,
// window_reverse and reverse shift of the reference (swin_transformer_mod.py:312-334) are pure
// index maps, so they are folded into the q/k/v gathers and the output scatter: the kernel reads
// the token-major qkv buffer [B·L, 3C] and writes the token-major attention output [B·L, C].
// The relative-position index (:163-173) and the SW-MSA mask (:281-297) are recomputed from token
// coordinates; only the (2ws-1)² x heads bias table is read.
//
// Roofline: per (window, head) 2,654,208 FLOP against 36,864 B (bf16) / 73,728 B (fp32) of
// compulsory q,k,v,out traffic → AI 72 / 36 FLOP/B, far left of the ridge: HBM-bound.
//
// All MFMA kernels: 3 waves per (window, head) (the fused one: 9 per window); a wave owns 16-query tiles.
// Sᵀ = K·Qᵀ by v_mfma_f32_16x16x32 (head dim 32 = exactly one MFMA per 16x16 score tile), so each
// lane holds, for ITS query (lane&15), keys 16kt+4(lane>>4)+{0..3} of all 9 key tiles: the row
// softmax is 36 in-register values + 2 shuffle steps.  Those registers are already the B operand
// of Oᵀ = Vᵀ·Pᵀ (K index = key, permuted consistently on both operands), so P never touches LDS.
//
// Six kernels:
//   window_attention_f32_kernel       parity path: one thread per query row, K/V fp32 in LDS (broadcast reads),
//                                     scores recomputed in two passes (max, then exp/sum/PV) — plain fp32 FMA chains.
//   window_attention_bf16_kernel      bf16, bias from the (2ws-1)² table (what a NULL packed bias selects): K row-major,
//                                     V transposed by the staging stores, Q straight into MFMA fragments.
//   window_attention_bf16_v3_kernel   bf16 / fp16 with the packed bias: the tuned core ("the v3 core" below).
//   swin_qkv_attention_kernel         norm1 → qkv → core in one launch for the width-192 stage.
//   swin_qkv_attention_tiled_kernel   qkv → core in one launch for the wider stages: the tiled GEMM's 144 x 288 tile as (window, 3 heads).
//   window_attention_h2_kernel        split-fp16 (hi + lo) activations, three MFMAs per contraction.
// All but the first two run the same core ("the v3 core"): K row-major and chunk-swizzled, V row-major, zero-padded to 160 keys
// and read through ds_read_b64_tr_b16.  Shared helpers: window geometry, the slot → token map, the rows[] / rids[] fill,
// the zeroed padding keys, the bias-initialised accumulators, the score MFMAs, the row max and the output store.  Block
// map, bias staging, key-quad offsets, bias origin, V-fragment offset, mask, softmax and P·V are still text in each of
// them: as helpers each compiles to another instruction stream (profiles/r09_window_attention_core_bench.txt).
#include "gemm_tile.h"        // gptr_t / lptr_t, wperm

namespace {

constexpr int HD = 32;        // head dim of every Swin-L stage
constexpr int MAXN = 144;     // ws*ws upper bound

struct WinGeom {
  int B, res, C, heads, ws, shift, nwin_side;
  float scale;
};
struct WinParams {
  const void* qkv; const float* table; const float* bias_shifted; void* out;
  WinGeom g;
};

// window `win` of the launch: image b, window (wy, wx) of its grid
struct Window { int b, wy, wx; };
__device__ __forceinline__ Window window_of(const WinGeom& g, int win) {
  const int wpi = g.nwin_side * g.nwin_side;
  const int b = win / wpi, wrem = win - b * wpi;
  const int wy = wrem / g.nwin_side, wx = wrem - wy * g.nwin_side;
  return {b, wy, wx};
}
// the window touches the seam of the shifted grid: some of its key / query pairs lie in different regions
__device__ __forceinline__ bool on_shift_seam(const WinGeom& g, const Window& w) {
  return g.shift > 0 && (w.wy == g.nwin_side - 1 || w.wx == g.nwin_side - 1);
}

// token index (row of the [B*L, *] buffers) of slot n of window w, and the region id of that slot on
// the shifted grid (0..8; all equal when shift == 0)
__device__ __forceinline__ void slot_to_token(const WinGeom& g, const Window& w, int n, long& row, int& rid) {
  const int ny = n / g.ws, nx = n - ny * g.ws;
  const int sy = w.wy * g.ws + ny, sx = w.wx * g.ws + nx;      // coords on the shifted grid
  int y = sy + g.shift, x = sx + g.shift;                     // roll(-shift): shifted[p] = x[p+shift]
  if (y >= g.res) y -= g.res;
  if (x >= g.res) x -= g.res;
  row = ((long)w.b * g.res + y) * g.res + x;
  if (g.shift > 0) {
    const int ey = sy < g.res - g.ws ? 0 : (sy < g.res - g.shift ? 1 : 2);
    const int ex = sx < g.res - g.ws ? 0 : (sx < g.res - g.shift ? 1 : 2);
    rid = ey * 3 + ex;
  } else {
    rid = 0;
  }
}

// =================================================================================================
// fp32 parity kernel
// =================================================================================================
__global__ __launch_bounds__(192) void window_attention_f32_kernel(WinParams p) {
  __shared__ __attribute__((aligned(16))) float Ks[MAXN][HD];
  __shared__ __attribute__((aligned(16))) float Vs[MAXN][HD];
  __shared__ float tab[23 * 23];
  __shared__ int rids[MAXN];
  __shared__ long rows[MAXN];

  const int N = p.g.ws * p.g.ws;
  const int head = blockIdx.y;
  const Window w = window_of(p.g, blockIdx.x);
  const int tid = threadIdx.x;
  const float* qkv = (const float*)p.qkv;
  const int ld = 3 * p.g.C;
  const int ntab = (2 * p.g.ws - 1) * (2 * p.g.ws - 1);

  for (int i = tid; i < ntab; i += blockDim.x) tab[i] = p.table[(long)i * p.g.heads + head];
  if (tid < N) {
    long r; int rid;
    slot_to_token(p.g, w, tid, r, rid);
    rows[tid] = r; rids[tid] = rid;
  }
  __syncthreads();
  // stage K and V: N rows x 32 floats = 8 float4 per row
  for (int i = tid; i < N * 8; i += blockDim.x) {
    const int n = i >> 3, c = (i & 7) * 4;
    const float* src = qkv + rows[n] * ld + head * HD + c;
    *(float4*)&Ks[n][c] = *(const float4*)(src + p.g.C);
    *(float4*)&Vs[n][c] = *(const float4*)(src + 2 * p.g.C);
  }
  __syncthreads();
  if (tid >= N) return;

  float q[HD];
  {
    const float* src = qkv + rows[tid] * ld + head * HD;
#pragma unroll
    for (int c = 0; c < HD; c += 4) {
      const float4 t = *(const float4*)(src + c);
      q[c] = t.x * p.g.scale; q[c + 1] = t.y * p.g.scale; q[c + 2] = t.z * p.g.scale; q[c + 3] = t.w * p.g.scale;
    }
  }
  const int iy = tid / p.g.ws, ix = tid - iy * p.g.ws;
  const int my_rid = rids[tid];
  const int tw = 2 * p.g.ws - 1;
  const int ibase = (iy + p.g.ws - 1) * tw + (ix + p.g.ws - 1);

  auto score = [&](int j, int jy, int jx) -> float {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < HD; ++c) s = fmaf(q[c], Ks[j][c], s);
    s += tab[ibase - jy * tw - jx];
    if (rids[j] != my_rid) s += -100.0f;
    return s;
  };

  float m = -INFINITY;
  for (int j = 0, jy = 0, jx = 0; j < N; ++j) {
    m = fmaxf(m, score(j, jy, jx));
    if (++jx == p.g.ws) { jx = 0; ++jy; }
  }
  float l = 0.f, o[HD];
#pragma unroll
  for (int c = 0; c < HD; ++c) o[c] = 0.f;
  for (int j = 0, jy = 0, jx = 0; j < N; ++j) {
    const float pj = expf(score(j, jy, jx) - m);
    l += pj;
#pragma unroll
    for (int c = 0; c < HD; ++c) o[c] = fmaf(pj, Vs[j][c], o[c]);
    if (++jx == p.g.ws) { jx = 0; ++jy; }
  }
  const float inv = 1.0f / l;
  float* dst = (float*)p.out + rows[tid] * p.g.C + head * HD;
#pragma unroll
  for (int c = 0; c < HD; c += 4)
    *(float4*)(dst + c) = make_float4(o[c] * inv, o[c + 1] * inv, o[c + 2] * inv, o[c + 3] * inv);
}

// =================================================================================================
// bf16 MFMA kernel
// =================================================================================================
constexpr int VT_LD = 164;    // keys per transposed-V row (160 used + 4 pad → 328-byte rows, 8-B aligned)

__global__ __launch_bounds__(192, 2) void window_attention_bf16_kernel(WinParams p) {
  __shared__ __attribute__((aligned(16))) bf16_raw Ks[MAXN][HD];       // 9216 B, row-major keys
  __shared__ __attribute__((aligned(16))) bf16_raw Vt[HD][VT_LD];      // 10496 B, [d][key]
  __shared__ float tab[23 * 23];
  __shared__ int rids[MAXN];
  __shared__ long rows[MAXN];

  const int head = blockIdx.y;
  const Window w = window_of(p.g, blockIdx.x);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bf16_raw* qkv = (const bf16_raw*)p.qkv;
  const int ld = 3 * p.g.C;

  for (int i = tid; i < 23 * 23; i += 192) tab[i] = p.table[(long)i * p.g.heads + head];
  if (tid < MAXN) {
    long r; int rid;
    slot_to_token(p.g, w, tid, r, rid);
    rows[tid] = r; rids[tid] = rid;
  }
  // zero the padded key columns 144..163 of Vᵀ (they meet P = 0, but 0·NaN garbage would poison O)
  for (int i = tid; i < HD * (VT_LD - MAXN); i += 192) {
    const int d = i / (VT_LD - MAXN), kk = i - d * (VT_LD - MAXN);
    Vt[d][MAXN + kk] = 0;
  }
  __syncthreads();

  // ---- stage K (row-major) and V (transposed): 144 rows x 4 chunks of 8 bf16
  for (int i = tid; i < MAXN * 4; i += 192) {
    const int n = i >> 2, c = (i & 3) * 8;
    const bf16_raw* src = qkv + rows[n] * ld + head * HD + c;
    *(bf16x8_t*)&Ks[n][c] = *(const bf16x8_t*)(src + p.g.C);
    const bf16x8_t v = *(const bf16x8_t*)(src + 2 * p.g.C);
#pragma unroll
    for (int e = 0; e < 8; ++e) Vt[c + e][n] = (bf16_raw)v[e];
  }

  // ---- Q fragments straight from global: B operand of Sᵀ = K·Qᵀ is Q[query = lane&15][d = 8(lane>>4)+j]
  const int fr = lane & 15, fq = lane >> 4;
  bf16x8_t qf[3];
#pragma unroll
  for (int qt = 0; qt < 3; ++qt) {
    const int qn = (wave * 3 + qt) * 16 + fr;
    qf[qt] = *(const bf16x8_t*)(qkv + rows[qn] * ld + head * HD + fq * 8);
  }
  __syncthreads();

  // ---- scores: acc[qt][kt][j] = S[query (3w+qt)*16 + fr][key 16kt + 4fq + j]
  f32x4_t sc[3][9];
#pragma unroll
  for (int kt = 0; kt < 9; ++kt) {
    const bf16x8_t kf = *(const bf16x8_t*)&Ks[kt * 16 + fr][fq * 8];
#pragma unroll
    for (int qt = 0; qt < 3; ++qt)
      sc[qt][kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[qt], f32x4_t{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
  }

  // ---- scale + relative-position bias + shift mask, row softmax (per query = per lane&15 column)
  const int tw = 23;
  float inv_l[3];
#pragma unroll
  for (int qt = 0; qt < 3; ++qt) {
    const int qn = (wave * 3 + qt) * 16 + fr;
    const int iy = qn / 12, ix = qn - iy * 12;
    const int ibase = (iy + 11) * tw + (ix + 11);
    const int my_rid = rids[qn];
    float m = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 9; ++kt) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int key = kt * 16 + fq * 4 + j;
        const int jy = key / 12, jx = key - jy * 12;
        float s = sc[qt][kt][j] * p.g.scale + tab[ibase - jy * tw - jx];
        if (rids[key] != my_rid) s += -100.0f;
        sc[qt][kt][j] = s;
        m = fmaxf(m, s);
      }
    }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    float l = 0.f;
#pragma unroll
    for (int kt = 0; kt < 9; ++kt) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float e = __expf(sc[qt][kt][j] - m);
        sc[qt][kt][j] = e;
        l += e;
      }
    }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    inv_l[qt] = 1.0f / l;
  }

  // ---- Oᵀ = Vᵀ·Pᵀ : A = Vᵀ[d = 16nt + fr][k-slot], B = Pᵀ[k-slot][query = fr]
  //      k-slot (fq, e) of K-step s  ↔  key 32s + 16(e>>2) + 4fq + (e&3)   (same map on both operands)
  f32x4_t oacc[3][2];
#pragma unroll
  for (int qt = 0; qt < 3; ++qt) { oacc[qt][0] = f32x4_t{0.f, 0.f, 0.f, 0.f}; oacc[qt][1] = f32x4_t{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
  for (int s = 0; s < 5; ++s) {
    bf16x8_t vf[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const bf16x4_t lo = *(const bf16x4_t*)&Vt[nt * 16 + fr][32 * s + 4 * fq];
      const bf16x4_t hi = *(const bf16x4_t*)&Vt[nt * 16 + fr][32 * s + 16 + 4 * fq];
      vf[nt] = bf16x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    }
#pragma unroll
    for (int qt = 0; qt < 3; ++qt) {
      bf16x8_t pf;
#pragma unroll
      for (int e = 0; e < 4; ++e) pf[e] = (short)f32_to_bf16(sc[qt][2 * s][e]);
      if (s < 4) {
#pragma unroll
        for (int e = 0; e < 4; ++e) pf[4 + e] = (short)f32_to_bf16(sc[qt][2 * s + 1][e]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) pf[4 + e] = 0;
      }
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
        oacc[qt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[nt], pf, oacc[qt][nt], 0, 0, 0);
    }
  }

  // ---- store: lane holds O[query = fr][d = 16nt + 4fq + {0..3}] → 8-byte stores
  bf16_raw* out = (bf16_raw*)p.out;
#pragma unroll
  for (int qt = 0; qt < 3; ++qt) {
    const int qn = (wave * 3 + qt) * 16 + fr;
    bf16_raw* dst = out + rows[qn] * p.g.C + head * HD + fq * 4;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      ushort4 pk;
      pk.x = f32_to_bf16(oacc[qt][nt][0] * inv_l[qt]);
      pk.y = f32_to_bf16(oacc[qt][nt][1] * inv_l[qt]);
      pk.z = f32_to_bf16(oacc[qt][nt][2] * inv_l[qt]);
      pk.w = f32_to_bf16(oacc[qt][nt][3] * inv_l[qt]);
      *(ushort4*)(dst + nt * 16) = pk;
    }
  }
}


// =================================================================================================
// bf16 MFMA kernel, v3 (used when the caller supplies the packed bias).  The kernel is VALU-issue- and
// latency-bound (36 scores per lane and query tile: v_exp_f32 alone is 144 of ~250 issue slots), so everything
// around the exponentials is squeezed:
//   * K and V are gathered straight into LDS by LDS-DMA (global_load_lds_dwordx4: per-lane source address = the
//     window's token row, lane-linear destination = row-major [144][32]); no VGPR round trip and no transposing
//     stores: V is consumed through ds_read_b64_tr_b16.  The 16-byte chunks of a K row are XOR-swizzled with
//     (row >> 2) & 3 (on the DMA source address and again on the fragment read): the ds_read_b128 of a K
//     fragment then spreads a 16-lane service group over all 16 slots of the 256-byte bank row (it was 2-way).
//   * the relative-position bias is the ACCUMULATOR INIT of the score MFMA and comes from LDS, not from HBM/L2:
//     for a query (iy, ix) the four keys 16kt + 4fq .. +3 of an accumulator register quad lie in ONE window row
//     (12 = 3 x 4), so their biases are four CONSECUTIVE entries of the (2ws-1)² table once its x axis is
//     reversed: R[r][c'] = table[r][22 - c'], r = iy - jy + 11, c' = 11 - ix + jx.  With rows padded to 24 the
//     quad starts at r·24 + 11 - ix + jx0, whose alignment mod 4 depends on the query only (jx0 ∈ {0,4,8}), so
//     the host packs FOUR copies of R shifted by 0..3 floats (per head 9 KiB, pre-divided by `scale`) and one
//     aligned ds_read_b128 per quad — from the copy (11 - ix) & 3 — lands the bias in the accumulator.  The
//     dense [144,144] fp32 bias of v2 cost 83 KB of L2→CU traffic per (window, head) against 37 KB of q/k/v/o;
//     this costs 9 KiB once per block (LDS-DMA) and one integer add per quad.
//   * softmax in base 2 on the raw accumulators: row max by v_max3_f32, then ONE packed FMA per score pair
//     (acc·scale·log2e − max·scale·log2e) feeding v_exp_f32; row sums by packed adds; P is rounded to bf16 pairs
//     as it is produced (18 registers).
//   * the SW-MSA mask costs nothing on interior windows (wave-uniform branch); edge windows compare 4 packed
//     region ids per LDS word.
// =================================================================================================
typedef __attribute__((ext_vector_type(4))) short v4s_t;
typedef __attribute__((ext_vector_type(2))) float f32x2_t;

constexpr int BS_COPY = 576;          // floats per shifted bias copy (23 rows x 24 + slack; 4 copies = 9 x 1 KiB)

__device__ __forceinline__ float max3f(float a, float b, float c) {      // inputs are MFMA results: canonical
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

// 16-bit element flavour of the fast kernel: bf16 (the default backbone mode) or IEEE fp16 (the low-precision mode's
// activations, BASELINE.json configs[4]); same MFMA shape, same fragment layouts, same LDS image.
template <bool F16> __device__ __forceinline__ f32x4_t mfma16(bf16x8_t a, bf16x8_t b, f32x4_t c) {
  if constexpr (F16)
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
template <bool F16> __device__ __forceinline__ unsigned short cvt16(float f) {
  if constexpr (F16) { const _Float16 h = (_Float16)f; return __builtin_bit_cast(unsigned short, h); }
  else return f32_to_bf16(f);
}

// ------------------------------------------------------------------------------------------------- the v3 core
// Pieces of the core shared by window_attention_bf16_v3_kernel<F16>, swin_qkv_attention_kernel,
// swin_qkv_attention_tiled_kernel and window_attention_h2_kernel.  Lane (fr, fq) = (lane & 15, lane >> 4) holds, for query fr of its tile, keys
// 16kt + 4fq + {0..3} of the nine key tiles in sc[9].  Only helpers that leave every kernel's instruction stream as it was
// are here.  The block map, bias staging, key-quad offsets, bias origin, V-fragment offset, mask, softmax and P·V were each
// shown to change it and stay as text in each kernel until they are timed on the device
// (profiles/r09_window_attention_core_bench.txt).

// token rows and packed region ids of the window's 144 slots (one thread each)
__device__ __forceinline__ void stage_rows(const WinGeom& g, const Window& w, int tid, int* rows, unsigned char* rids) {
  if (tid < MAXN) {
    long r; int rid;
    slot_to_token(g, w, tid, r, rid);
    rows[tid] = (int)r; rids[tid] = (unsigned char)rid;
  }
}

// rows 144..159 of a [160][32] V image: the padding keys of the fifth P·V step meet P = 0, but must not be NaN garbage
__device__ __forceinline__ void zero_padding_keys(void* V, int tid) {
  if (tid < 128) ((unsigned long long*)((char*)V + MAXN * HD * 2))[tid] = 0ull;      // 16 x 64 B
}

// The K / V / bias fragment addresses are made opaque once per tile: otherwise hipcc hoists the loop-invariant LDS
// reads out of the tile loop and parks dozens of registers on them.
__device__ __forceinline__ void opaque_offsets(int& k, int& v, int& b) { asm volatile("" : "+v"(k), "+v"(v), "+v"(b)); }

// the relative-position bias (pre-divided by scale) as the accumulator init of the score MFMAs
__device__ __forceinline__ void load_bias36(const char* bbase, const int (&koffs)[9], f32x4_t (&sc)[9]) {
#pragma unroll
  for (int kt = 0; kt < 9; ++kt) sc[kt] = *(const f32x4_t*)(bbase + koffs[kt]);
}

// Sᵀ = K·Qᵀ on top of the bias: kbase = this lane's fragment of key row fr in the chunk-swizzled [144][32] K image
template <bool F16> __device__ __forceinline__ void scores16(const char* kbase, bf16x8_t q, f32x4_t (&sc)[9]) {
#pragma unroll
  for (int kt = 0; kt < 9; ++kt) {
    const bf16x8_t kf = *(const bf16x8_t*)(kbase + kt * 16 * HD * 2);
    sc[kt] = mfma16<F16>(kf, q, sc[kt]);
  }
}

// row max of the query's 144 raw scores: 18 v_max3_f32 over the lane's 36, two shuffles across the fq groups
__device__ __forceinline__ float row_max36(const f32x4_t (&sc)[9]) {
  float m = max3f(sc[0][0], sc[0][1], sc[0][2]);
  m = max3f(m, sc[0][3], sc[1][0]);
  m = max3f(m, sc[1][1], sc[1][2]);
#pragma unroll
  for (int kt = 2; kt < 9; kt += 2) {                                  // (sc[kt-1][3], sc[kt][0..3], sc[kt+1][0..2]) pairs
    m = max3f(m, sc[kt - 1][3], sc[kt][0]);
    m = max3f(m, sc[kt][1], sc[kt][2]);
    if (kt + 1 < 9) {
      m = max3f(m, sc[kt][3], sc[kt + 1][0]);
      m = max3f(m, sc[kt + 1][1], sc[kt + 1][2]);
    } else {
      m = fmaxf(m, sc[kt][3]);
    }
  }
  m = fmaxf(m, __shfl_xor(m, 16, 64));
  return fmaxf(m, __shfl_xor(m, 32, 64));
}

// lane holds O[query = fr][d = 16nt + 4fq + {0..3}] → two 8-byte stores; dst = the query's row + head·32 + 4fq
template <bool F16> __device__ __forceinline__ void store_o16(bf16_raw* dst, const f32x4_t (&oacc)[2], float inv_l) {
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    ushort4 o4;
    o4.x = cvt16<F16>(oacc[nt][0] * inv_l); o4.y = cvt16<F16>(oacc[nt][1] * inv_l);
    o4.z = cvt16<F16>(oacc[nt][2] * inv_l); o4.w = cvt16<F16>(oacc[nt][3] * inv_l);
    *(ushort4*)(dst + nt * 16) = o4;
  }
}

template <bool F16>
__global__ __launch_bounds__(192, 4) void window_attention_bf16_v3_kernel(WinParams p) {
  __shared__ __attribute__((aligned(16))) bf16_raw Ks[MAXN][HD];        // 9216 B (chunk-swizzled rows)
  __shared__ __attribute__((aligned(16))) bf16_raw Vs[MAXN + 16][HD];   // 10240 B (rows 144..159 zero)
  __shared__ __attribute__((aligned(16))) float Bs[4 * BS_COPY];        // 9216 B: 4 shifted copies of the bias table
  __shared__ int rows[MAXN];
  __shared__ __attribute__((aligned(4))) unsigned char rids[MAXN];

  // Block → (window, head): blocks b, b+8, ... share an XCD and its L2.  Each XCD walks its windows with
  // the HEAD index fastest, so the 64-byte q/k/v segments of neighbouring heads — two per 128-byte
  // line — are requested back-to-back from the same L2 and every HBM line is fetched once.
  ODIC_ENCODE_PRIO();
  const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
  const int head = idx % p.g.heads;
  const int win = (idx / p.g.heads) * 8 + xcd;
  if (win >= p.g.B * (p.g.nwin_side * p.g.nwin_side)) return;
  const Window w = window_of(p.g, win);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bf16_raw* qkv = (const bf16_raw*)p.qkv;
  const long ld = 3 * p.g.C;
  const bool masked = on_shift_seam(p.g, w);

  // bias copies of this head: 9 x 1 KiB of LDS-DMA, 3 per wave (independent of the token rows)
  {
    const float* bsrc = p.bias_shifted + (long)head * 4 * BS_COPY + lane * 4;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int blk = wave * 3 + i;
      __builtin_amdgcn_global_load_lds((gptr_t)(bsrc + blk * 256), (lptr_t)((char*)&Bs[0] + blk * 1024), 16, 0, 0);
    }
  }
  stage_rows(p.g, w, tid, rows, rids);
  zero_padding_keys(Vs, tid);
  __syncthreads();

  // ---- LDS-DMA gather: instruction i covers window slots 16i .. 16i+15 (16 rows x 64 B = 1 KiB)
  {
    const int r_in = lane >> 2, ch = lane & 3;
    const int chk = ch ^ ((r_in >> 2) & 3);                             // K: this LDS slot holds logical chunk chk
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int blk = wave * 3 + i;                                       // 0..8
      const bf16_raw* src = qkv + (long)rows[blk * 16 + r_in] * ld + head * HD;
      __builtin_amdgcn_global_load_lds((gptr_t)(src + p.g.C + chk * 8), (lptr_t)((char*)&Ks[0][0] + blk * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((gptr_t)(src + 2 * p.g.C + ch * 8), (lptr_t)((char*)&Vs[0][0] + blk * 1024), 16, 0, 0);
    }
  }
  const int fr = lane & 15, fq = lane >> 4;
  const float scale2 = p.g.scale * 1.4426950408889634f;
  const float mask_acc = 100.0f / p.g.scale;                              // -100 in accumulator units
  bf16_raw* out = (bf16_raw*)p.out;
  // transposed-read addresses of V: lane (fr = 4q+p) of 16-lane group fq supplies row r0+q, cols 4p..4p+3
  const int voff = ((4 * fq + (fr >> 2)) * HD + 4 * (fr & 3)) * 2;
  // byte offset of key quad (kt, fq) inside a bias copy, relative to the query's origin: (-jy·24 + jx0)·4
  int koffs[9];
#pragma unroll
  for (int kt = 0; kt < 9; ++kt) {
    const int key0 = kt * 16 + fq * 4;
    const int jy = key0 / 12, jx0 = key0 - jy * 12;
    koffs[kt] = (jx0 - jy * 24) * 4;
  }
  auto bias_base = [&](int qn) -> int {                                  // byte address of the query's origin in ITS copy
    const int iy = qn / 12, ix = qn - iy * 12;
    const int s = (11 - ix) & 3;
    return (s * BS_COPY + (iy + 11) * 24 + 11 - ix - s) * 4;
  };

  // first tile's Q fragment (B operand of Sᵀ = K·Qᵀ: Q[query = fr][d = 8·fq ..])
  bf16x8_t q = *(const bf16x8_t*)(qkv + (long)rows[wave * 48 + fr] * ld + head * HD + fq * 8);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

#pragma unroll
  for (int qt = 0; qt < 3; ++qt) {
    const int qn = (wave * 3 + qt) * 16 + fr;
    const int orow = rows[qn];
    int koff = (fr * HD + ((fq ^ ((fr >> 2) & 3)) * 8)) * 2, vo = voff, bb = bias_base(qn);
    opaque_offsets(koff, vo, bb);
    const char* kbase = (const char*)&Ks[0][0] + koff;
    const char* vbase = (const char*)&Vs[0][0] + vo;
    const char* bbase = (const char*)&Bs[0] + bb;
    f32x4_t sc[9];
    load_bias36(bbase, koffs, sc);
    scores16<F16>(kbase, q, sc);
    if (masked) {
      const unsigned my = rids[qn];
#pragma unroll
      for (int kt = 0; kt < 9; ++kt) {
        const unsigned kr = *(const unsigned*)&rids[kt * 16 + fq * 4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (((kr >> (8 * j)) & 0xff) != my) sc[kt][j] -= mask_acc;
      }
    }
    const float m = row_max36(sc);
    const f32x2_t s2 = {scale2, scale2};
    const f32x2_t c2 = {-m * scale2, -m * scale2};
    f32x2_t lsum = {0.f, 0.f};
    bf16x4_t pk[9];
#pragma unroll
    for (int kt = 0; kt < 9; ++kt) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const f32x2_t a = f32x2_t{sc[kt][2 * h], sc[kt][2 * h + 1]} * s2 + c2;
        const f32x2_t e = {__builtin_amdgcn_exp2f(a[0]), __builtin_amdgcn_exp2f(a[1])};
        lsum += e;
        pk[kt][2 * h] = (short)cvt16<F16>(e[0]);
        pk[kt][2 * h + 1] = (short)cvt16<F16>(e[1]);
      }
    }
    // request the next tile's Q under the P·V work below
    if (qt < 2) q = *(const bf16x8_t*)(qkv + (long)rows[qn + 16] * ld + head * HD + fq * 8);
    float l = lsum[0] + lsum[1];
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    const float inv_l = __builtin_amdgcn_rcpf(l);

    // Oᵀ = Vᵀ·Pᵀ : K-slot (fq, e) of step s ↔ key 32s + 16(e>>2) + 4fq + (e&3) on both operands
    f32x4_t oacc[2] = {f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int s5 = 0; s5 < 5; ++s5) {
      const bf16x4_t lo4 = pk[2 * s5];
      const bf16x4_t hi4 = s5 < 4 ? pk[2 * s5 + (s5 < 4)] : bf16x4_t{0, 0, 0, 0};
      const bf16x8_t pf = bf16x8_t{lo4[0], lo4[1], lo4[2], lo4[3], hi4[0], hi4[1], hi4[2], hi4[3]};
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const v4s_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) v4s_t*)(vbase + (32 * s5) * HD * 2 + nt * 32));
        const v4s_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) v4s_t*)(vbase + (32 * s5 + 16) * HD * 2 + nt * 32));
        const bf16x8_t vf = bf16x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        oacc[nt] = mfma16<F16>(vf, pf, oacc[nt]);
      }
    }
    store_o16<F16>(out + (long)orow * p.g.C + head * HD + fq * 4, oacc, inv_l);
  }
}


// =================================================================================================
// norm1 → qkv → attention core in ONE launch for the stage of width 192 (Swin-L stage 0): VERDICT r2 #5.
//
// Unfused, a stage-0 block at B = 16 writes 170 MB of qkv and reads it back (plus the 57 MB bf16 copy of the
// normalised rows): LayerNorm 37 µs + qkv product 56 µs + attention core 53 µs.  Here one block of NINE waves owns one
// window; wave w owns the window's tokens 16w .. 16w+15 for the whole launch:
//   * it reads its 16 fp32 rows of the residual stream ONCE, normalises them in registers (the row's 192 values sit in
//     the four fq lanes; gamma / beta are folded into W / bias by the caller) and keeps them as six MFMA B-operand
//     fragments — 24 registers, never in LDS (the A-resident GEMM's LayerNorm-while-reading form, gemm_bf16.hip);
//   * per head, the 96 W rows of that head's q / k / v channels (36 KiB, the tiled GEMM's swizzled sub-tile image, rows
//     permuted so that an accumulator pair is 8 adjacent channels) and the head's packed bias copies (9 KiB) arrive by
//     LDS-DMA one head ahead; 36 MFMAs give the wave q, k, v of its 16 tokens: q stays in registers — the accumulator
//     pair IS the Q fragment of the score MFMA — k and v go to the window's K / V images in LDS (16 bytes per lane);
//   * barrier, then the v3 core above on one query tile per wave (bias as accumulator init, base-2 softmax on the raw
//     accumulators, P·V through ds_read_b64_tr_b16), 8 bytes x 2 of output per lane;
//   * the counted wait in front of a head's first barrier is vmcnt(2): that head's DMA was issued BEFORE the previous
//     head's two stores (vmcnt retires in order), so the stores stay in flight.
// Bit-identical to LayerNorm-while-reading product + v3 core (same MFMAs in the same K order, the same roundings of
// q / k / v to bf16): tests/test_hip_ops.py::test_swin_qkv_attention_fused.
// =================================================================================================
struct FusedParams {
  const float* x; long ldx; const bf16_raw* W; const float* bqkv; const float* bias_shifted; bf16_raw* out;
  WinGeom g;
  float eps;
};

template <int KT>
__global__ __launch_bounds__(576, 1) void swin_qkv_attention_kernel(FusedParams p) {
  constexpr int C = KT * 64;
  constexpr int WSUB = 96 * 128;                            // one 64-deep sub-tile of a head's 96 W rows
  constexpr int WBUF = KT * WSUB;
  constexpr int NWV = 9;
  static_assert((WBUF / 1024) % NWV == 0, "a head's W image must split evenly over the nine waves");
  constexpr int WI = WBUF / 1024 / NWV;                     // W DMA instructions per wave and head
  extern __shared__ __attribute__((aligned(16))) char lds[];
  char* Wb = lds;                                                                    // 2 x WBUF
  char* Kp = lds + 2 * WBUF;                                                         // [144][32] bf16, chunk-swizzled
  char* Vp = Kp + MAXN * HD * 2;                                                     // [160][32] bf16 (rows 144.. zero)
  char* Bp = Vp + (MAXN + 16) * HD * 2;                                              // 2 x 4 bias copies
  float* sbq = (float*)(Bp + 2 * 4 * BS_COPY * 4);                                   // qkv bias, 3C floats
  int* rows = (int*)(sbq + 3 * C);
  unsigned char* rids = (unsigned char*)(rows + MAXN);

  ODIC_ENCODE_PRIO();
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const Window w = window_of(p.g, blockIdx.x);
  const bool masked = on_shift_seam(p.g, w);
  stage_rows(p.g, w, tid, rows, rids);
  zero_padding_keys(Vp, tid);
  for (int t = tid; t < 3 * C; t += 64 * NWV) sbq[t] = p.bqkv[t];

  // ---- per-head DMA: W rows (part, 32-row group permuted) as KT swizzled sub-tiles, then the head's bias copies
  int w_off[WI];
#pragma unroll
  for (int i = 0; i < WI; ++i) {
    const int j = i * NWV + wave, kt = j / 12, rg = j - kt * 12;
    const int srow = lane >> 3, r = rg * 8 + srow;
    w_off[i] = ((r >> 5) * C + wperm(r & 31)) * C + kt * 64 + ((lane & 7) ^ srow) * 8;
  }
  auto issue = [&](int h, int buf) {
    const bf16_raw* wb = p.W + (long)h * HD * C;
#pragma unroll
    for (int i = 0; i < WI; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(wb + w_off[i]), (lptr_t)(Wb + buf * WBUF + (i * NWV + wave) * 1024), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((gptr_t)(p.bias_shifted + (long)h * 4 * BS_COPY + wave * 256 + lane * 4),
                                     (lptr_t)(Bp + buf * 4 * BS_COPY * 4 + wave * 1024), 16, 0, 0);
  };
  issue(0, 0);
  __syncthreads();                                          // rows[] / rids / bias staged

  // ---- this wave's 16 tokens: LayerNorm in registers → six B-operand fragments (lane (fr, fq): row fr, k = 32kk + 8fq ..)
  const int slot = wave * 16 + fr;
  const int orow = rows[slot];
  bf16x8_t af[2 * KT];
  {
    const float* xr = p.x + (long)orow * p.ldx + fq * 8;
    f32x4_t xv[2 * KT][2];
#pragma unroll
    for (int k = 0; k < 2 * KT; ++k) { xv[k][0] = *(const f32x4_t*)(xr + k * 32); xv[k][1] = *(const f32x4_t*)(xr + k * 32 + 4); }
    f32x4_t s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 2 * KT; ++k) s4 += xv[k][0] + xv[k][1];
    float sum = (s4[0] + s4[1]) + (s4[2] + s4[3]);
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float mean = sum / (float)C;                // (as gemm_bf16.hip's LayerNorm-while-reading form: the two must agree bit for bit)
    f32x4_t q4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 2 * KT; ++k) {
      xv[k][0] -= mean; xv[k][1] -= mean;
      q4 += xv[k][0] * xv[k][0] + xv[k][1] * xv[k][1];
    }
    float ssq = (q4[0] + q4[1]) + (q4[2] + q4[3]);
    ssq += __shfl_xor(ssq, 16, 64);
    ssq += __shfl_xor(ssq, 32, 64);
    const float rstd = rsqrtf(ssq / (float)C + p.eps);
#pragma unroll
    for (int k = 0; k < 2 * KT; ++k) {
      bf16x8_t f;
#pragma unroll
      for (int e = 0; e < 4; ++e) { f[e] = (short)f32_to_bf16(xv[k][0][e] * rstd); f[4 + e] = (short)f32_to_bf16(xv[k][1][e] * rstd); }
      af[k] = f;
    }
  }

  const float scale2 = p.g.scale * 1.4426950408889634f;
  const float mask_acc = 100.0f / p.g.scale;
  const int voff = ((4 * fq + (fr >> 2)) * HD + 4 * (fr & 3)) * 2;
  int koffs[9];
#pragma unroll
  for (int kt = 0; kt < 9; ++kt) {
    const int key0 = kt * 16 + fq * 4;
    const int jy = key0 / 12, jx0 = key0 - jy * 12;
    koffs[kt] = (jx0 - jy * 24) * 4;
  }
  int bias_org;                                             // byte address of the query's origin in ITS bias copy
  {
    const int iy = slot / 12, ix = slot - iy * 12;
    const int sft = (11 - ix) & 3;
    bias_org = (sft * BS_COPY + (iy + 11) * 24 + 11 - ix - sft) * 4;
  }
  const unsigned my_rid = rids[slot];

  __builtin_amdgcn_s_waitcnt(0x0070);                       // vmcnt(0) lgkmcnt(0): x rows and head 0's DMA
  for (int h = 0; h < p.g.heads; ++h) {
    const int buf = h & 1;
    if (h) __builtin_amdgcn_s_waitcnt(0x0F72);              // vmcnt(2): this head's DMA landed, last head's stores may fly
    __builtin_amdgcn_s_barrier();                           // ... for every wave; everyone is done with K / V / the other buffers
    if (h + 1 < p.g.heads) issue(h + 1, buf ^ 1);

    // ---- q, k, v of this wave's tokens for head h: [96 channels] x [16 tokens], K = C
    f32x4_t acc[6];
#pragma unroll
    for (int t = 0; t < 6; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const char* lw = Wb + buf * WBUF + fr * 128;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int chunk = ((kk * 4 + fq) ^ (fr & 7)) << 4;
        bf16x8_t wf[6];
#pragma unroll
        for (int t = 0; t < 6; ++t) wf[t] = *(const bf16x8_t*)(lw + kt * WSUB + t * 16 * 128 + chunk);
#pragma unroll
        for (int t = 0; t < 6; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[t], af[2 * kt + kk], acc[t], 0, 0, 0);
      }
    }
    bf16x8_t qkv8[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      const f32x4_t* sb = (const f32x4_t*)(sbq + u * C + h * HD + fq * 8);
      const f32x4_t v0 = acc[2 * u] + sb[0], v1 = acc[2 * u + 1] + sb[1];
#pragma unroll
      for (int e = 0; e < 4; ++e) { qkv8[u][e] = (short)f32_to_bf16(v0[e]); qkv8[u][4 + e] = (short)f32_to_bf16(v1[e]); }
    }
    const bf16x8_t q = qkv8[0];
    *(bf16x8_t*)(Kp + slot * HD * 2 + ((fq ^ ((fr >> 2) & 3)) << 4)) = qkv8[1];
    *(bf16x8_t*)(Vp + slot * HD * 2 + (fq << 4)) = qkv8[2];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                           // the window's K / V of head h are complete

    // ---- the v3 core on this wave's query tile
    int koff = (fr * HD + ((fq ^ ((fr >> 2) & 3)) * 8)) * 2, vo = voff, bb = bias_org;
    opaque_offsets(koff, vo, bb);
    const char* kbase = Kp + koff;
    const char* vbase = Vp + vo;
    const char* bbase = Bp + buf * 4 * BS_COPY * 4 + bb;
    f32x4_t sc[9];
    load_bias36(bbase, koffs, sc);
    scores16<false>(kbase, q, sc);
    if (masked) {
#pragma unroll
      for (int kt = 0; kt < 9; ++kt) {
        const unsigned kr = *(const unsigned*)&rids[kt * 16 + fq * 4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (((kr >> (8 * j)) & 0xff) != my_rid) sc[kt][j] -= mask_acc;
      }
    }
    const float m = row_max36(sc);
    const f32x2_t s2 = {scale2, scale2};
    const f32x2_t c2 = {-m * scale2, -m * scale2};
    f32x2_t lsum = {0.f, 0.f};
    bf16x4_t pk[9];
#pragma unroll
    for (int kt = 0; kt < 9; ++kt) {
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const f32x2_t a = f32x2_t{sc[kt][2 * hh], sc[kt][2 * hh + 1]} * s2 + c2;
        const f32x2_t e = {__builtin_amdgcn_exp2f(a[0]), __builtin_amdgcn_exp2f(a[1])};
        lsum += e;
        pk[kt][2 * hh] = (short)f32_to_bf16(e[0]);
        pk[kt][2 * hh + 1] = (short)f32_to_bf16(e[1]);
      }
    }
    float l = lsum[0] + lsum[1];
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    const float inv_l = __builtin_amdgcn_rcpf(l);
    f32x4_t oacc[2] = {f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int s5 = 0; s5 < 5; ++s5) {
      const bf16x4_t lo4 = pk[2 * s5];
      const bf16x4_t hi4 = s5 < 4 ? pk[2 * s5 + (s5 < 4)] : bf16x4_t{0, 0, 0, 0};
      const bf16x8_t pf = bf16x8_t{lo4[0], lo4[1], lo4[2], lo4[3], hi4[0], hi4[1], hi4[2], hi4[3]};
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const v4s_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) v4s_t*)(vbase + (32 * s5) * HD * 2 + nt * 32));
        const v4s_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) v4s_t*)(vbase + (32 * s5 + 16) * HD * 2 + nt * 32));
        const bf16x8_t vf = bf16x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        oacc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, oacc[nt], 0, 0, 0);
      }
    }
    store_o16<false>(p.out + (long)orow * C + h * HD + fq * 4, oacc, inv_l);
  }
}


// =================================================================================================
// qkv product → attention core in ONE launch for the wide stages (C = 384 / 768 / 1536): the bf16 qkv tensor [B·L, 3C] —
// 42.5 MB at stage 2, B = 16 — is never written and never gathered back.
//
// The tile is the tiled GEMM's configuration 41 (gemm_bf16_nt_kernel<3,3,3,6,2,64>: 144 x 288, nine waves, two 54-KiB
// stages) read as a window: its 144 rows are the 144 tokens of ONE 12 x 12 window (the LDS-DMA source rows come from
// slot_to_token, cyclic shift included — nothing is permuted in memory), its 288 columns are q | k | v (32 channels each) of
// THREE heads.  Tile column j = LDS row j of the W image is wave column j / 96, part u = (j % 96) / 32, channel j % 32:
// source row u·C + (3·tn + wn)·32 + wperm(channel) of the unpacked qkv weight.  Wave (wm, wn) of the 3 x 3 grid leaves the
// K loop with q, k, v of head 3·tn + wn for the window's slots 48·wm .. 48·wm + 47, and with the swapped-operand layout a
// lane's accumulator pair (2u, 2u + 1) of row tile mi is slot 48·wm + 16·mi + frow, channels 8·fq .. 8·fq + 7 of part u:
// pair 0 IS the Q fragment of the score MFMA, pairs 1 and 2 are 16 bytes of the head's K and V images.
//   * the K loop is configuration 41's, statement for statement (two stages, BK = 64, vmcnt + raw s_barrier, the same
//     fragment reads and MFMA order): every accumulator is the chain the tiled GEMM computes for that element;
//   * under the LAST K-tile the three heads' packed bias copies (3 x 9 KiB) arrive by LDS-DMA in the stage buffer the loop
//     has finished with;
//   * after the loop: acc + bias rounded to bf16 (the tiled epilogue's acc·alpha + bias with alpha = 1: the bits of the
//     stored qkv tensor), barrier, K (chunk-swizzled) and V (+ zeroed padding keys) written over the stage buffers, barrier;
//   * each wave runs the v3 core on its three query tiles against its head's 144 keys.
// LDS after the loop: free stage = bias 3 x 9216 | K 3 x 9216 (= 55296, exactly one stage), other stage = V 3 x 10240;
// rows[] / rids[] live in the tail behind the stages (config 41's footprint, 111744 B, is kept).
// Grid: config 41's XCD rectangle walk with tile row = window, tile column = head group.
// Bit-identical to odic_gemm(tile_cfg 41) + odic_window_attention (bf16, packed bias):
// tests/test_swin_qkv_attention_tiled_gpu.py.
// =================================================================================================
struct TiledParams {
  const bf16_raw* A; const bf16_raw* W; const float* bqkv; const float* bias_shifted; bf16_raw* out;
  WinGeom g;
  TileGrid grid;
};

constexpr int QT_ROWB = 128, QT_A_BYTES = 144 * QT_ROWB, QT_W_BYTES = 288 * QT_ROWB, QT_STAGE = QT_A_BYTES + QT_W_BYTES;
constexpr int QT_KIMG = MAXN * HD * 2, QT_VIMG = (MAXN + 16) * HD * 2, QT_BIMG = 4 * BS_COPY * 4;
constexpr int QT_SHMEM = 2 * QT_STAGE + 144 * 8;             // configuration 41's footprint; the tail holds rows[] / rids[]
static_assert(3 * QT_BIMG + 3 * QT_KIMG <= QT_STAGE && 3 * QT_VIMG <= QT_STAGE, "the core's images reuse the two stages");
static_assert(MAXN * 4 + MAXN <= 144 * 8, "rows[] and rids[] fit the tail");

__global__ __launch_bounds__(576, 1) void swin_qkv_attention_tiled_kernel(TiledParams p) {
  constexpr int NW = 9, NWN = 3, MI = 3, NI = 6, BK = 64;
  constexpr int ROWB = QT_ROWB, A_BYTES = QT_A_BYTES, STAGE = QT_STAGE;
  constexpr int A_INSTR = 2, W_INSTR = 4;                    // 1-KiB DMA instructions per wave and K-tile (8 rows each)
  extern __shared__ __attribute__((aligned(16))) char lds[];          // stage0 {A,W} | stage1 {A,W} | rows[144] | rids[144]
  int* rows = (int*)(lds + 2 * STAGE);
  unsigned char* rids = (unsigned char*)(rows + MAXN);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
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
    if (idx >= (r1 - r0) * w) return;
    const int lr = idx / w;
    tm = r0 + lr; tn = c0 + (idx - lr * w);
  }
  const int C = p.g.C;
  const Window w = window_of(p.g, tm);
  const bool masked = on_shift_seam(p.g, w);
  const int head = 3 * tn + wn;
  stage_rows(p.g, w, tid, rows, rids);                      // read after the loop: its barriers order the writes

  // ---- LDS-DMA source addresses: instruction i of this wave fills rows (i*NW+wave)*8 .. +7
  const int srow = lane >> 3;
  const int schunk = swz<ROWB>(lane & 7, srow);
  const bf16_raw* a_src[A_INSTR];
  const bf16_raw* w_src[W_INSTR];
#pragma unroll
  for (int i = 0; i < A_INSTR; ++i) {
    long r; int rid;
    slot_to_token(p.g, w, (i * NW + wave) * 8 + srow, r, rid);
    a_src[i] = p.A + r * C + schunk * 8;
  }
#pragma unroll
  for (int i = 0; i < W_INSTR; ++i) {
    const int row = (i * NW + wave) * 8 + srow;              // tile column: wave column row / 96, part, channel
    const int wc = row / 96, rem = row - wc * 96;
    w_src[i] = p.W + (long)((rem >> 5) * C + (3 * tn + wc) * HD + wperm(rem & 31)) * C + schunk * 8;
  }

  auto stage = [&](int buf, int kt) {
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

  const int nk = C / BK;
  const int frow = lane & 15, fq = lane >> 4;
  // after the loop: the stage tile nk-1 does not use holds bias | K, the other one V
  char* Bp = lds + (nk & 1) * STAGE;
  char* Kp = Bp + 3 * QT_BIMG;
  char* Vp = lds + ((nk & 1) ^ 1) * STAGE;

  stage(0, 0);
  for (int kt = 0; kt < nk; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (kt + 1 < nk) {
      stage((kt + 1) & 1, kt + 1);
    } else {
      // last K-tile: the other stage is free — the three heads' bias copies, 27 x 1 KiB, three per wave
      const float* bsrc = p.bias_shifted + (long)(3 * tn) * 4 * BS_COPY + lane * 4;
#pragma unroll
      for (int i = 0; i < 3; ++i)
        __builtin_amdgcn_global_load_lds((gptr_t)(bsrc + (i * NW + wave) * 256), (lptr_t)(Bp + (i * NW + wave) * 1024), 16, 0, 0);
    }

    const int cur = kt & 1;
    const char* la = lds + cur * STAGE + (wm * MI * 16 + frow) * ROWB;
    const char* lw = lds + cur * STAGE + A_BYTES + (wn * NI * 16 + frow) * ROWB;
#pragma unroll
    for (int kk = 0; kk < BK / 32; ++kk) {
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

  // ---- q, k, v of this wave's 48 slots, head `head`: acc + bias → bf16 (the stored qkv tensor's bits)
  bf16x8_t qf[MI], kf8[MI], vf8[MI];
  {
    f32x4_t bc[3][2];
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      const f32x4_t* bp = (const f32x4_t*)(p.bqkv + u * C + head * HD + fq * 8);
      bc[u][0] = bp[0]; bc[u][1] = bp[1];
    }
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      bf16x8_t o[3];
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        const f32x4_t v0 = acc[mi][2 * u] * 1.0f + bc[u][0], v1 = acc[mi][2 * u + 1] * 1.0f + bc[u][1];
#pragma unroll
        for (int e = 0; e < 4; ++e) { o[u][e] = (short)f32_to_bf16(v0[e]); o[u][4 + e] = (short)f32_to_bf16(v1[e]); }
      }
      qf[mi] = o[0]; kf8[mi] = o[1]; vf8[mi] = o[2];
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();                             // every wave is past its last fragment read: the stages are free
  {
    char* kimg = Kp + wn * QT_KIMG;
    char* vimg = Vp + wn * QT_VIMG;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      const int slot = (wm * MI + mi) * 16 + frow;
      *(bf16x8_t*)(kimg + slot * HD * 2 + ((fq ^ ((frow >> 2) & 3)) << 4)) = kf8[mi];
      *(bf16x8_t*)(vimg + slot * HD * 2 + (fq << 4)) = vf8[mi];
    }
    if (tid < 3 * 128) ((unsigned long long*)(Vp + (tid >> 7) * QT_VIMG + MAXN * HD * 2))[tid & 127] = 0ull;   // padding keys
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();                             // the three heads' K / V images and bias copies are complete

  // ---- the v3 core on this wave's three query tiles
  const float scale2 = p.g.scale * 1.4426950408889634f;
  const float mask_acc = 100.0f / p.g.scale;
  const int voff = ((4 * fq + (frow >> 2)) * HD + 4 * (frow & 3)) * 2;
  int koffs[9];
#pragma unroll
  for (int kt = 0; kt < 9; ++kt) {
    const int key0 = kt * 16 + fq * 4;
    const int jy = key0 / 12, jx0 = key0 - jy * 12;
    koffs[kt] = (jx0 - jy * 24) * 4;
  }
  auto bias_base = [&](int qn) -> int {
    const int iy = qn / 12, ix = qn - iy * 12;
    const int s = (11 - ix) & 3;
    return (s * BS_COPY + (iy + 11) * 24 + 11 - ix - s) * 4;
  };
#pragma unroll
  for (int qt = 0; qt < 3; ++qt) {
    const int qn = (wm * 3 + qt) * 16 + frow;
    const int orow = rows[qn];
    int koff = (frow * HD + ((fq ^ ((frow >> 2) & 3)) * 8)) * 2, vo = voff, bb = bias_base(qn);
    opaque_offsets(koff, vo, bb);
    const char* kbase = Kp + wn * QT_KIMG + koff;
    const char* vbase = Vp + wn * QT_VIMG + vo;
    const char* bbase = Bp + wn * QT_BIMG + bb;
    f32x4_t sc[9];
    load_bias36(bbase, koffs, sc);
    scores16<false>(kbase, qf[qt], sc);
    if (masked) {
      const unsigned my = rids[qn];
#pragma unroll
      for (int kt = 0; kt < 9; ++kt) {
        const unsigned kr = *(const unsigned*)&rids[kt * 16 + fq * 4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (((kr >> (8 * j)) & 0xff) != my) sc[kt][j] -= mask_acc;
      }
    }
    const float m = row_max36(sc);
    const f32x2_t s2 = {scale2, scale2};
    const f32x2_t c2 = {-m * scale2, -m * scale2};
    f32x2_t lsum = {0.f, 0.f};
    bf16x4_t pk[9];
#pragma unroll
    for (int kt = 0; kt < 9; ++kt) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const f32x2_t a = f32x2_t{sc[kt][2 * h], sc[kt][2 * h + 1]} * s2 + c2;
        const f32x2_t e = {__builtin_amdgcn_exp2f(a[0]), __builtin_amdgcn_exp2f(a[1])};
        lsum += e;
        pk[kt][2 * h] = (short)f32_to_bf16(e[0]);
        pk[kt][2 * h + 1] = (short)f32_to_bf16(e[1]);
      }
    }
    float l = lsum[0] + lsum[1];
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    const float inv_l = __builtin_amdgcn_rcpf(l);
    f32x4_t oacc[2] = {f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int s5 = 0; s5 < 5; ++s5) {
      const bf16x4_t lo4 = pk[2 * s5];
      const bf16x4_t hi4 = s5 < 4 ? pk[2 * s5 + (s5 < 4)] : bf16x4_t{0, 0, 0, 0};
      const bf16x8_t pf = bf16x8_t{lo4[0], lo4[1], lo4[2], lo4[3], hi4[0], hi4[1], hi4[2], hi4[3]};
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const v4s_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) v4s_t*)(vbase + (32 * s5) * HD * 2 + nt * 32));
        const v4s_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) v4s_t*)(vbase + (32 * s5 + 16) * HD * 2 + nt * 32));
        const bf16x8_t vf = bf16x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        oacc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, oacc[nt], 0, 0, 0);
      }
    }
    store_o16<false>(p.out + (long)orow * C + head * HD + fq * 4, oacc, inv_l);
  }
}


// =================================================================================================
// Split-fp16 ("h2") flavour of the v3 kernel — the attention core of the near-exact fast mode (`precision='x3'`).
// q, k, v arrive as hi + lo fp16 pairs (odic_common.h; a head's 32 channels are 128 bytes: [8 hi | 8 lo] x 4) and
// both contractions run as three fp16 MFMAs each:  S = Kh·Qh + Kh·Ql + Kl·Qh,  O = Vh·Ph + Vh·Pl + Vl·Ph  with
// P = exp2(...)·2^12 split into hi + lo as it is produced (the 2^12 keeps the lo halves of the small probabilities
// out of the fp16 subnormals; it cancels in the row normalisation).  Everything between the MFMAs — bias as the
// accumulator init, base-2 softmax on the raw fp32 accumulators, mask — is the v3 code.
//   K image  [144][128 B]: per row the four hi fragments then the four lo fragments, slots XOR-swizzled with row & 7
//            (the planar order and the swizzle are applied through the per-lane LDS-DMA source address);
//   V images [160][64 B] x 2 (hi, lo), consumed through ds_read_b64_tr_b16 exactly like the 16-bit kernel's V.
// 48 KiB of LDS → three blocks per CU.
// =================================================================================================
__global__ __launch_bounds__(192, 3) void window_attention_h2_kernel(WinParams p) {
  __shared__ __attribute__((aligned(16))) char Kx[MAXN * 128];          // 18432 B
  __shared__ __attribute__((aligned(16))) bf16_raw Vh[MAXN + 16][HD];   // 10240 B (rows 144..159 zero)
  __shared__ __attribute__((aligned(16))) bf16_raw Vl[MAXN + 16][HD];   // 10240 B
  __shared__ __attribute__((aligned(16))) float Bs[4 * BS_COPY];        // 9216 B
  __shared__ int rows[MAXN];
  __shared__ __attribute__((aligned(4))) unsigned char rids[MAXN];

  ODIC_ENCODE_PRIO();
  const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
  const int head = idx % p.g.heads;
  const int win = (idx / p.g.heads) * 8 + xcd;
  if (win >= p.g.B * (p.g.nwin_side * p.g.nwin_side)) return;
  const Window w = window_of(p.g, win);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const char* qkv = (const char*)p.qkv;
  const long ldb = 12L * p.g.C;                                           // bytes per token row of [*, 3C] h2
  const long kbyte = 4L * p.g.C, vbyte = 8L * p.g.C;                        // byte offsets of the k / v column blocks
  const bool masked = on_shift_seam(p.g, w);

  {
    const float* bsrc = p.bias_shifted + (long)head * 4 * BS_COPY + lane * 4;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int blk = wave * 3 + i;
      __builtin_amdgcn_global_load_lds((gptr_t)(bsrc + blk * 256), (lptr_t)((char*)&Bs[0] + blk * 1024), 16, 0, 0);
    }
  }
  stage_rows(p.g, w, tid, rows, rids);
  zero_padding_keys(Vh, tid);
  zero_padding_keys(Vl, tid);
  __syncthreads();

  // ---- LDS-DMA gather.  K: instruction j covers window slots 8j .. 8j+7 (8 rows x 128 B); V: slots 16i .. 16i+15
  //      of one plane (16 rows x 64 B).  Six K and six V instructions per wave.
  {
    const int r8 = lane >> 3, pos = lane & 7;
    const int img = pos ^ r8;                                            // image chunk held by this LDS slot
    const int mc = img < 4 ? 2 * img : 2 * (img - 4) + 1;                // its 16-byte chunk in memory
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const int j = wave * 6 + i;                                        // 0..17
      const char* src = qkv + (long)rows[j * 8 + r8] * ldb + kbyte + head * 128 + mc * 16;
      __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(Kx + j * 1024), 16, 0, 0);
    }
    const int r16 = lane >> 2, ch = lane & 3;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int blk = wave * 3 + i;                                      // 0..8
      const char* src = qkv + (long)rows[blk * 16 + r16] * ldb + vbyte + head * 128 + ch * 32;
      __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)((char*)&Vh[0][0] + blk * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((gptr_t)(src + 16), (lptr_t)((char*)&Vl[0][0] + blk * 1024), 16, 0, 0);
    }
  }
  const int fr = lane & 15, fq = lane >> 4;
  const float scale2 = p.g.scale * 1.4426950408889634f;
  const float mask_acc = 100.0f / p.g.scale;
  const int voff = ((4 * fq + (fr >> 2)) * HD + 4 * (fr & 3)) * 2;
  int koffs[9];
#pragma unroll
  for (int kt = 0; kt < 9; ++kt) {
    const int key0 = kt * 16 + fq * 4;
    const int jy = key0 / 12, jx0 = key0 - jy * 12;
    koffs[kt] = (jx0 - jy * 24) * 4;
  }
  auto bias_base = [&](int qn) -> int {
    const int iy = qn / 12, ix = qn - iy * 12;
    const int s = (11 - ix) & 3;
    return (s * BS_COPY + (iy + 11) * 24 + 11 - ix - s) * 4;
  };

  // first tile's Q fragments (B operand of Sᵀ = K·Qᵀ: Q[query = fr][d = 8·fq ..], hi chunk then lo chunk)
  const char* qp = qkv + (long)rows[wave * 48 + fr] * ldb + head * 128 + fq * 32;
  f16x8_t qh = *(const f16x8_t*)qp, ql = *(const f16x8_t*)(qp + 16);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

#pragma unroll
  for (int qt = 0; qt < 3; ++qt) {
    const int qn = (wave * 3 + qt) * 16 + fr;
    const int orow = rows[qn];
    int koh = fr * 128 + ((fq ^ (fr & 7)) << 4), vo = voff, bb = bias_base(qn);
    opaque_offsets(koh, vo, bb);
    const char* kbase = Kx + koh;                                        // hi fragment; lo = slot ^ 4 → byte ^ 64
    const char* bbase = (const char*)&Bs[0] + bb;
    f32x4_t sc[9];
    load_bias36(bbase, koffs, sc);
#pragma unroll
    for (int kt = 0; kt < 9; ++kt) {
      const f16x8_t kh = *(const f16x8_t*)(kbase + kt * 16 * 128);
      const f16x8_t kl = *(const f16x8_t*)(Kx + ((koh ^ 64) + kt * 16 * 128));
      sc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kl, qh, sc[kt], 0, 0, 0);
      sc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh, ql, sc[kt], 0, 0, 0);
      sc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh, qh, sc[kt], 0, 0, 0);
    }
    if (masked) {
      const unsigned my = rids[qn];
#pragma unroll
      for (int kt = 0; kt < 9; ++kt) {
        const unsigned kr = *(const unsigned*)&rids[kt * 16 + fq * 4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (((kr >> (8 * j)) & 0xff) != my) sc[kt][j] -= mask_acc;
      }
    }
    const float m = row_max36(sc);
    const float c2 = 12.0f - m * scale2;                                 // P carries a factor 2^12
    float lsum = 0.f;
    f16x4_t ph[9], pl[9];
#pragma unroll
    for (int kt = 0; kt < 9; ++kt) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float e = __builtin_amdgcn_exp2f(fmaf(sc[kt][j], scale2, c2));
        lsum += e;
        const f16_t h = (f16_t)e;
        ph[kt][j] = h;
        pl[kt][j] = (f16_t)(e - (float)h);
      }
    }
    if (qt < 2) {                                                        // next tile's Q under the P·V work below
      const char* qn_p = qkv + (long)rows[qn + 16] * ldb + head * 128 + fq * 32;
      qh = *(const f16x8_t*)qn_p; ql = *(const f16x8_t*)(qn_p + 16);
    }
    float l = lsum;
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    const float inv_l = 1.0f / l;

    f32x4_t oacc[2] = {f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}};
    const f16x4_t z4 = {(f16_t)0.f, (f16_t)0.f, (f16_t)0.f, (f16_t)0.f};
#pragma unroll
    for (int s5 = 0; s5 < 5; ++s5) {
      const f16x4_t h0 = ph[2 * s5], l0 = pl[2 * s5];
      const f16x4_t h1 = s5 < 4 ? ph[2 * s5 + (s5 < 4)] : z4, l1 = s5 < 4 ? pl[2 * s5 + (s5 < 4)] : z4;
      const f16x8_t pfh = f16x8_t{h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
      const f16x8_t pfl = f16x8_t{l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]};
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const int off = vo + (32 * s5) * HD * 2 + nt * 32;
        const v4s_t ah0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s_t*)((char*)&Vh[0][0] + off));
        const v4s_t ah1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s_t*)((char*)&Vh[0][0] + off + 16 * HD * 2));
        const v4s_t al0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s_t*)((char*)&Vl[0][0] + off));
        const v4s_t al1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s_t*)((char*)&Vl[0][0] + off + 16 * HD * 2));
        const bf16x8_t vh8 = bf16x8_t{ah0[0], ah0[1], ah0[2], ah0[3], ah1[0], ah1[1], ah1[2], ah1[3]};
        const bf16x8_t vl8 = bf16x8_t{al0[0], al0[1], al0[2], al0[3], al1[0], al1[1], al1[2], al1[3]};
        const f16x8_t vh = __builtin_bit_cast(f16x8_t, vh8), vl = __builtin_bit_cast(f16x8_t, vl8);
        oacc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vl, pfh, oacc[nt], 0, 0, 0);
        oacc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, pfl, oacc[nt], 0, 0, 0);
        oacc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, pfh, oacc[nt], 0, 0, 0);
      }
    }
    h2_t* drow = (h2_t*)p.out + (long)orow * p.g.C + head * HD;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
      h2_store4(drow, nt * 16 + fq * 4, oacc[nt][0] * inv_l, oacc[nt][1] * inv_l, oacc[nt][2] * inv_l, oacc[nt][3] * inv_l);
  }
}

}  // namespace

extern "C" int odic_window_attention(const void* qkv, const float* bias_table, const float* bias_shifted_prescaled,
                                     void* out, int32_t B, int32_t res, int32_t C, int32_t heads, int32_t ws,
                                     int32_t shift, float scale, int32_t dtype, void* stream) {
  if (!qkv || !bias_table || !out) return ODIC_ENULL;
  if (B <= 0 || ws <= 0 || ws * ws > MAXN || res % ws || heads * HD != C || shift < 0 || shift >= ws)
    return ODIC_EINVAL;
  if (((uintptr_t)qkv & 15) || ((uintptr_t)out & 15)) return ODIC_EINVAL;
  const WinParams p = {qkv, bias_table, bias_shifted_prescaled, out, {B, res, C, heads, ws, shift, res / ws, scale}};
  const int nwin = B * p.g.nwin_side * p.g.nwin_side;
  const dim3 grid(nwin, heads), block(192);
  // the packed-bias kernels: 32-bit token rows, 16-byte DMA of the bias; one round of eight blocks per 8 windows and head
  const bool packed = bias_shifted_prescaled && (long)B * res * res < 2147483647L && !(((uintptr_t)bias_shifted_prescaled) & 15);
  const dim3 xgrid(((nwin + 7) / 8) * 8 * heads);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == ODIC_F32) {
    hipLaunchKernelGGL(window_attention_f32_kernel, grid, block, 0, s, p);
  } else if (dtype == ODIC_BF16) {
    if (ws != 12) return ODIC_EUNSUPPORTED;      // MFMA tiling is specialised for N = 144
    // (a persistent, double-buffered variant — one head x several windows per block — measured
    //  slower at every stage: with ~0.5 us of work per window a prefetch distance of one window does
    //  not cover the gather latency, and six independent 3-wave blocks per CU keep more bytes in flight)
    if (packed) hipLaunchKernelGGL(window_attention_bf16_v3_kernel<false>, xgrid, block, 0, s, p);
    else hipLaunchKernelGGL(window_attention_bf16_kernel, grid, block, 0, s, p);
  } else if (dtype == ODIC_F16) {
    if (ws != 12 || !packed) return ODIC_EUNSUPPORTED;      // fp16 activations: packed-bias MFMA kernel only
    hipLaunchKernelGGL(window_attention_bf16_v3_kernel<true>, xgrid, block, 0, s, p);
  } else if (dtype == ODIC_H2) {
    if (ws != 12 || !packed || ((uintptr_t)qkv & 31) || ((uintptr_t)out & 31))
      return ODIC_EUNSUPPORTED;                  // split-fp16 activations: packed-bias MFMA kernel only
    hipLaunchKernelGGL(window_attention_h2_kernel, xgrid, block, 0, s, p);
  } else {
    return ODIC_EINVAL;
  }
  return odic_launch_status();
}

/* norm1 → qkv → attention core of one Swin block in one launch (stage width 192; see swin_qkv_attention_kernel). */
extern "C" int odic_swin_qkv_attention(const float* x, int64_t ldx, const void* w_qkv_folded, const float* b_qkv_folded,
                                       const float* bias_shifted_prescaled, void* out, int32_t B, int32_t res, int32_t C,
                                       int32_t heads, int32_t ws, int32_t shift, float scale, float ln_eps, void* stream) {
  if (!x || !w_qkv_folded || !b_qkv_folded || !bias_shifted_prescaled || !out) return ODIC_ENULL;
  if (B <= 0 || ws != 12 || res % ws || heads * HD != C || shift < 0 || shift >= ws || ldx < C) return ODIC_EINVAL;
  if (C != 192) return ODIC_EUNSUPPORTED;
  if (((uintptr_t)x & 15) || (ldx & 3) || ((uintptr_t)w_qkv_folded & 15) || ((uintptr_t)out & 7) ||
      ((uintptr_t)bias_shifted_prescaled & 15) || ((uintptr_t)b_qkv_folded & 3) || (long)B * res * res >= 2147483647L)
    return ODIC_EINVAL;
  const FusedParams p = {x, ldx, (const bf16_raw*)w_qkv_folded, b_qkv_folded, bias_shifted_prescaled, (bf16_raw*)out,
                         {B, res, C, heads, ws, shift, res / ws, scale}, ln_eps};
  constexpr int SHMEM = 2 * 3 * 96 * 128 + MAXN * HD * 2 + (MAXN + 16) * HD * 2 + 2 * 4 * BS_COPY * 4 + 3 * 192 * 4 + MAXN * 4 + MAXN;
  auto k = swin_qkv_attention_kernel<3>;
  static bool done = false;
  if (!done) { (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, SHMEM); done = true; }
  hipLaunchKernelGGL(k, dim3(B * p.g.nwin_side * p.g.nwin_side), dim3(576), SHMEM, (hipStream_t)stream, p);
  return odic_launch_status();
}

/* qkv Linear → attention core of one Swin block in one launch for the wide stages (see swin_qkv_attention_tiled_kernel). */
extern "C" int odic_swin_qkv_attention_tiled(const void* xn, const void* w_qkv, const float* b_qkv,
                                             const float* bias_shifted_prescaled, void* out, int32_t B, int32_t res,
                                             int32_t C, int32_t heads, int32_t ws, int32_t shift, float scale, void* stream) {
  if (!xn || !w_qkv || !b_qkv || !bias_shifted_prescaled || !out) return ODIC_ENULL;
  if (B <= 0 || res <= 0 || ws <= 0 || heads <= 0 || res % ws || shift < 0 || shift >= ws) return ODIC_EINVAL;
  if (ws != 12 || heads * HD != C || heads % 3 || C % 64) return ODIC_EUNSUPPORTED;
  if (((uintptr_t)xn & 15) || ((uintptr_t)w_qkv & 15) || ((uintptr_t)out & 7) || ((uintptr_t)bias_shifted_prescaled & 15) ||
      ((uintptr_t)b_qkv & 15) || (long)B * res * res >= 2147483647L)
    return ODIC_EINVAL;
  TiledParams p = {(const bf16_raw*)xn, (const bf16_raw*)w_qkv, b_qkv, bias_shifted_prescaled, (bf16_raw*)out,
                   {B, res, C, heads, ws, shift, res / ws, scale}, {}};
  // one tile form, chosen by rule (legal inside a stream capture at a shape never run before): configuration 41's grid
  const long M = (long)B * res * res;
  const int max_rect = tile_grid(p.grid, (int)M, 3 * C, 144, 288, (double)M * C * 2.0, 3.0 * C * C * 2.0, 32);
  tile_allow_lds<QT_SHMEM, swin_qkv_attention_tiled_kernel>();
  hipLaunchKernelGGL(swin_qkv_attention_tiled_kernel, dim3(8 * max_rect), dim3(576), QT_SHMEM, (hipStream_t)stream, p);
  return odic_launch_status();
}
