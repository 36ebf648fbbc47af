// Shared by the three MFMA NT GEMM families (gemm_bf16.hip, gemm_x3.hip, gemm_lowp.hip): the chunk swizzle, the W row
// permutation, the tile grid with its XCD partition, and the host's launch helpers.  The kernels' rectangle walk, LDS-DMA
// staging and counted wait stay as text in each kernel: written as helpers here they compile to another instruction
// stream in every tiled kernel (profiles/r08_gemm_tile_header_bench.txt).
#pragma once
#include "odic_common.h"

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

// 16-byte-chunk swizzle inside an LDS row of ROWB bytes.  128-byte rows (8 chunks): chunk ^ (row & 7).  64-byte rows
// (4 chunks; 4 rows share a 256-byte bank row): chunk ^ f((row >> 2) & 3) with f = {0, 2, 3, 1}, which makes every
// 16-lane service group of ds_read_b128 hit 16 distinct slots.  Applied to the per-lane DMA SOURCE address and again on
// the fragment read: both sides or neither.
template <int ROWB> __device__ __forceinline__ int swz(int chunk, int row) {
  static_assert(ROWB == 128 || ROWB == 64, "LDS rows are 128 or 64 bytes");
  if constexpr (ROWB == 128) return chunk ^ (row & 7);
  else return chunk ^ ((0x78 >> (2 * ((row >> 2) & 3))) & 3);
}

// LDS row r of the W tile holds tile-local output column wperm(r): inside each 32-row group the two 16-row MFMA tiles
// interleave in runs of 4, so that MFMA slot 4·fq + j of tile h is column 8·fq + 4·h + j and a lane's registers across
// the tile pair are 8 adjacent output columns.
__device__ __forceinline__ int wperm(int r) {
  return (r & ~31) + 8 * ((r & 15) >> 2) + 4 * ((r >> 4) & 1) + (r & 3);
}

// The tile grid and its XCD partition (pm * pn == 8), filled by tile_grid() on the host.  Each family's Params embeds it
// where these four ints have always been: no kernel-argument offset depends on this header.
struct TileGrid { int tiles_m, tiles_n, pm, pn; };

// ------------------------------------------------------------------------------------------------------------- host
// XCD partition of a GEMM's tile grid: pm x pn = 8 rectangles, one per XCD (= per 4 MiB L2; blocks b, b + 8, ... share an
// XCD).  Every row panel of A is fetched by the pn XCDs of its rectangle row and W by the pm XCDs of its rectangle column,
// so the split that moves the fewest bytes across the fabric minimises  pn·|A| + pm·|W|;  a W sub-panel that does not fit
// an L2 share beside the streaming A panels is fetched again by every round of its rectangle.  (Rounds 1-2 only asked for
// the W sub-panel to fit: with A >> W — fc2: 56 MB of hidden activations against 4.7 MB of weights — that read A two
// to four times: PMC FETCH_SIZE 3.3x the algorithmic bytes on the split-fp16 fc2.)
static inline void odic_xcd_partition(int tiles_m, int tiles_n, double a_bytes, double w_bytes, int slots_per_xcd,
                                      int* pm_out, int* pn_out) {
  double best = 1e300;
  int bpm = 0, bpn = 0;
  for (int pn = 1; pn <= 8; pn *= 2) {
    const int pm = 8 / pn;
    if (pn > tiles_n || pm > tiles_m) continue;
    const long rect = (long)((tiles_m + pm - 1) / pm) * ((tiles_n + pn - 1) / pn);
    const long rounds = (rect + slots_per_xcd - 1) / slots_per_xcd;
    const double wf = (w_bytes / pn > 2.5 * 1024 * 1024) ? (double)rounds : 1.0;
    const double cost = pn * a_bytes + pm * w_bytes * wf;
    if (cost < best) { best = cost; bpm = pm; bpn = pn; }
  }
  if (!bpm) {                                             // fewer tiles than XCDs along both axes: as many row parts as there are
    bpm = 8;
    while (bpm > tiles_m && bpm > 1) bpm /= 2;
    bpn = 8 / bpm;
  }
  *pm_out = bpm; *pn_out = bpn;
}

// Fills the tile grid of an M x N product in BM x BN tiles and returns the tile count of its largest XCD rectangle: the
// launch is 8 * that many blocks; the kernels' rectangle walk uses the same arithmetic and retires the surplus blocks.
static inline int tile_grid(TileGrid& g, int M, int N, int BM, int BN, double a_bytes, double w_bytes, int slots_per_xcd) {
  g.tiles_m = (M + BM - 1) / BM; g.tiles_n = (N + BN - 1) / BN;
  odic_xcd_partition(g.tiles_m, g.tiles_n, a_bytes, w_bytes, slots_per_xcd, &g.pm, &g.pn);
  int max_rect = 0;
  for (int xm = 0; xm < g.pm; ++xm)
    for (int xn = 0; xn < g.pn; ++xn) {
      const int r = ((xm + 1) * g.tiles_m / g.pm - xm * g.tiles_m / g.pm) * ((xn + 1) * g.tiles_n / g.pn - xn * g.tiles_n / g.pn);
      if (r > max_rect) max_rect = r;
    }
  return max_rect;
}

// Kernels that ask for more than 64 KiB of dynamic LDS have the limit raised before their first launch (a code-object
// attribute: idempotent, and racing first calls set the same value).  One flag per set of kernels.
template <int SHMEM, auto... KERNELS> static inline void tile_allow_lds() {
  if constexpr (SHMEM > 64 * 1024) {
    static bool done = false;
    if (!done) {
      ((void)hipFuncSetAttribute((const void*)KERNELS, hipFuncAttributeMaxDynamicSharedMemorySize, SHMEM), ...);
      done = true;
    }
  }
}

// Built-in tile choice: a launch of bm x bn tiles runs in ceil(tiles / resident slots) rounds.  The per-tile cost each
// family weighs the rounds with, and the choice, stay in its file.
static inline double tile_rounds(int M, int N, int batch, int bm, int bn, int slots) {
  const long t = (long)((M + bm - 1) / bm) * ((N + bn - 1) / bn) * batch;
  return (double)((t + slots - 1) / slots);
}

// A-resident kernels: column ranges per row panel = the smallest divisor of the chunk count that gives the chip at least
// `want` blocks — a block should keep its A rows for as many chunks as the grid size allows.
static inline int panel_split(int panels, int nchunks, int want) {
  for (int d = 1; d <= nchunks; ++d)
    if (nchunks % d == 0 && (long)panels * d >= want) return d;
  return nchunks;
}
