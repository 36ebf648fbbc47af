// EXIF orientation on the device: the seven non-trivial values of tag 0x0112 as a permutation of packed
// RGB8 pixels, bit for bit what Pillow's Image.transpose does for ImageOps.exif_transpose:
//
//   2 FLIP_LEFT_RIGHT   3 ROTATE_180   4 FLIP_TOP_BOTTOM   5 TRANSPOSE   6 ROTATE_270   7 TRANSVERSE   8 ROTATE_90
//
// Every one of them is "mirror x?, mirror y?, then swap the axes?":  with u = flip_y ? H-1-y : y and
// v = flip_x ? W-1-x : x, source pixel (y, x) lands at (u, v), or at (v, u) for the swapping orientations 5..8.
//
// One block moves one T x T pixel tile of one job through LDS.  The source tile is read row by row and the destination
// tile written row by row, one wave per row, so that every global access of a wave covers one contiguous run of at
// most 3 T bytes whatever the orientation; the permutation happens in the LDS read between the two.  Rows of 3 W bytes
// start at any byte address, so a lane owns one ALIGNED dword of the run: whole dwords move as dwords, the run's first
// and last partial dwords as bytes.  An LDS row keeps the run at its global misalignment (run byte q of tile row r at
// r·PITCH + mis(r) + q), which makes an aligned global dword an aligned LDS dword.  PITCH is 49 dwords: the swapping
// orientations read one source COLUMN per destination row, and an odd dword pitch spreads that column over all banks
// (48 dwords would put it on two).
#include "odic_common.h"

namespace {

constexpr int T = 64;                    // tile side in pixels
constexpr int PITCH = 3 * T + 4;         // bytes per LDS row: 3 T of pixels + up to 3 of misalignment, 49 dwords
constexpr int MAX_JOBS = 64;             // jobs per launch: they travel as kernel arguments

static_assert(PITCH % 4 == 0 && (PITCH / 4) % 2 == 1, "an odd dword pitch keeps the column read off one bank");
static_assert(PITCH / 4 <= ODIC_WAVE, "one lane per dword of a row");

struct OrientBatch {
  odic_orient_job job[MAX_JOBS];
  int tile_end[MAX_JOBS];                // running total of tiles up to and including job j
};

__global__ __launch_bounds__(256) void orient_rgb8_kernel(const OrientBatch b, const unsigned char* __restrict__ src_base,
                                                          unsigned char* __restrict__ dst_base) {
  __shared__ __attribute__((aligned(16))) unsigned char tile[T * PITCH];
  const int t = blockIdx.x;
  int j = 0;
  while (j < MAX_JOBS - 1 && t >= b.tile_end[j]) ++j;                    // uniform: the grid ends at the last tile_end
  const int first = j ? b.tile_end[j - 1] : 0;
  const long src_stride = b.job[j].src_stride_bytes;
  const int H = b.job[j].H, W = b.job[j].W, o = b.job[j].orientation;
  const bool flip_x = (0x18C >> o) & 1, flip_y = (0x0D8 >> o) & 1, swap = o >= 5;      // {2,3,7,8}, {3,4,6,7}
  const int tiles_x = (W + T - 1) / T;
  const int ty = (t - first) / tiles_x, tx = (t - first) - ty * tiles_x;
  const int y0 = ty * T, x0 = tx * T;
  const int th = min(T, H - y0), tw = min(T, W - x0);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;

  // source tile → LDS, one wave per row
  const unsigned char* s0 = src_base + b.job[j].src_off + (long)y0 * src_stride + 3L * x0;
  const unsigned sm0 = (unsigned)(uintptr_t)s0 & 3u, sms = (unsigned)src_stride & 3u;
  const int sbytes = 3 * tw;
  unsigned word[T / 4];                                                   // all of a wave's row loads in flight at once
#pragma unroll
  for (int i = 0; i < T / 4; ++i) {
    const int r = wave + 4 * i;
    const int lo = 4 * lane - (int)((sm0 + r * sms) & 3u);               // the lane's dword holds run bytes [lo, lo + 4)
    word[i] = 0;
    if (r < th && lo >= 0 && lo + 4 <= sbytes) word[i] = *(const unsigned*)(s0 + (long)r * src_stride + lo);
  }
#pragma unroll
  for (int i = 0; i < T / 4; ++i) {
    const int r = wave + 4 * i;
    if (r >= th) break;
    const unsigned char* row = s0 + (long)r * src_stride;
    const int lo = 4 * lane - (int)((sm0 + r * sms) & 3u);
    unsigned char* l = tile + r * PITCH + 4 * lane;
    if (lo >= 0 && lo + 4 <= sbytes) {
      *(unsigned*)l = word[i];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (lo + e >= 0 && lo + e < sbytes) l[e] = row[lo + e];
    }
  }
  __syncthreads();

  // LDS → destination tile, one wave per row
  const int dh = swap ? tw : th, dw = swap ? th : tw;
  const int u0 = flip_y ? H - y0 - th : y0, v0 = flip_x ? W - x0 - tw : x0;
  const long dst_stride = 3L * (swap ? H : W);
  unsigned char* d0 = dst_base + b.job[j].dst_off + (long)(swap ? v0 : u0) * dst_stride + 3L * (swap ? u0 : v0);
  const unsigned dm0 = (unsigned)(uintptr_t)d0 & 3u, dms = (unsigned)dst_stride & 3u;
  const int dbytes = 3 * dw;
#pragma unroll 4
  for (int r = wave; r < dh; r += 4) {
    unsigned char* row = d0 + (long)r * dst_stride;
    const int lo = 4 * lane - (int)((dm0 + r * dms) & 3u);
    if (lo >= dbytes) continue;
    unsigned v = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int q = min(max(lo + e, 0), dbytes - 1);                     // a byte outside the run repeats its neighbour: not stored
      const int px = q / 3, c = q - 3 * px;
      const int lu = swap ? px : r, lv = swap ? r : px;                  // along the source's y and x
      const int sy = flip_y ? th - 1 - lu : lu, sx = flip_x ? tw - 1 - lv : lv;
      v |= (unsigned)tile[sy * PITCH + ((sm0 + sy * sms) & 3u) + 3 * sx + c] << (8 * e);
    }
    if (lo >= 0 && lo + 4 <= dbytes) {
      *(unsigned*)(row + lo) = v;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (lo + e >= 0 && lo + e < dbytes) row[lo + e] = (unsigned char)(v >> (8 * e));
    }
  }
}

}  // namespace

static_assert(sizeof(odic_orient_job) == 40, "odic_orient_job is packed by image_utils.ORIENT_JOB_DTYPE");

extern "C" int odic_orient_rgb8(const odic_orient_job* jobs, int32_t n_jobs, const uint8_t* src_base, uint8_t* dst_base,
                                void* stream) {
  if (n_jobs < 0) return ODIC_EINVAL;
  if (n_jobs == 0) return 0;
  if (!jobs || !src_base || !dst_base) return ODIC_EINVAL;
  for (int32_t k = 0; k < n_jobs; ++k) {
    const odic_orient_job& q = jobs[k];
    if (q.orientation < 2 || q.orientation > 8 || q.H <= 0 || q.W <= 0 || q.src_stride_bytes < 3L * q.W) return ODIC_EINVAL;
    if ((((long)q.H + T - 1) / T) * (((long)q.W + T - 1) / T) > 0x7fffffffL) return ODIC_EINVAL;     // tiles of one job: a grid
  }
  hipStream_t s = (hipStream_t)stream;
  OrientBatch b;
  for (int32_t k = 0; k < n_jobs;) {                                     // one launch per MAX_JOBS jobs or 2^31 - 1 tiles
    long tiles = 0;
    int n = 0;
    for (; k < n_jobs && n < MAX_JOBS; ++k, ++n) {
      const long more = (((long)jobs[k].H + T - 1) / T) * (((long)jobs[k].W + T - 1) / T);
      if (tiles + more > 0x7fffffffL) break;
      tiles += more;
      b.job[n] = jobs[k];
      b.tile_end[n] = (int)tiles;
    }
    for (int m = n; m < MAX_JOBS; ++m) { b.job[m] = b.job[n - 1]; b.tile_end[m] = (int)tiles; }
    hipLaunchKernelGGL(orient_rgb8_kernel, dim3((unsigned)tiles), dim3(256), 0, s, b, src_base, dst_base);
  }
  return odic_launch_status();
}
