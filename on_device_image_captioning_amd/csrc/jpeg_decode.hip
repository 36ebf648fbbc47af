// Batched baseline JPEG decode, bit-exact with np.asarray(PIL.Image.open(f)) — Pillow on
// libjpeg-turbo's default path: ISLOW IDCT, "fancy" triangle upsampling, table-driven YCbCr→RGB.
//
// The host parser (on_device_image_captioning_amd/jpeg.py) walks the markers up to SOS and packs one
// odic_jpeg_header per image: quantisation tables in natural order, Huffman tables in a lookup form, the
// restart interval and the workspace offsets.  Everything after SOS is decoded here, the whole batch in one
// pass of launches on the caller's stream.  Progressive files (second half of the file) take their own segment
// and decode kernels and then the same IDCT and colour kernels; both paths share one workspace layout (layout(),
// bind()), the bit reader and the Huffman lookup (huff(), fill_lim()).  The baseline launches:
//
//   segment     one workgroup per image: classify every byte of the scan (data, stuffed 0x00, RSTn, EOI, any
//               other marker → error), compact the data bytes with a prefix sum, record the start bit of each
//               restart interval (without DRI the whole scan is one interval) and split every interval into
//               units of subseq_bits bits.
//   speculate   one lane per unit: decode from the unit's first bit with a guessed state (bit position,
//               block in MCU, zig-zag index) = (start, 0, 0) until the unit's end; record the end state and the
//               number of blocks begun.  The first unit of an interval starts from the exact state.
//   sync × P    Jacobi passes of the self-synchronising scheme of Weißenberger & Schmidt (ICPP 2018): unit u
//               decodes again from the end state of unit u-1 of the previous pass.  A pass in which no unit
//               of an interval changes its end state proves that interval's states exact; once a whole pass
//               changes nothing, the remaining passes return at once (device flag).
//   serial      one wave per interval that did not converge (all of them with max_sync_passes = 0): walk its
//               units from the exact start, decoding again every unit whose last start state was wrong.
//   scan        per image: exclusive prefix of the blocks begun per unit.
//   write-out   one lane per unit: decode again from the synchronised start state and write int16
//               coefficients in natural order (DC as a difference) at the unit's block indices.
//   dc          per image and component: DC prediction, a scan that resets at each restart interval.
//   idct        jidctint.c jpeg_idct_islow with dequantisation and the masked post-IDCT range limit
//               (range_limit[x & 1023]), writing uint8 planes padded to whole MCUs.
//   color       h2v1 / h2v2 fancy upsampling + jdcolor.c ycc_rgb_convert, cropped H×W×3 into the caller's
//               buffer, and the per-image status.
//
// odic_jpeg_decode_scaled / odic_jpeg_decode_progressive_scaled (Pillow's Image.draft) run the same launches up to the
// coefficients and then the scaled forms of the last two: reduced 4x4 / 2x2 / 1x1 inverse transforms per component
// (idct_blocks) and a colour pass over ceil(W / s) × ceil(H / s) pixels (color_pixel), s = 1, 2, 4, 8 per image.
//
// One-component (grayscale) frames, sampling = 3, take the same launches in the same batch: one block per MCU in
// block-raster order, tables 0 / 3, one plane, and a colour pass that writes R = G = B = Y (Pillow's L → RGB).
//
// All of the above is the COMMON record family: odic_jpeg_header (baseline) and odic_jpeg_prog_header (progressive),
// whose frame is one `sampling` word.  Every kernel is a template over the header type, and the second family goes
// through the same launches:
//
// The PER-COMPONENT family — odic_jpeg_header_any (odic_jpeg_any_decode) and odic_jpeg_prog_header_any
// (odic_jpeg_decode_progressive_any) — carries ncomp = 3 or 4, the sampling of every component in h[] / v[], a `color`
// flag, four quantisation tables and, in the baseline record, eight Huffman tables.  It holds four-component frames (CMYK,
// or YCCK with color = 1) and three-component frames at any other sampling layout libjpeg decodes (4:4:0, 4:1:1, 4:1:0,
// chroma sub-sampled one way under a 2x2 luma, a component 0 that is not the largest), stored as YCbCr or, with
// color = 1, as RGB; one batch may mix the counts.  One rule set admits a frame (layout_ok); Frame<Header> gives the
// entropy kernels the blocks per MCU and the component of each, ProgGeo the same to the progressive coding procedures;
// the IDCT writes ncomp planes (block_geo_own), and one colour kernel (color_own_pixels) reads every component through
// upsampled_by() — copy, h2v1 / h2v2 / h1v2 fancy, or replication by an integral ratio — and then converts: YCbCr → RGB
// or a copy for three components; YCCK → CMYK, Pillow's inversion and Pillow's CMYK → RGB for four:
// np.asarray(PIL.Image.open(f).convert("RGB")).  The _scaled entry points of this family take every component at
// libjpeg's own transform size for the scale (scaled_size_own), planes at those sizes (plane_bytes_own), and the
// upsampling that remains, with the triangle filters while the smallest transform is above 1x1.
//
// An image whose entropy data does not decode (invalid code, unexpected marker, RST out of sequence, too few
// or too many intervals, an interval whose MCUs need bits past its end, a run past coefficient 63, no EOI), or
// whose coefficients leave the range where libjpeg-turbo's SIMD and C IDCTs agree (kIdctLimit), gets status 1:
// the caller decodes it again on the host.  Entropy data that does decode yields libjpeg's coefficients exactly.
#include <type_traits>

#include "odic_common.h"

static_assert(sizeof(odic_jpeg_header) == 9016 && offsetof(odic_jpeg_header, qt) == 88 &&
                  offsetof(odic_jpeg_header, huffval) == 7480,
              "odic_jpeg_header layout is mirrored by jpeg.HEADER_DTYPE");
static_assert(sizeof(odic_jpeg_header_any) == 12032 && offsetof(odic_jpeg_header_any, h) == 88 &&
                  offsetof(odic_jpeg_header_any, ncomp) == 120 && offsetof(odic_jpeg_header_any, qt) == 128 &&
                  offsetof(odic_jpeg_header_any, huffval) == 9984,
              "odic_jpeg_header_any layout is mirrored by jpeg.HEADER_ANY_DTYPE");

namespace {

constexpr int kInvalidPos = 0x7fffffff;
constexpr int kLutBits = 9;
constexpr int kStateWords = 8;            // per image: [0] error bits, [1] intervals finished
constexpr int kErrSegment = 1, kErrDecode = 2, kErrRange = 4;
// Pillow's libjpeg-turbo runs the SIMD ISLOW IDCT: 16-bit dequantisation products, 16-bit sums of up to four inputs,
// pass-1 results packed to 16 bits, and a saturating final clamp where the C code masks (x & 1023).  The two agree,
// and this file's int32 arithmetic is exact, while every dequantised coefficient and every pass-1 value stays within
// ±kIdctLimit and every final value within [-512, 511].  Legitimate 8-bit images stay far inside (the extreme cases
// tried — 1-pixel checkerboards and binary noise at quality 100 — reach 838, 3702 and [-134, 131]); anything else gets
// kErrRange and is decoded by the host.  A DC value that leaves int16 (JCOEF) gets it too.
constexpr int kIdctLimit = 8191;

__device__ const unsigned char kNatural[64] = {
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
    28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
    54, 47, 55, 62, 63};

struct Ws {                                // workspace regions (host-computed from the batch totals)
  int* state;                              // [n_images][kStateWords]
  int* flags;                              // [0] last sync pass that ran, [1 + p] pass p changed something
  int* last_change;                        // per interval: last pass that changed one of its units
  unsigned char* scan;                     // compacted entropy data
  int* int_bits;                           // per image n_intervals + 1 interval boundaries (bits)
  int* unit_start;                         // per image n_intervals + 1 first unit of each interval
  int4* est[2];                            // per unit end state {pos, blk, k, blocks begun}, two pass buffers
  int* unit_first;                         // per unit: blocks begun in the image before it
  short* coef;                             // [blocks][64]
  unsigned char* planes;
};

struct Layout {
  size_t state, flags, last_change, scan, int_bits, unit_start, est0, est1, unit_first, coef, planes, total;
};

size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

// The one workspace layout.  The baseline path passes sync_intervals = intervals; the progressive path, which has no
// synchronisation stage, passes 0 for flag_words, sync_intervals and units: a region of size 0 takes no room (every
// offset is a multiple of 256), so its five live regions lie exactly where they would with those regions left out.
Layout layout(size_t n_images, size_t flag_words, size_t sync_intervals, size_t scan_bytes, size_t intervals,
              size_t units, size_t blocks, size_t plane_bytes) {
  Layout L;
  size_t o = 0;
  L.state = o; o = align256(o + sizeof(int) * kStateWords * n_images);
  L.flags = o; o = align256(o + sizeof(int) * flag_words);
  L.last_change = o; o = align256(o + sizeof(int) * sync_intervals);
  L.scan = o; o = align256(o + scan_bytes);
  L.int_bits = o; o = align256(o + sizeof(int) * intervals);
  L.unit_start = o; o = align256(o + sizeof(int) * sync_intervals);
  L.est0 = o; o = align256(o + sizeof(int4) * units);
  L.est1 = o; o = align256(o + sizeof(int4) * units);
  L.unit_first = o; o = align256(o + sizeof(int) * units);
  L.coef = o; o = align256(o + 128 * blocks);
  L.planes = o; o = align256(o + plane_bytes);
  L.total = o;
  return L;
}

Layout layout(const odic_jpeg_batch& b) {
  return layout(b.n_images, 2 + (size_t)b.max_sync_passes, b.total_intervals, b.total_scan_bytes, b.total_intervals,
                b.total_units, b.total_blocks, b.total_plane_bytes);
}

Layout layout(const odic_jpeg_prog_batch& b) {
  return layout(b.n_images, 0, 0, b.total_scan_bytes, b.total_intervals, 0, b.total_blocks, b.total_plane_bytes);
}

// A region of size 0 gets the address of the region behind it; no kernel of the path that passed 0 reads it.
Ws bind(void* workspace, const Layout& L) {
  unsigned char* base = (unsigned char*)workspace;
  Ws ws;
  ws.state = (int*)(base + L.state);
  ws.flags = (int*)(base + L.flags);
  ws.last_change = (int*)(base + L.last_change);
  ws.scan = base + L.scan;
  ws.int_bits = (int*)(base + L.int_bits);
  ws.unit_start = (int*)(base + L.unit_start);
  ws.est[0] = (int4*)(base + L.est0);
  ws.est[1] = (int4*)(base + L.est1);
  ws.unit_first = (int*)(base + L.unit_first);
  ws.coef = (short*)(base + L.coef);
  ws.planes = base + L.planes;
  return ws;
}

// The limits both batch descriptors share: grid dimensions that fit 16 bits, and something in every live region.
template <typename Batch>
bool batch_dims_ok(const Batch& b) {
  return b.n_images > 0 && b.n_images <= 65535 && b.max_width > 0 && b.max_width <= 65535 && b.max_height > 0 &&
         b.max_height <= 65535 && b.max_blocks > 0 && b.total_scan_bytes > 0 && b.total_intervals > 0 &&
         b.total_blocks > 0 && b.total_plane_bytes > 0;
}

// sampling 3 is a one-component (grayscale) frame: one 8x8 block per MCU in block-raster order, Huffman tables 0 (DC)
// and 3 (AC), quantisation table 0, a single plane and no colour conversion.
constexpr int kGray = 3;
__device__ __forceinline__ int blocks_per_mcu(int sampling) {
  return sampling == kGray ? 1 : (sampling == 0 ? 3 : (sampling == 1 ? 4 : 6));
}
__device__ __forceinline__ int luma_blocks(int sampling) {
  return sampling == 0 || sampling == kGray ? 1 : (sampling == 1 ? 2 : 4);
}
// luma blocks of an MCU across and down
__device__ __forceinline__ int luma_h(int sampling) { return sampling == 0 || sampling == kGray ? 1 : 2; }
__device__ __forceinline__ int luma_v(int sampling) { return sampling == 2 ? 2 : 1; }

// What the entropy kernels need of a frame: the blocks of an MCU and the component of each, which is also its Huffman
// table pair (DC table c, AC table kComps + c) and its DC predictor.  A common record derives both from `sampling`; a
// per-component one carries the sampling of every component, and the map from a block of the MCU to its component is
// packed from the record, two bits per block (at most 10 blocks).
constexpr int kMaxMcuBlocks = 10;                  // libjpeg's D_MAX_BLOCKS_IN_MCU

// The two record families: per-component records have ncomp, h[] and v[]; common ones have `sampling`.
template <typename Header, typename = void>
constexpr bool kPerComponent = false;
template <typename Header>
constexpr bool kPerComponent<Header, std::void_t<decltype(Header::ncomp)>> = true;
// When the colour pass writes an image's pixels.  A baseline record's are written whenever its frame rules hold (an
// image whose entropy data failed gets status 1 beside whatever its coefficients gave, as in the common family); a
// progressive per-component record's only when the whole decode succeeded — its state words are final by then, every
// kernel that sets them lies ahead of the colour kernel on the stream.
template <typename Header>
constexpr bool kPixelsOnlyWhenDecoded = std::is_same<Header, odic_jpeg_prog_header_any>::value;

// The frame rules of the per-component family, libjpeg's and the host parser's: three or four components; factors in
// 1..4, every factor a divisor of the largest in its direction, at most 10 blocks per MCU; four components: component 0
// at 1x1, 2x1 or 2x2 and every other one at 1x1 or at component 0's sampling, which the colour pass's plane addressing
// relies on.  A record that breaks them is a frame of one block of component 0 to the entropy kernels, which stay inside
// whatever the record's offsets span; the IDCT and the colour pass write nothing for it and the image gets status 1.
template <typename Header>
__device__ __forceinline__ bool layout_ok(const Header& h) {
  if (h.ncomp != 3 && h.ncomp != 4) return false;
  int hm = 1, vm = 1, n = 0;
  for (int c = 0; c < h.ncomp; ++c) {
    if ((unsigned)(h.h[c] - 1) > 3u || (unsigned)(h.v[c] - 1) > 3u) return false;
    hm = max(hm, h.h[c]);
    vm = max(vm, h.v[c]);
    n += h.h[c] * h.v[c];
  }
  if (n > kMaxMcuBlocks) return false;
  for (int c = 0; c < h.ncomp; ++c)
    if (hm % h.h[c] || vm % h.v[c]) return false;
  if (h.ncomp == 4) {
    if (h.h[0] > 2 || h.v[0] > h.h[0]) return false;
    for (int c = 1; c < 4; ++c)
      if ((h.h[c] != 1 || h.v[c] != 1) && (h.h[c] != h.h[0] || h.v[c] != h.v[0])) return false;
  }
  return true;
}
// blocks of an MCU; of a per-component record that layout_ok() admits
template <typename Header>
__device__ __forceinline__ int mcu_blocks(const Header& h) {
  if constexpr (kPerComponent<Header>) {
    int n = 0;
    for (int c = 0; c < h.ncomp; ++c) n += h.h[c] * h.v[c];
    return n;
  } else {
    return blocks_per_mcu(h.sampling);
  }
}

template <typename Header>
struct Frame;
template <>
struct Frame<odic_jpeg_header> {
  static constexpr int kComps = 3;
  int nY, bpm;
  __device__ explicit Frame(const odic_jpeg_header& h)
      : nY(luma_blocks(h.sampling)), bpm(blocks_per_mcu(h.sampling)) {}
  __device__ __forceinline__ int comp(int blk) const { return blk < nY ? 0 : blk - nY + 1; }
};
template <>
struct Frame<odic_jpeg_header_any> {
  static constexpr int kComps = 4;                   // table and predictor slots; a three-component file uses three
  unsigned map;
  int bpm;
  __device__ explicit Frame(const odic_jpeg_header_any& h) : map(0), bpm(0) {
    if (!layout_ok(h)) {
      bpm = 1;
      return;
    }
    for (int c = 0; c < h.ncomp; ++c)
      for (int j = 0; j < h.h[c] * h.v[c]; ++j) map |= (unsigned)c << (2 * bpm++);
  }
  __device__ __forceinline__ int comp(int blk) const { return (map >> (2 * blk)) & 3; }
};

// ---------------------------------------------------------------------------------------------------------------
// segment: one workgroup of 256 lanes per image, 16 bytes per lane per 4 KiB tile
// ---------------------------------------------------------------------------------------------------------------
template <typename T>
__device__ T block_exclusive_scan(T v, T* lds, T& total) {   // 256 lanes; lds holds 256 T
  const int t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const T x = t >= off ? lds[t - off] : T(0);
    __syncthreads();
    lds[t] += x;
    __syncthreads();
  }
  total = lds[255];
  const T incl = lds[t];
  __syncthreads();
  return incl - v;
}

// Classify and compact the bytes [src, src + len) of one scan into dst and record the start bit of every restart
// interval in ib[0 .. nint] (256 lanes).  want_eoi: the data must end with EOI inside the range (a baseline file is
// passed up to its last byte); otherwise the host parser has already cut the range at the scan's closing marker, and
// any marker other than RSTn inside it is an error.  Returns nonzero on an error; carry_data = compacted bytes.
__device__ int segment_bytes(const unsigned char* __restrict__ src, const long len, unsigned char* __restrict__ dst,
                             int* __restrict__ ib, const int nint, const bool want_eoi, long& carry_data,
                             int& carry_marks) {
  const int t = threadIdx.x;
  __shared__ int sh_scan[256];
  __shared__ long sh_stop;
  __shared__ int sh_err;
  carry_data = 0;
  carry_marks = 0;
  int err = 0;
  bool eoi = false, stopped = false;
  if (t == 0) sh_err = 0;
  for (long base = 0; base < len; base += 4096) {
    if (t == 0) sh_stop = len;
    __syncthreads();
    const long i0 = base + 16L * t;
    unsigned char bb[18];                                    // bytes i0 - 1 .. i0 + 16, 0 outside the scan
#pragma unroll
    for (int j = 0; j < 18; ++j) {
      const long i = i0 - 1 + j;
      bb[j] = (i >= 0 && i < len) ? src[i] : 0;
    }
    // the first stop (EOI or error) of the tile; a byte after 0xFF is the second byte of a pair
    for (int j = 0; j < 16; ++j) {
      const long i = i0 + j;
      if (i >= len) break;
      if (bb[j + 1] != 0xFF || bb[j] == 0xFF) continue;
      const int nx = i + 1 < len ? bb[j + 2] : -1;
      if (nx == 0 || (nx >= 0xD0 && nx <= 0xD7)) continue;
      atomicMin((unsigned long long*)&sh_stop, (unsigned long long)i);
      break;
    }
    __syncthreads();
    const long stop = sh_stop;
    int nd = 0, nm = 0;
    for (int j = 0; j < 16; ++j) {
      if (i0 + j >= stop) break;
      if (bb[j] == 0xFF) continue;
      if (bb[j + 1] != 0xFF || bb[j + 2] == 0) ++nd; else ++nm;
    }
    int tot_d, tot_m;
    int ed = block_exclusive_scan(nd, sh_scan, tot_d);
    int em = block_exclusive_scan(nm, sh_scan, tot_m);
    long d = carry_data + ed;
    int m = carry_marks + em;
    for (int j = 0; j < 16; ++j) {
      if (i0 + j >= stop) break;
      if (bb[j] == 0xFF) continue;
      if (bb[j + 1] != 0xFF || bb[j + 2] == 0) {
        dst[d++] = bb[j + 1];
      } else {                                               // RSTn ends interval m
        if (m + 1 >= nint || (bb[j + 2] & 7) != (m & 7)) sh_err = 1;   // too many, or out of sequence
        if (m + 1 < nint) ib[m + 1] = (int)(d * 8);
        ++m;
      }
    }
    carry_data += tot_d;
    carry_marks += tot_m;
    if (stop < len) {
      eoi = stop + 1 < len && src[stop + 1] == 0xD9;
      stopped = true;
      break;
    }
    __syncthreads();
  }
  __syncthreads();
  err = sh_err;
  if ((want_eoi ? !eoi : stopped) || carry_marks != nint - 1) err = 1;
  if (t == 0) ib[0] = 0;
  const int endbits = (int)(carry_data * 8);
  for (int k = min(carry_marks, nint - 1) + 1 + t; k <= nint; k += 256) ib[k] = endbits;   // end; missing: empty
  if (t < 16) dst[carry_data + t] = 0;
  __syncthreads();
  return err;
}

template <typename Header>                                      // odic_jpeg_header or odic_jpeg_header_any
__global__ __launch_bounds__(256) void jpeg_segment_kernel(const Header* __restrict__ hdrs,
                                                           const unsigned char* __restrict__ data, Ws ws,
                                                           int subseq_bits) {
  const Header& h = hdrs[blockIdx.x];
  const int t = threadIdx.x;
  int* ib = ws.int_bits + h.int_off;
  int* us = ws.unit_start + h.int_off;
  int* state = ws.state + kStateWords * blockIdx.x;
  const int nint = h.n_intervals;
  __shared__ int sh_scan[256];
  long carry_data;
  int carry_marks;
  const int err = segment_bytes(data + h.data_off, h.data_end - h.data_off, ws.scan + h.scan_off, ib, nint, true,
                                carry_data, carry_marks);
  if (t == 0 && err) state[0] |= kErrSegment;
  // units: interval k gets max(1, ceil(bits / subseq_bits)) of them
  int carry_u = 0;
  for (int k0 = 0; k0 < nint; k0 += 256) {
    const int k = k0 + t;
    int n = 0;
    if (k < nint) {
      const int bits = ib[k + 1] - ib[k];
      n = bits > 0 ? (bits + subseq_bits - 1) / subseq_bits : 1;
    }
    int tot;
    const int e = block_exclusive_scan(n, sh_scan, tot);
    if (k < nint) us[k] = carry_u + e;
    carry_u += tot;
  }
  if (t == 0) us[nint] = min(carry_u, h.n_units);                 // never more than the slots reserved
}

// ---------------------------------------------------------------------------------------------------------------
// Huffman decoding, shared by the speculative, sync, write-out and serial kernels
// ---------------------------------------------------------------------------------------------------------------
template <int kTables>             // 6 (common records: DC 0..2, AC 3..5) or 8 (per-component ones: DC 0..3, AC 4..7)
struct Tabs {
  unsigned short lut[kTables * 512];
  int lim[kTables * 8];            // [l - 9]: one past the last code of length <= l, left-justified to 16 bits
  int maxcode[kTables * 18];
  int valoff[kTables * 18];
  unsigned char huffval[kTables * 256];
  unsigned char natural[64];
};
template <typename Header>
using TabsOf = Tabs<2 * Frame<Header>::kComps>;

// canonical codes: the codes of length l, left-justified, end where those of l + 1 begin → lim[] of table `tab` (Tabs:
// one of six or eight; PTab: tab = 0)
__device__ __forceinline__ void fill_lim(const int* maxcode, int* lim, int tab) {
  int last = 0;
  for (int l = 1; l <= 16; ++l) {
    const int mc = maxcode[tab * 18 + l];
    if (mc >= 0) last = (mc + 1) << (16 - l);
    if (l >= 9) lim[tab * 8 + l - 9] = last;
  }
}

// The tables of the frame's components: all of a common record's; of a per-component record the pairs of components
// below ncomp, so a three-component file does not pay for the fourth pair.  The slots left out are never indexed:
// Frame::comp() is below ncomp for a frame layout_ok() admits and 0 for one it refuses.
template <typename Header, int kTables>
__device__ void load_tabs(const Header& h, Tabs<kTables>& T) {
  constexpr int kC = kTables / 2;
  const int t = threadIdx.x;
  constexpr bool kAll = !kPerComponent<Header>;
  int nc = kC;
  if constexpr (!kAll) nc = min(max(h.ncomp, 1), kC);
  for (int i = t; i < kTables * 512; i += blockDim.x)
    if (kAll || (i >> 9) % kC < nc) T.lut[i] = (&h.lut[0][0])[i];
  for (int i = t; i < kTables * 18; i += blockDim.x) {
    T.maxcode[i] = (&h.maxcode[0][0])[i];
    T.valoff[i] = (&h.valoff[0][0])[i];
  }
  for (int i = t; i < kTables * 256; i += blockDim.x)
    if (kAll || (i >> 8) % kC < nc) T.huffval[i] = (&h.huffval[0][0])[i];
  for (int i = t; i < 64; i += blockDim.x) T.natural[i] = kNatural[i];
  if (t < kTables) fill_lim(&h.maxcode[0][0], T.lim, t);
  __syncthreads();
}

struct St {
  int pos, blk, k;                 // next bit; block within the MCU; 0: next symbol is a DC, else the AC index
};

// Bit reader: the 64-bit window [32 wi, 32 wi + 64) in registers plus two prefetched words, so a symbol costs no
// memory access and a word is read 64 bits before it is needed.  w[i - off] holds compacted word i (the unit kernels
// stage their words in LDS, the serial walk reads global memory with off = 0).  Reads stop 16 bytes past the
// compacted data, inside the 16 bytes reserved behind every image's scan.
struct Bits {
  const unsigned* __restrict__ w;
  int off;
  int wi;
  unsigned w0, w1, w2, w3;
};

__device__ __forceinline__ void bits_seek(Bits& b, int pos) {
  b.wi = pos >> 5;
  const unsigned* p = b.w + (b.wi - b.off);
  b.w0 = __builtin_bswap32(p[0]);
  b.w1 = __builtin_bswap32(p[1]);
  b.w2 = __builtin_bswap32(p[2]);
  b.w3 = __builtin_bswap32(p[3]);
}

__device__ __forceinline__ unsigned bits_peek(Bits& b, int pos) {      // the 32 bits from `pos` (pos never decreases)
  while ((pos >> 5) > b.wi) {
    ++b.wi;
    b.w0 = b.w1;
    b.w1 = b.w2;
    b.w2 = b.w3;
    b.w3 = __builtin_bswap32(b.w[b.wi - b.off + 3]);
  }
  const unsigned long long x = ((unsigned long long)b.w0 << 32) | b.w1;
  return (unsigned)(x >> (32 - (pos & 31)));
}

template <typename Tab>          // Tabs: six or eight tables, `tab` picks one; PTab (the progressive path): one table, tab = 0
__device__ __forceinline__ int huff(const Tab& T, int tab, unsigned win, int& len) {
  const unsigned e = T.lut[tab * 512 + (win >> (32 - kLutBits))];
  if (e) {
    len = e >> 8;
    return e & 255;
  }
  // longer codes: the length is one more than the number of limits the 16-bit peek reaches (independent LDS reads
  // instead of a dependent loop that every lane of the wave would wait for)
  const int p16 = (int)(win >> 16);
  int l = kLutBits + 1;
#pragma unroll
  for (int i = 1; i <= 7; ++i) l += p16 >= T.lim[tab * 8 + i];
  if (l > 16) return -1;
  len = l;
  return T.huffval[tab * 256 + (((p16 >> (16 - l)) + T.valoff[tab * 18 + l]) & 255)];
}

__device__ __forceinline__ int extend(unsigned bits, int s) {    // HUFF_EXTEND
  return (int)bits < (1 << (s - 1)) ? (int)bits - (1 << s) + 1 : (int)bits;
}

// One symbol at s.pos.  zz = zig-zag index written (-1: none), val its value.  Returns false on an invalid code.
template <typename F>            // F: the Frame of the header type
__device__ __forceinline__ bool step(const Tabs<2 * F::kComps>& T, Bits& br, St& s, const F& f, int& zz, int& val) {
  const unsigned win = bits_peek(br, s.pos);
  const int comp = f.comp(s.blk);
  int len;
  if (s.k == 0) {
    const int cat = huff(T, comp, win, len);
    if (cat < 0) return false;
    val = cat ? extend((win << len) >> (32 - cat), cat) : 0;
    s.pos += len + cat;
    zz = 0;
    s.k = 1;
    return true;
  }
  const int rs = huff(T, F::kComps + comp, win, len);
  if (rs < 0) return false;
  const int r = rs >> 4, c = rs & 15;
  if (c) {
    s.k += r;
    zz = s.k;
    val = extend((win << len) >> (32 - c), c);
    s.pos += len + c;
    s.k += 1;
  } else {
    zz = -1;
    s.pos += len;
    s.k = r == 15 ? s.k + 16 : 64;
  }
  if (s.k >= 64) {
    s.k = 0;
    s.blk = s.blk + 1 == f.bpm ? 0 : s.blk + 1;
  }
  return true;
}

// decode [s.pos, end) counting the blocks begun; an invalid code ends the span with pos = kInvalidPos
template <typename F>
__device__ int4 decode_span(const Tabs<2 * F::kComps>& T, const unsigned* __restrict__ w, int off, St s, int end,
                            const F& f) {
  int count = 0;
  Bits br{w, off};
  if (s.pos < end) bits_seek(br, s.pos);
  while (s.pos < end) {
    count += s.k == 0;
    int zz, val;
    if (!step(T, br, s, f, zz, val)) {
      s = St{kInvalidPos, 0, 0};
      break;
    }
  }
  return make_int4(s.pos, s.blk, s.k, count);
}

struct Unit {
  int k, u, first, start, end, int_end;
};

// unit u of an image → its interval (binary search in unit_start) and bit range; false past the last unit
__device__ __forceinline__ bool locate(const int* __restrict__ us, const int* __restrict__ ib, int nint, int S, int u,
                                       Unit& U) {
  if (u >= us[nint]) return false;
  int lo = 0, hi = nint - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (us[mid] <= u) lo = mid; else hi = mid - 1;
  }
  U.k = lo;
  U.u = u;
  U.first = us[lo];
  U.int_end = ib[lo + 1];
  U.start = ib[lo] + (u - us[lo]) * S;
  U.end = min(U.start + S, U.int_end);
  return true;
}

constexpr int kUnitLanes = 64;                  // unit kernels: one wave per workgroup spreads a batch over more CUs
constexpr int kMaxSubseqBits = 4096;            // a workgroup's units are staged in LDS: 64 * 4096 bits = 32 KiB
// bit positions are int32: with at most 2^27 scan bytes every position, unit end (+ subseq_bits) and end state
// (+ 31 bits) stays below 2^30 + 2^13, far from kInvalidPos
constexpr long kMaxScanBytes = 1L << 27;

__host__ __device__ constexpr int stage_words(int S) { return kUnitLanes * S / 32 + 8; }

// Copy the compacted words the workgroup's units read (bits [lo, hi) plus the reader's 3 words of look-ahead) to
// LDS; returns the index of the first word staged.  Units are contiguous, so hi - lo <= 64 S.
__device__ int stage_units(const unsigned* __restrict__ gw, unsigned* sdata, bool valid, int start, int end) {
  __shared__ int sh_lo, sh_hi;
  if (threadIdx.x == 0) {
    sh_lo = 0x7fffffff;
    sh_hi = 0;
  }
  __syncthreads();
  if (valid) {
    atomicMin(&sh_lo, start);
    atomicMax(&sh_hi, end);
  }
  __syncthreads();
  const int lo = sh_lo, hi = sh_hi;
  if (lo > hi) return 0;                                          // no valid unit in this workgroup
  const int w_lo = lo >> 5, n = ((hi > 0 ? hi - 1 : 0) >> 5) + 3 - w_lo + 1;
  for (int i = threadIdx.x; i < n; i += kUnitLanes) sdata[i] = gw[w_lo + i];
  __syncthreads();
  return w_lo;
}

template <typename Header>
__global__ __launch_bounds__(kUnitLanes) void jpeg_sync_kernel(const Header* __restrict__ hdrs, Ws ws, int S,
                                                        int pass) {
  if (pass >= 2 && ws.flags[pass] == 0) return;                // pass - 1 changed nothing: converged
  __shared__ TabsOf<Header> T;
  const int img = blockIdx.y;
  const Header& h = hdrs[img];
  if (blockIdx.x * kUnitLanes >= h.n_units) return;
  if (pass >= 1 && threadIdx.x == 0) atomicMax(&ws.flags[0], pass);
  load_tabs(h, T);
  const int* us = ws.unit_start + h.int_off;
  const int* ib = ws.int_bits + h.int_off;
  Unit U{};
  const bool valid = locate(us, ib, h.n_intervals, S, blockIdx.x * kUnitLanes + threadIdx.x, U);
  extern __shared__ unsigned sdata[];
  const int off = stage_units((const unsigned*)(ws.scan + h.scan_off), sdata, valid, U.start, U.end);
  if (!valid) return;
  const Frame<Header> f(h);
  int4* out = ws.est[pass & 1] + h.unit_off;
  St s{U.start, 0, 0};
  if (pass >= 1 && U.u != U.first) {
    const int4 p = ws.est[(pass - 1) & 1][h.unit_off + U.u - 1];
    s = St{p.x, p.y, p.z};
  }
  const int4 e = decode_span(T, sdata, off, s, U.end, f);
  if (pass >= 1) {
    const int4 old = ws.est[(pass - 1) & 1][h.unit_off + U.u];
    if (old.x != e.x || old.y != e.y || old.z != e.z || old.w != e.w) {
      ws.flags[1 + pass] = 1;
      atomicMax(&ws.last_change[h.int_off + U.k], pass);
    }
  }
  out[U.u] = e;
}

// an interval's end states are exact once a pass changed none of them, or after jpeg_serial_kernel walked it (-1)
template <typename Header>
__device__ __forceinline__ bool converged(const Ws& ws, const Header& h, int k) {
  const int ran = ws.flags[0], last = ws.last_change[h.int_off + k];
  return last < 0 || (ran >= 1 && last < ran);
}

// per image: exclusive prefix of the blocks begun per unit (final pass buffer)
template <typename Header>
__global__ __launch_bounds__(256) void jpeg_block_scan_kernel(const Header* __restrict__ hdrs, Ws ws) {
  const Header& h = hdrs[blockIdx.x];
  __shared__ int sh[256];
  const int n = ws.unit_start[h.int_off + h.n_intervals];
  const int4* e = ws.est[ws.flags[0] & 1] + h.unit_off;
  int carry = 0;
  for (int u0 = 0; u0 < n; u0 += 256) {
    const int u = u0 + threadIdx.x;
    const int v = u < n ? e[u].w : 0;
    int tot;
    const int x = block_exclusive_scan(v, sh, tot);
    if (u < n) ws.unit_first[h.unit_off + u] = carry + x;
    carry += tot;
  }
}

// decode from s to `end` (or the interval's last block) writing coefficients; bcur = block in progress (local)
template <typename F>
__device__ void write_span(const Tabs<2 * F::kComps>& T, const unsigned* __restrict__ w, int off, St s, int bcur, int end,
                           int int_end, int nblk, short* __restrict__ coef, const F& f, int* state) {
  Bits br{w, off};
  if (s.pos < end) bits_seek(br, s.pos);
  while (s.pos < end) {
    const int nb = s.k == 0 ? bcur + 1 : bcur;
    if (nb >= nblk) return;                                   // past the interval's last block: padding
    int zz, val;
    if (nb < 0 || !step(T, br, s, f, zz, val) || zz > 63) {   // zz > 63: libjpeg would clobber coef 63
      atomicOr(&state[0], kErrDecode);
      return;
    }
    bcur = nb;
    if (zz >= 0) coef[(long)bcur * 64 + T.natural[zz]] = (short)val;
    if (s.k == 0 && bcur == nblk - 1) {                       // the interval's last block is complete
      if (s.pos > int_end) atomicOr(&state[0], kErrDecode);   // its MCUs needed bits past the interval
      else atomicAdd(&state[1], 1);
      return;
    }
  }
  // the unit's bits are used up; the interval's completion is counted by the unit that finishes it
}

template <typename Header>
__device__ __forceinline__ int interval_blocks(const Header& h, int k, int bpm) {
  const int nmcu = h.mcus_x * h.mcus_y;
  return min(h.restart, nmcu - k * h.restart) * bpm;
}

template <typename Header>
__global__ __launch_bounds__(kUnitLanes) void jpeg_writeout_kernel(const Header* __restrict__ hdrs, Ws ws, int S) {
  __shared__ TabsOf<Header> T;
  const int img = blockIdx.y;
  const Header& h = hdrs[img];
  if (blockIdx.x * kUnitLanes >= h.n_units) return;
  load_tabs(h, T);
  const int* us = ws.unit_start + h.int_off;
  const int* ib = ws.int_bits + h.int_off;
  Unit U{};
  const bool valid = locate(us, ib, h.n_intervals, S, blockIdx.x * kUnitLanes + threadIdx.x, U);
  extern __shared__ unsigned sdata[];
  const int off = stage_units((const unsigned*)(ws.scan + h.scan_off), sdata, valid, U.start, U.end);
  if (!valid) return;
  const Frame<Header> f(h);
  const int bpm = f.bpm;
  St s{U.start, 0, 0};
  if (U.u != U.first) {
    const int4 p = ws.est[ws.flags[0] & 1][h.unit_off + U.u - 1];
    s = St{p.x, p.y, p.z};
  }
  const int* uf = ws.unit_first + h.unit_off;
  const int bcur = uf[U.u] - uf[U.first] - 1;
  short* coef = ws.coef + (h.coef_off + (long)U.k * h.restart * bpm) * 64;
  write_span(T, sdata, off, s, bcur, U.end, U.int_end, interval_blocks(h, U.k, bpm), coef, f,
             ws.state + kStateWords * img);
}

// One wave per interval that did not converge: walk its units in order from the interval's exact start.  A unit whose
// start state in the last pass equals the walker's state kept a correct end state and is stepped over; any other unit
// is decoded again from the walker's state.  The wave loads 64 units' states at a time and broadcasts them; all lanes
// decode redundantly (same state, same addresses).  With max_sync_passes = 0 this is a serial decode of each interval.
template <typename Header>
__global__ __launch_bounds__(64) void jpeg_serial_kernel(const Header* __restrict__ hdrs, Ws ws, int S) {
  __shared__ TabsOf<Header> T;
  const int img = blockIdx.y, k = blockIdx.x;
  const Header& h = hdrs[img];
  if (k >= h.n_intervals || converged(ws, h, k)) return;
  load_tabs(h, T);
  const int* ib = ws.int_bits + h.int_off;
  const int* us = ws.unit_start + h.int_off;
  const int ran = ws.flags[0];
  int4* cur = ws.est[ran & 1] + h.unit_off;
  const int4* prev = ws.est[(ran - 1) & 1] + h.unit_off;
  const unsigned* w = (const unsigned*)(ws.scan + h.scan_off);
  const Frame<Header> f(h);
  const int lane = threadIdx.x, u_end = us[k + 1];
  St s{ib[k], 0, 0};
  for (int u0 = us[k]; u0 < u_end; u0 += 64) {
    const int u = u0 + lane;
    int4 rec = make_int4(ib[k] + (u - us[k]) * S, 0, 0, 0), e = make_int4(0, 0, 0, 0);   // start unit u was decoded from
    if (u < u_end) {
      if (ran >= 1 && u != us[k]) rec = prev[u - 1];
      e = cur[u];
    }
    for (int j = 0; j < 64 && u0 + j < u_end; ++j) {
      const int rp = __shfl(rec.x, j), rb = __shfl(rec.y, j), rk = __shfl(rec.z, j);
      const int ep = __shfl(e.x, j), eb = __shfl(e.y, j), ek = __shfl(e.z, j);
      if (rp == s.pos && rb == s.blk && rk == s.k) {
        s = St{ep, eb, ek};
      } else {
        const int start = ib[k] + (u0 + j - us[k]) * S;
        const int4 d = decode_span(T, w, 0, s, min(start + S, ib[k + 1]), f);
        if (lane == 0) cur[u0 + j] = d;
        s = St{d.x, d.y, d.z};
      }
    }
  }
  if (lane == 0) ws.last_change[h.int_off + k] = -1;        // its end states are now exact
}

// ---------------------------------------------------------------------------------------------------------------
// DC prediction: per image, one lane per MCU, a segmented scan of the components' differences (three or four)
// ---------------------------------------------------------------------------------------------------------------
template <typename Header>
__global__ __launch_bounds__(256) void jpeg_dc_kernel(const Header* __restrict__ hdrs, Ws ws) {
  const Header& h = hdrs[blockIdx.x];
  const int t = threadIdx.x;
  constexpr int kC = Frame<Header>::kComps;
  const Frame<Header> fr(h);                                 // gray: one predictor, every block is component 0
  const int bpm = fr.bpm;
  const int nmcu = h.mcus_x * h.mcus_y, R = h.restart;
  short* coef = ws.coef + h.coef_off * 64;
  __shared__ int sv[kC][256];
  __shared__ int sf[256];
  int carry[kC] = {};
  for (int m0 = 0; m0 < nmcu; m0 += 256) {
    const int m = m0 + t;
    int own[kC] = {};
    if (m < nmcu) {
      for (int j = 0; j < bpm; ++j) own[fr.comp(j)] += coef[((long)m * bpm + j) * 64];
    }
    int f = m % R == 0;
    int v[kC];
    for (int c = 0; c < kC; ++c) v[c] = own[c] + (t == 0 && !f ? carry[c] : 0);
    for (int off = 1; off < 256; off <<= 1) {
      for (int c = 0; c < kC; ++c) sv[c][t] = v[c];
      sf[t] = f;
      __syncthreads();
      if (t >= off && !f) {
        for (int c = 0; c < kC; ++c) v[c] += sv[c][t - off];
        f = sf[t - off];
      }
      __syncthreads();
    }
    if (m < nmcu) {
      int run[kC];
      for (int c = 0; c < kC; ++c) run[c] = v[c] - own[c];
      for (int j = 0; j < bpm; ++j) {
        const int c = fr.comp(j);
        short* p = &coef[((long)m * bpm + j) * 64];
        run[c] += *p;
        if (run[c] < -32768 || run[c] > 32767) atomicOr(&ws.state[kStateWords * blockIdx.x], kErrRange);
        *p = (short)run[c];                                  // JCOEF is a short
      }
    }
    for (int c = 0; c < kC; ++c) sv[c][t] = v[c];
    __syncthreads();
    for (int c = 0; c < kC; ++c) carry[c] = sv[c][255];
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------
// ISLOW IDCT (jidctint.c): 8 lanes per block, column pass → LDS → row pass
// ---------------------------------------------------------------------------------------------------------------
constexpr int FIX_0_298631336 = 2446, FIX_0_390180644 = 3196, FIX_0_541196100 = 4433, FIX_0_765366865 = 6270,
              FIX_0_899976223 = 7373, FIX_1_175875602 = 9633, FIX_1_501321110 = 12299, FIX_1_847759065 = 15137,
              FIX_1_961570560 = 16069, FIX_2_053119869 = 16819, FIX_2_562915447 = 20995, FIX_3_072711026 = 25172;

__device__ __forceinline__ void idct_1d(const int* in, int* out, int shift) {
  int z2 = in[2], z3 = in[6];
  int z1 = (z2 + z3) * FIX_0_541196100;
  const int tmp2 = z1 - z3 * FIX_1_847759065;
  const int tmp3 = z1 + z2 * FIX_0_765366865;
  const int tmp0 = (in[0] + in[4]) * (1 << 13);
  const int tmp1 = (in[0] - in[4]) * (1 << 13);
  const int t10 = tmp0 + tmp3, t13 = tmp0 - tmp3, t11 = tmp1 + tmp2, t12 = tmp1 - tmp2;
  int t0 = in[7], t1 = in[5], t2 = in[3], t3 = in[1];
  z1 = t0 + t3; z2 = t1 + t2; z3 = t0 + t2;
  int z4 = t1 + t3;
  const int z5 = (z3 + z4) * FIX_1_175875602;
  t0 *= FIX_0_298631336; t1 *= FIX_2_053119869; t2 *= FIX_3_072711026; t3 *= FIX_1_501321110;
  z1 *= -FIX_0_899976223; z2 *= -FIX_2_562915447;
  z3 = z3 * -FIX_1_961570560 + z5;
  z4 = z4 * -FIX_0_390180644 + z5;
  t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
  const int r = 1 << (shift - 1);
  out[0] = (t10 + t3 + r) >> shift; out[7] = (t10 - t3 + r) >> shift;
  out[1] = (t11 + t2 + r) >> shift; out[6] = (t11 - t2 + r) >> shift;
  out[2] = (t12 + t1 + r) >> shift; out[5] = (t12 - t1 + r) >> shift;
  out[3] = (t13 + t0 + r) >> shift; out[4] = (t13 - t0 + r) >> shift;
}

__device__ __forceinline__ unsigned range_limit(int x) {   // IDCT_range_limit[x & RANGE_MASK] (jdmaster.c table)
  const int s = ((x + 512) & 1023) - 512 + 128;
  return (unsigned)(s < 0 ? 0 : (s > 255 ? 255 : s));
}

// The reduced transforms of a scaled decode (jidctred.c jpeg_idct_4x4 / jpeg_idct_2x2; libjpeg's scale_denom 2, 4, 8):
// the same two passes on fewer inputs.  4x4 never reads column 4 or row 4; 2x2 reads columns and rows 0, 1, 3, 5, 7.
__device__ __forceinline__ void idct4_1d(const int* in, int* out, int shift) {
  const int t0 = in[0] * (1 << 14);
  const int t2 = in[2] * FIX_1_847759065 - in[6] * FIX_0_765366865;
  const int t10 = t0 + t2, t12 = t0 - t2;
  const int z1 = in[7], z2 = in[5], z3 = in[3], z4 = in[1];
  const int o0 = -z1 * 1730 + z2 * 11893 - z3 * 17799 + z4 * 8697;
  const int o2 = -z1 * 4176 - z2 * 4926 + z3 * FIX_0_899976223 + z4 * FIX_2_562915447;
  const int r = 1 << (shift - 1);
  out[0] = (t10 + o2 + r) >> shift; out[3] = (t10 - o2 + r) >> shift;
  out[1] = (t12 + o0 + r) >> shift; out[2] = (t12 - o0 + r) >> shift;
}

__device__ __forceinline__ void idct2_1d(const int* in, int* out, int shift) {
  const int t10 = in[0] * (1 << 15);
  const int t0 = -in[7] * 5906 + in[5] * 6967 - in[3] * 10426 + in[1] * 29692;
  const int r = 1 << (shift - 1);
  out[0] = (t10 + t0 + r) >> shift;
  out[1] = (t10 - t0 + r) >> shift;
}

// Transform size of the luma (ny) and chroma (nc) blocks at scale 1 / 2^lg (jdmaster.c: every component starts at
// 8 >> lg and doubles while that keeps it on the luma grid in both directions).  Only 4:2:0 chroma doubles: it then
// shares the luma's grid and is not upsampled; 4:2:2 chroma fails the vertical test and stays.
__device__ __forceinline__ void scaled_sizes(int sampling, int lg, int& ny, int& nc) {
  ny = 8 >> lg;
  nc = (sampling == 2 && lg > 0) ? 2 * ny : ny;
}

// The same rule for a component of a frame with per-component sampling (hc, vc; hm, vm: the frame's largest factors):
// doubling must keep the block on the largest component's grid in both directions.  4:2:0 chroma at 1/2 reaches 8,
// 4:2:2 chroma stays, 4:1:1 chroma never doubles; lg = 0 gives 8.  The factors are clamped to 1..4, which changes
// nothing for a record the parser made and keeps one that breaks its rules away from a zero divisor.
__device__ __forceinline__ int factor14(int f) { return min(max(f, 1), 4); }
__device__ __forceinline__ int scaled_size_own(int hc, int vc, int hm, int vm, int lg) {
  const int mn = 8 >> lg;
  int n = mn;
  while (n < 8 && (hm * mn) % (hc * n * 2) == 0 && (vm * mn) % (vc * n * 2) == 0) n *= 2;
  return n;
}

// row / column i is an input of the n-point transform
__device__ __forceinline__ bool idct_reads(int n, int i) {
  return n == 8 || (n == 4 ? i != 4 : (n == 2 ? (i < 2 || (i & 1)) : i == 0));
}

// Where block j of an MCU goes: its component, the transform size n, the component's blocks per MCU across and down
// (hc, vc), the block's place among them (jx, jy) and the byte offset of the component's plane.  Every plane is
// mcus_x·n·hc wide and mcus_y·n·vc high, padded to whole MCUs.
struct BlockGeo {
  int comp, n, hc, vc, jx, jy;
  long plane;
};
// every component with its own sampling (the per-component records, kC = ncomp): the planes follow
// each other in component order, plane c at the component's transform size n (8 at full size), each rounded up to a
// multiple of 16 bytes, which a plane of 8x8 blocks is anyway and which keeps the n-aligned row stores of the IDCT
// aligned behind a plane of 1x1 or 2x2 blocks
template <typename Header>
__device__ __forceinline__ long plane_bytes_own(const Header& h, int c, int n) {
  return ((long)h.mcus_x * n * h.h[c] * h.mcus_y * n * h.v[c] + 15) & ~15L;
}
// the largest factors of the record's first kC components, each clamped to 1..4
template <int kC, typename Header>
__device__ __forceinline__ void largest_factors(const Header& h, int& hm, int& vm) {
  hm = vm = 1;
  for (int c = 0; c < kC; ++c) {
    hm = max(hm, factor14(h.h[c]));
    vm = max(vm, factor14(h.v[c]));
  }
}
template <int kC, typename Header>
__device__ __forceinline__ BlockGeo block_geo_own(const Header& h, int j, int lg) {
  int hm = 1, vm = 1;
  if (lg) largest_factors<kC>(h, hm, vm);
  BlockGeo g{kC - 1, 8, h.h[kC - 1], h.v[kC - 1], 0, 0, 0};
  for (int c = 0; c < kC; ++c) {
    const int n = lg ? scaled_size_own(factor14(h.h[c]), factor14(h.v[c]), hm, vm, lg) : 8;
    const int nb = h.h[c] * h.v[c];
    if (j < nb || c == kC - 1) {
      g.comp = c; g.n = n; g.hc = h.h[c]; g.vc = h.v[c]; g.jx = j % g.hc; g.jy = min(j / g.hc, g.vc - 1);
      break;
    }
    j -= nb;
    g.plane += plane_bytes_own(h, c, n);
  }
  return g;
}
// Block j of an MCU of any record at scale 1 / 2^lg (kScaled = false: lg = 0).  A common record: component 0 at the
// luma sampling with transform size ny, the others 1x1 with size nc.
template <bool kScaled, typename Header>
__device__ __forceinline__ BlockGeo block_geo(const Header& h, int j, int lg) {
  if constexpr (kPerComponent<Header>) {
    return h.ncomp == 4 ? block_geo_own<4>(h, j, kScaled ? lg : 0) : block_geo_own<3>(h, j, kScaled ? lg : 0);
  } else {
    int ny = 8, nc = 8;
    if constexpr (kScaled) scaled_sizes(h.sampling, lg, ny, nc);
    const int nY = luma_blocks(h.sampling), hy = luma_h(h.sampling), vy = luma_v(h.sampling);
    BlockGeo g;
    g.comp = j < nY ? 0 : j - nY + 1;
    if (g.comp == 0) {
      g.n = ny; g.hc = hy; g.vc = vy; g.jx = j % hy; g.jy = j / hy; g.plane = 0;
    } else {
      const long ysz = (long)h.mcus_x * ny * hy * h.mcus_y * ny * vy, csz = (long)h.mcus_x * nc * h.mcus_y * nc;
      g.n = nc; g.hc = 1; g.vc = 1; g.jx = 0; g.jy = 0; g.plane = ysz + (g.comp - 1) * csz;
    }
    return g;
  }
}
// One block per 8 lanes: column pass → LDS → row pass, n×n samples into the component's plane.  kScaled = false is
// the full-size decode (lg = 0, n = 8 throughout, the branches below fold away).  A scaled image's planes keep the
// full-size order (Y, Cb, Cr from plane_off) with every block n wide and high.  The range rule of kIdctLimit holds for
// the reduced transforms as it stands: on the inputs a transform reads, its pass-1 values and its results (1x1 has
// only the input and the result).  libjpeg-turbo's SIMD 4x4 / 2x2 keep the same 16-bit intermediates as its 8x8.
template <bool kScaled, typename Header>
__device__ __forceinline__ void idct_blocks(const Header& h, const Ws& ws, int img, int lg, int (*ws8)[8][9]) {
  if constexpr (kPerComponent<Header>) {
    if (!layout_ok(h)) return;                                // the whole workgroup: one image per blockIdx.y
  }
  const int bpm = mcu_blocks(h);                              // gray: every block is component 0
  const long nblocks = (long)h.mcus_x * h.mcus_y * bpm;
  const long b = (long)blockIdx.x * 32 + (threadIdx.x >> 3);
  const int lane = threadIdx.x & 7, slot = threadIdx.x >> 3;
  if ((long)blockIdx.x * 32 >= nblocks) return;
  const bool live = b < nblocks;
  const int j = (int)(live ? b % bpm : 0);
  const BlockGeo g = block_geo<kScaled>(h, j, lg);
  const int comp = g.comp, n = g.n;
  bool outside = false;                                       // a value where libjpeg-turbo's SIMD and C IDCTs part
  if (live && idct_reads(n, lane)) {                          // column `lane`
    const short* c = ws.coef + (h.coef_off + b) * 64;
    int in[8], out[8];
    for (int r = 0; r < 8; ++r) {
      in[r] = idct_reads(n, r) ? (int)c[r * 8 + lane] * (int)h.qt[comp][r * 8 + lane] : 0;
      if (in[r] < -kIdctLimit || in[r] > kIdctLimit) {
        outside = true;
        in[r] = 0;                                            // keeps the int32 arithmetic in range; image is redone
      }
    }
    if (n == 8) idct_1d(in, out, 13 - 2);
    else if (n == 4) idct4_1d(in, out, 13 - 2 + 1);
    else if (n == 2) idct2_1d(in, out, 13 - 2 + 2);
    else out[0] = in[0];                                      // 1x1: DESCALE(in0, 3) below, no pass 1
    for (int r = 0; r < 8; ++r) {
      if (r >= n) break;
      if (out[r] < -kIdctLimit || out[r] > kIdctLimit) {
        outside = true;
        out[r] = 0;
      }
      ws8[slot][r][lane] = out[r];
    }
  }
  __syncthreads();
  if (!live) return;
  int in[8], out[8];                                          // row `lane`
  if (lane < n) {
    for (int x = 0; x < 8; ++x) in[x] = idct_reads(n, x) ? ws8[slot][lane][x] : 0;
    if (n == 8) idct_1d(in, out, 13 + 2 + 3);
    else if (n == 4) idct4_1d(in, out, 13 + 2 + 3 + 1);
    else if (n == 2) idct2_1d(in, out, 13 + 2 + 3 + 2);
    else out[0] = (in[0] + 4) >> 3;
    for (int x = 0; x < 8; ++x) outside |= x < n && (out[x] < -512 || out[x] > 511);
  }
  if (outside) atomicOr(&ws.state[kStateWords * img], kErrRange);
  if (lane >= n) return;
  const long mcu = b / bpm;
  const int mx = (int)(mcu % h.mcus_x), my = (int)(mcu / h.mcus_x);
  const int bx = mx * g.hc + g.jx, by = my * g.vc + g.jy, pw = h.mcus_x * n * g.hc;
  unsigned char* plane = ws.planes + h.plane_off + g.plane;
  unsigned char* row = plane + (long)(by * n + lane) * pw + bx * n;
  if (n == 8) {
    uint2 v;
    v.x = range_limit(out[0]) | range_limit(out[1]) << 8 | range_limit(out[2]) << 16 | range_limit(out[3]) << 24;
    v.y = range_limit(out[4]) | range_limit(out[5]) << 8 | range_limit(out[6]) << 16 | range_limit(out[7]) << 24;
    *(uint2*)row = v;
  } else if (n == 4) {                                        // every row of an n-wide block is n-aligned: plane sizes and
    *(unsigned*)row =                                         // row pitches are multiples of 16 n / 4, plane_off of 16
        range_limit(out[0]) | range_limit(out[1]) << 8 | range_limit(out[2]) << 16 | range_limit(out[3]) << 24;
  } else if (n == 2) {
    *(unsigned short*)row = (unsigned short)(range_limit(out[0]) | range_limit(out[1]) << 8);
  } else {
    row[0] = (unsigned char)range_limit(out[0]);
  }
}

template <typename Header>                                      // odic_jpeg_header or odic_jpeg_prog_header
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const Header* __restrict__ hdrs, Ws ws) {
  __shared__ int ws8[32][8][9];
  idct_blocks<false>(hdrs[blockIdx.y], ws, blockIdx.y, 0, ws8);
}

// scale_log2[image] = 0..3: decode at 1 / 2 / 4 / 8 of the frame's size.  The caller vouches for the range; a value
// outside it is kept away from the shifts and the plane geometry (the image is left undecoded, with status 1).
template <typename Header>
__global__ __launch_bounds__(256) void jpeg_idct_scaled_kernel(const Header* __restrict__ hdrs, Ws ws,
                                                               const int* __restrict__ scale_log2) {
  __shared__ int ws8[32][8][9];
  const int lg = scale_log2[blockIdx.y];
  if ((unsigned)lg > 3u) return;
  idct_blocks<true>(hdrs[blockIdx.y], ws, blockIdx.y, lg, ws8);
}

// ---------------------------------------------------------------------------------------------------------------
// fancy upsampling + YCbCr→RGB (jdsample.c h2v1/h2v2_fancy_upsample, jdcolor.c ycc_rgb_convert) + status
// ---------------------------------------------------------------------------------------------------------------
constexpr int kCrR = 91881, kCbB = 116130, kCrG = 46802, kCbG = 22554;   // FIX(1.402), FIX(1.772), FIX(.71414), FIX(.34414)

__device__ __forceinline__ unsigned char clamp255(int v) { return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// jdsample.c: one sample of a plane with half the output's width (and, v2, half its height) at output pixel (x, y).
// dw, dh: the plane's own width and height in samples (the clamp at the image's edges); plain: replication in both
// directions instead of the triangle filters h2v1_fancy_upsample / h2v2_fancy_upsample.
__device__ __forceinline__ int upsampled(const unsigned char* __restrict__ P, int cw, int x, int y, bool v2, bool plain,
                                         int dw, int dh) {
  const int c = x >> 1, odd = x & 1;
  const int cn = odd ? min(c + 1, dw - 1) : max(c - 1, 0);
  if (plain) return P[(long)(v2 ? y >> 1 : y) * cw + c];
  if (!v2) {
    const long r = (long)y * cw;
    return (3 * P[r + c] + P[r + cn] + 1 + odd) >> 2;
  }
  const int rr = y >> 1;
  const int rn = (y & 1) ? min(rr + 1, dh - 1) : max(rr - 1, 0);
  const long r0 = (long)rr * cw, r1 = (long)rn * cw;
  const int s0 = 3 * P[r0 + c] + P[r1 + c], s1 = 3 * P[r0 + cn] + P[r1 + cn];
  return (3 * s0 + s1 + 8 - odd) >> 4;
}

// jdcolor.c ycc_rgb_convert on one pixel, cb and cr as stored
__device__ __forceinline__ void ycc_rgb_pixel(int yv, int cb, int cr, unsigned char* __restrict__ o) {
  cb -= 128;
  cr -= 128;
  o[0] = clamp255(yv + ((kCrR * cr + 32768) >> 16));
  o[1] = clamp255(yv + ((-kCbG * cb + 32768 - kCrG * cr) >> 16));
  o[2] = clamp255(yv + ((kCbB * cb + 32768) >> 16));
}

// jdsample.c jinit_upsampler for any component: one sample at output pixel (x, y) of a plane with 1 / rh of the
// output's width and 1 / rv of its height, dw x dh real samples.  (1, 1) is the plane itself; (2, 1) and (2, 2) are
// upsampled() above, fancy unless the plane is at most two samples wide; (1, 2) is h1v2_fancy_upsample at every width:
// three parts of the nearer row and one of the farther, the row above for an upper output row (bias 1) and below for a
// lower one (bias 2), the plane's first and last real rows standing in for the rows outside it; every other integral
// ratio is int_upsample: replication.  fancy = false (a scaled decode whose smallest transform is 1x1, where jdsample.c
// drops the triangle filters): replication at every ratio.
__device__ __forceinline__ int upsampled_by(const unsigned char* __restrict__ P, int cw, int x, int y, int rh, int rv,
                                            int dw, int dh, bool fancy = true) {
  if (rh == 2 && rv <= 2) return upsampled(P, cw, x, y, rv == 2, dw <= 2 || !fancy, dw, dh);
  if (rh == 1 && rv == 2 && fancy) {
    const int r = y >> 1, odd = y & 1;
    const int rn = odd ? min(r + 1, dh - 1) : max(r - 1, 0);
    return (3 * P[(long)r * cw + x] + P[(long)rn * cw + x] + 1 + odd) >> 2;
  }
  return P[(long)(y / rv) * cw + x / rh];
}

// One output pixel.  kScaled = false is the full-size decode (lg = 0).  At scale 1 / 2^lg the output is
// ceil(W / 2^lg) × ceil(H / 2^lg) and the planes hold the transform sizes of scaled_sizes(): 4:4:4 and, for lg > 0,
// 4:2:0 read chroma on the luma grid; 4:2:2 upsamples horizontally (jdsample.c): fancy while the chroma transform is
// larger than 1x1 and the component's downsampled width ceil(W·nc / 16) is above 2, else by replication.  The width
// rule holds at full size too, for 4:2:2 and 4:2:0 alike: chroma at most two samples wide (a frame at most 4 pixels
// wide) is replicated in both directions, without the triangle filter.
template <bool kScaled, typename Header>
__device__ __forceinline__ void color_pixel(const Header& h, const Ws& ws, int img, int lg,
                                            unsigned char* __restrict__ out, int* __restrict__ status) {
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x == 0 && y == 0) {
    const int* st = ws.state + kStateWords * img;
    status[img] = (st[0] == 0 && st[1] == h.n_intervals) ? 0 : 1;
  }
  const int round = (1 << lg) - 1;
  const int W = kScaled ? (h.width + round) >> lg : h.width, H = kScaled ? (h.height + round) >> lg : h.height;
  if (x >= W || y >= H) return;
  const int sampling = h.sampling, hy = luma_h(sampling), vy = luma_v(sampling);
  int ny = 8, nc = 8;
  if (kScaled) scaled_sizes(sampling, lg, ny, nc);
  const int yw = h.mcus_x * ny * hy, cw = h.mcus_x * nc;
  const unsigned char* Y = ws.planes + h.plane_off;
  const unsigned char* Cb = Y + (long)yw * h.mcus_y * ny * vy;
  const unsigned char* Cr = Cb + (long)cw * h.mcus_y * nc;
  const int yv = Y[(long)y * yw + x];
  unsigned char* o = out + h.out_off + ((long)y * W + x) * 3;
  if (sampling == kGray) {                                    // the one plane is the image: Pillow's L → RGB
    o[0] = o[1] = o[2] = (unsigned char)yv;
    return;
  }
  int cb, cr;
  if (sampling == 0 || (kScaled && sampling == 2 && lg > 0)) {
    cb = Cb[(long)y * cw + x];
    cr = Cr[(long)y * cw + x];
  } else {
    const int dw = kScaled ? (h.width * nc + 15) >> 4 : (W + 1) >> 1;      // the same number at lg = 0
    // jdsample.c: h2v1_upsample / h2v2_upsample, no filter in either direction, for chroma at most two samples wide
    // (a frame at most 4 pixels wide) or a 1x1 chroma transform
    const bool plain = dw <= 2 || (kScaled && nc == 1);
    cb = upsampled(Cb, cw, x, y, sampling == 2, plain, dw, (H + 1) >> 1);
    cr = upsampled(Cr, cw, x, y, sampling == 2, plain, dw, (H + 1) >> 1);
  }
  ycc_rgb_pixel(yv, cb, cr, o);
}

template <typename Header>
__global__ __launch_bounds__(256) void jpeg_color_kernel(const Header* __restrict__ hdrs, Ws ws,
                                                         unsigned char* __restrict__ out, int* __restrict__ status) {
  color_pixel<false>(hdrs[blockIdx.z], ws, blockIdx.z, 0, out, status);
}

template <typename Header>
__global__ __launch_bounds__(256) void jpeg_color_scaled_kernel(const Header* __restrict__ hdrs, Ws ws,
                                                                const int* __restrict__ scale_log2,
                                                                unsigned char* __restrict__ out,
                                                                int* __restrict__ status) {
  const int img = blockIdx.z, lg = scale_log2[img];
  if ((unsigned)lg > 3u) {                                    // not a scale: nothing was decoded, nothing is written
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && threadIdx.y == 0) status[img] = 1;
    return;
  }
  color_pixel<true>(hdrs[img], ws, img, lg, out, status);
}

// ---------------------------------------------------------------------------------------------------------------
// The colour pass of the per-component records.  Four components: what Image.open(f).convert("RGB") makes of a CMYK /
// YCCK file.
//   jdcolor.c ycck_cmyk_convert (Adobe transform 2): C, M, Y = 255 - (R, G, B) of the table-driven YCbCr→RGB above,
//       K as stored; other files hold C, M, Y, K as stored
//   Pillow's unpacker "CMYK;I", which JpegImagePlugin picks for every four-layer file: each sample becomes 255 - x
//   Pillow's Convert.c cmyk2rgb: per channel x with nk = 255 - K, t = x·nk + 128, out = clip(nk - (((t >> 8) + t) >> 8))
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void cmyk_pixel_rgb(int c, int m, int y, int k, int invert, unsigned char* __restrict__ o) {
  if (invert) {
    c = 255 - c; m = 255 - m; y = 255 - y; k = 255 - k;
  }
  const int nk = 255 - k;
  const int v[3] = {c, m, y};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int t = v[i] * nk + 128;
    o[i] = clamp255(nk - (((t >> 8) + t) >> 8));
  }
}

// n <= 4 pixels (3 n bytes) to o: three 32-bit stores where there are four pixels and o is 4-aligned, else bytes
__device__ __forceinline__ void store_rgb4(unsigned char* __restrict__ o, const unsigned char* px, int n) {
  if (n == 4 && ((size_t)o & 3) == 0) {
    unsigned* q = (unsigned*)o;
#pragma unroll
    for (int i = 0; i < 3; ++i) q[i] = px[4 * i] | px[4 * i + 1] << 8 | px[4 * i + 2] << 16 | (unsigned)px[4 * i + 3] << 24;
  } else {
    for (int i = 0; i < 3 * n; ++i) o[i] = px[i];
  }
}

constexpr int kColor4Pixels = 4;                   // pixels per lane of the kernels below

__global__ __launch_bounds__(256) void cmyk_to_rgb8_kernel(const unsigned char* __restrict__ cmyk,
                                                           unsigned char* __restrict__ rgb, long n_pixels, int invert) {
  const long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * kColor4Pixels;
  if (p0 >= n_pixels) return;
  const int n = (int)min((long)kColor4Pixels, n_pixels - p0);
  unsigned char in[4 * kColor4Pixels], px[3 * kColor4Pixels];
  const unsigned char* src = cmyk + 4 * p0;
  if (n == kColor4Pixels && ((size_t)src & 15) == 0) {
    *(uint4*)in = *(const uint4*)src;
  } else {
    for (int i = 0; i < 4 * n; ++i) in[i] = src[i];
  }
  for (int i = 0; i < n; ++i) cmyk_pixel_rgb(in[4 * i], in[4 * i + 1], in[4 * i + 2], in[4 * i + 3], invert, px + 3 * i);
  store_rgb4(rgb + 3 * p0, px, n);
}

// One component as the per-component colour pass reads it at scale 1 / 2^lg: its plane (pw samples a row) at
// the transform size of scaled_size_own(), the integral ratios (rh, rv) of the output grid to it, and its real samples
// dw x dh (jdmaster.c: the component's downsampled size, ceil(W·h·n / (8 hmax)) across).  At lg = 0 these are the
// full-size planes, the ratios of the sampling factors and ceil(W·h / hmax).
struct CompPlane {
  const unsigned char* P;
  int pw, rh, rv, dw, dh;
};
template <int kC, typename Header>
__device__ __forceinline__ void comp_planes(const Header& h, const Ws& ws, int lg, CompPlane* cp) {
  int hm, vm;
  largest_factors<kC>(h, hm, vm);
  const int mn = 8 >> lg;
  const unsigned char* base = ws.planes + h.plane_off;
  for (int c = 0; c < kC; ++c) {
    const int hc = factor14(h.h[c]), vc = factor14(h.v[c]);
    const int n = lg ? scaled_size_own(hc, vc, hm, vm, lg) : 8;
    cp[c].P = base;
    cp[c].pw = h.mcus_x * n * h.h[c];
    cp[c].rh = max(hm * mn / (hc * n), 1);
    cp[c].rv = max(vm * mn / (vc * n), 1);
    cp[c].dw = (int)(((long)h.width * hc * n + hm * 8 - 1) / (hm * 8));
    cp[c].dh = (int)(((long)h.height * vc * n + vm * 8 - 1) / (vm * 8));
    base += plane_bytes_own(h, c, n);
  }
}

// Four consecutive pixels of the image's H·W per lane (of ceil(W / s) · ceil(H / s) at scale 1 / s = 1 / 2^lg; kScaled =
// false is the full-size decode, lg = 0): every one of the kC components is read at its own sampling through
// upsampled_by() at its ratio to the largest sampling — component 0 too, where it is not the largest, and K like any
// other; at a reduced scale by the ratios that libjpeg's transform sizes leave.  Then, three components: ycc_rgb_convert,
// or the samples as they are for an RGB file (color = 1); four: the YCCK step (color = 1) and the chain of the comment
// above.  Plus the per-image status.  A record that layout_ok() refuses has status 1 and no pixels.
template <bool kScaled, int kC, typename Header>
__device__ __forceinline__ void color_own_pixels(const Header& h, const Ws& ws, int img, int lg_in,
                                                 unsigned char* __restrict__ out, int* __restrict__ status) {
  const int lg = kScaled ? lg_in : 0;
  const long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * kColor4Pixels;
  const int* st = ws.state + kStateWords * img;
  const bool framed = layout_ok(h), decoded = framed && st[0] == 0 && st[1] == h.n_intervals;
  if (p0 == 0) status[img] = decoded ? 0 : 1;
  const int round = (1 << lg) - 1;
  const int W = (h.width + round) >> lg, H = (h.height + round) >> lg;
  const long npix = (long)W * H;
  if (!(kPixelsOnlyWhenDecoded<Header> ? decoded : framed) || p0 >= npix) return;
  const int n = (int)min((long)kColor4Pixels, npix - p0);
  CompPlane cp[kC];
  comp_planes<kC>(h, ws, lg, cp);
  const bool fancy = lg < 3;
  unsigned char px[3 * kColor4Pixels];
  for (int i = 0; i < n; ++i) {
    const long p = p0 + i;
    const int y = (int)(p / W), x = (int)(p - (long)y * W);
    int s[kC];
#pragma unroll
    for (int c = 0; c < kC; ++c)
      s[c] = upsampled_by(cp[c].P, cp[c].pw, x, y, cp[c].rh, cp[c].rv, cp[c].dw, cp[c].dh, fancy);
    if constexpr (kC == 4) {
      if (h.color) {
        const int cb = s[1] - 128, cr = s[2] - 128, yv = s[0];
        s[0] = 255 - clamp255(yv + ((kCrR * cr + 32768) >> 16));
        s[1] = 255 - clamp255(yv + ((-kCbG * cb + 32768 - kCrG * cr) >> 16));
        s[2] = 255 - clamp255(yv + ((kCbB * cb + 32768) >> 16));
      }
      cmyk_pixel_rgb(s[0], s[1], s[2], s[3], 1, px + 3 * i);
    } else if (h.color) {
      for (int c = 0; c < 3; ++c) px[3 * i + c] = (unsigned char)s[c];
    } else {
      ycc_rgb_pixel(s[0], s[1], s[2], px + 3 * i);
    }
  }
  store_rgb4(out + h.out_off + 3 * p0, px, n);
}

// One launch for a batch of either per-component record: each image takes the body of its component count (a count
// that is neither, which layout_ok() refuses, the one for three: status 1, no pixels).
template <typename Header>
__global__ __launch_bounds__(256) void jpeg_color_own_kernel(const Header* __restrict__ hdrs, Ws ws,
                                                             unsigned char* __restrict__ out,
                                                             int* __restrict__ status) {
  const Header& h = hdrs[blockIdx.y];
  if (h.ncomp == 4) color_own_pixels<false, 4>(h, ws, blockIdx.y, 0, out, status);
  else color_own_pixels<false, 3>(h, ws, blockIdx.y, 0, out, status);
}

// The same at scale_log2[image] = 0..3.  Not a scale: nothing was decoded (jpeg_idct_scaled_kernel), nothing is written,
// and the image gets status 1.
template <typename Header>
__global__ __launch_bounds__(256) void jpeg_color_own_scaled_kernel(const Header* __restrict__ hdrs, Ws ws,
                                                                    const int* __restrict__ scale_log2,
                                                                    unsigned char* __restrict__ out,
                                                                    int* __restrict__ status) {
  const int img = blockIdx.y, lg = scale_log2[img];
  const Header& h = hdrs[img];
  if ((unsigned)lg > 3u) {
    if (blockIdx.x == 0 && threadIdx.x == 0) status[img] = 1;
    return;
  }
  if (h.ncomp == 4) color_own_pixels<true, 4>(h, ws, img, lg, out, status);
  else color_own_pixels<true, 3>(h, ws, img, lg, out, status);
}


// ---------------------------------------------------------------------------------------------------------------
// Progressive files (SOF2).  The host parser (jpeg.parse_progressive) reads the whole scan script and packs one
// odic_jpeg_prog_header per image, one odic_jpeg_scan per scan (sorted by dependency level) and the batch's distinct
// Huffman tables.  Launches:
//
//   segment   one workgroup per scan: the byte classification and compaction of the baseline path on the scan's own
//             byte range (the parser cut it at the closing marker), restart-interval start bits.
//   decode    one launch per dependency level, one wave per (scan, restart interval): the four coding procedures of
//             ITU T.81 G.1 / jdphuff.c, serial inside the interval.  Scans of one level touch disjoint coefficients
//             of an image, so all of them, for all images, run concurrently.  DC scans apply the prediction while
//             they decode (it resets at every interval), so the coefficient array holds libjpeg's values directly
//             and the baseline path's DC kernel is not needed.
//   idct / color   the baseline path's kernels on the same int16 natural-order coefficient array.
//
// Every lane of the wave runs the serial decode redundantly (uniform control flow, broadcast loads); what is
// parallel is per coefficient.  AC refinement holds zig-zag coefficient `lane` of the block in lane `lane`: the mask
// of already-nonzero coefficients is one ballot, a run of r zeros is r lowest-bit clears on the inverted mask, the
// correction bit of a nonzero coefficient passed over sits at (bit position of the step) + (nonzero coefficients
// passed before it), a popcount, and is fetched by that lane after the block's symbols are decoded.
//
// Bounds by construction, whatever the entropy data holds: a block ordinal is below the scan's n_units and its block
// index is checked against the image's block count; a zig-zag index is checked against Se <= 63 before it is used;
// the bit reader only advances while pos <= the interval's end, which keeps its look-ahead inside the 16 bytes reserved
// behind every compacted scan, and correction bits are fetched only after pos <= end was checked for the whole block.
//
// The per-component record (odic_jpeg_prog_header_any, entry point odic_jpeg_decode_progressive_any) runs the same
// segment kernel and the same decode kernel and coding procedures, instantiated for it: what differs is ProgGeo, the
// frame as the scans see it.  An interleaved scan walks the frame's MCUs, which span the largest factors whichever
// components the scan names, and writes the named components' blocks of each; a single-component scan walks the
// component's own raster, so the padding blocks outside it keep what the interleaved scans gave them (zero where there
// was none).  Then the per-component IDCT (block_geo_own) and colour kernel, as for odic_jpeg_header_any.
//
// The bounds argument, by record family.  A COMMON record's geometry is a function of `sampling` alone, which every
// helper maps to one of four fixed shapes (blocks_per_mcu, luma_h / luma_v), so a block index is below mcus_x · mcus_y ·
// bpm and a plane byte below 64 times that, the products the host sizes the coefficient array and the planes by.  A
// PER-COMPONENT record's geometry is built only from a record layout_ok() admits: ncomp 3 or 4, factors in 1..4 that
// divide the largest, at most 10 blocks per MCU — so the block-to-component map fits Frame's two bits per block, and hh,
// vv in 1..4 and first + nb <= bpm <= 10 fit ProgGeo's four-bit fields.  For a record it refuses, the baseline entropy
// kernels decode a frame of one block of component 0 into the record's own coefficient slice (interval_blocks() bounds
// every block index by the MCU count, write_span() by the interval's), and the progressive decode kernel reads nothing;
// a progressive scan whose mask names a component >= ncomp is refused before anything is read, so hh / vv of a named
// component are the record's own and never 0.  Every progressive block index, from raster_block() (single-component
// scans; bw is the scan's own and only has to be positive) or from u · bpm + first + j (interleaved scans, j < nb), is
// compared with nblocks = mcus_x · mcus_y · bpm before the coefficient array is touched, and the host sizes that array
// (coef_off, total_blocks) by the same product; the zig-zag index and bit reader rules are those above, unchanged.
// The IDCT reads block b < nblocks and writes plane bytes below 64 · nblocks from plane_off (block_geo_own places
// block j of MCU m at a row and column inside plane c's mcus_x·8·h[c] by mcus_y·8·v[c] samples); it returns at once
// for a record layout_ok() refuses.  The colour kernel returns before reading a plane, and writes status 1 and no
// pixel, for such a record (and, kPixelsOnlyWhenDecoded, for a progressive image whose state words report an error or
// a missing interval); otherwise it reads sample (y / rv, x / rh) and its neighbours clamped to the component's dw x dh
// real samples, which lie inside its plane because W <= mcus_x · 8 · hmax and H <= mcus_y · 8 · vmax.
// ---------------------------------------------------------------------------------------------------------------
static_assert(sizeof(odic_jpeg_prog_header) == 432 && offsetof(odic_jpeg_prog_header, qt) == 48 &&
                  sizeof(odic_jpeg_scan) == 88 && offsetof(odic_jpeg_scan, table) == 72 &&
                  sizeof(odic_jpeg_table) == 1424 && offsetof(odic_jpeg_table, huffval) == 1168,
              "the progressive records are mirrored by jpeg.PROG_HEADER_DTYPE / SCAN_DTYPE / TABLE_DTYPE");
static_assert(sizeof(odic_jpeg_prog_header_any) == 600 && offsetof(odic_jpeg_prog_header_any, ncomp) == 48 &&
                  offsetof(odic_jpeg_prog_header_any, h) == 56 && offsetof(odic_jpeg_prog_header_any, qt) == 88 &&
                  offsetof(odic_jpeg_prog_header_any, n_intervals) == offsetof(odic_jpeg_prog_header, n_intervals) &&
                  offsetof(odic_jpeg_scan, pad) == 84,
              "odic_jpeg_prog_header_any is mirrored by jpeg.PROG_HEADER_ANY_DTYPE; it shares odic_jpeg_prog_header's prefix");

struct PTab {                      // one Huffman table in LDS
  unsigned short lut[512];
  int lim[8];                      // as Tabs::lim
  int valoff[18];
  unsigned char huffval[256];
};

__device__ void load_ptab(const odic_jpeg_table& g, PTab& T) {          // one wave
  const int t = threadIdx.x;
  for (int i = t; i < 512; i += 64) T.lut[i] = g.lut[i];
  for (int i = t; i < 256; i += 64) T.huffval[i] = g.huffval[i];
  if (t < 18) T.valoff[t] = g.valoff[t];
  if (t == 0) fill_lim(g.maxcode, T.lim, 0);
}

// The frame as the scans see it: the blocks of an MCU, and for component c its blocks per MCU across and down
// (hh, vv), their number (nb) and the place of the first of them in the MCU (first) — the inverse of the map from a
// block of the MCU to its component that the IDCT follows (block_geo / block_geo_own).  set() is false for a frame or
// a scan mask the kernel does not decode; the geometry is then that of one 1x1 block, which nothing reads.
template <typename Header>
struct ProgGeo;
// three components or gray: component 0 carries the only sub-sampling
template <>
struct ProgGeo<odic_jpeg_prog_header> {
  static constexpr int kComps = 3;
  int nY, bpm, hy, vy;
  __device__ __forceinline__ bool set(const odic_jpeg_prog_header& h, int mask, int blocks_w) {
    nY = luma_blocks(h.sampling);
    bpm = blocks_per_mcu(h.sampling);                    // gray: the MCU order is the component's block raster
    hy = luma_h(h.sampling);
    vy = luma_v(h.sampling);
    return h.sampling != kGray || (mask == 1 && blocks_w > 0);   // gray: component 0 alone, every scan
  }
  __device__ __forceinline__ int hh(int c) const { return c == 0 ? hy : 1; }
  __device__ __forceinline__ int vv(int c) const { return c == 0 ? vy : 1; }
  __device__ __forceinline__ int nb(int c) const { return c == 0 ? nY : 1; }
  __device__ __forceinline__ int first(int c) const { return c == 0 ? 0 : nY + c - 1; }
};
// three or four components, each with its own sampling (layout_ok: factors in 1..4, at most 10 blocks), four bits per
// component and field: block_geo_own's order, component after component, each row by row
template <>
struct ProgGeo<odic_jpeg_prog_header_any> {
  static constexpr int kComps = 4;
  unsigned hp, vp, fp;
  int bpm;
  __device__ __forceinline__ bool set(const odic_jpeg_prog_header_any& h, int mask, int) {
    hp = vp = 0x1111u;
    fp = 0;
    bpm = 1;
    if (!layout_ok(h) || (mask >> h.ncomp) != 0) return false;   // the mask names a component the frame lacks
    hp = vp = 0;
    bpm = 0;
    for (int c = 0; c < 4; ++c) {
      const bool have = c < h.ncomp;
      hp |= (unsigned)(have ? h.h[c] : 1) << (4 * c);
      vp |= (unsigned)(have ? h.v[c] : 1) << (4 * c);
      fp |= (unsigned)bpm << (4 * c);
      if (have) bpm += h.h[c] * h.v[c];
    }
    return true;
  }
  __device__ __forceinline__ int hh(int c) const { return (hp >> (4 * c)) & 15; }
  __device__ __forceinline__ int vv(int c) const { return (vp >> (4 * c)) & 15; }
  __device__ __forceinline__ int nb(int c) const { return hh(c) * vv(c); }
  __device__ __forceinline__ int first(int c) const { return (fp >> (4 * c)) & 15; }
};

template <typename Header>
struct ScanCtx {
  static constexpr int kComps = ProgGeo<Header>::kComps;
  const unsigned* w;               // the scan's compacted words
  short* coef;                     // the image's coefficient blocks
  long nblocks;                    // ... and how many there are
  int mcus_x;
  ProgGeo<Header> g;
  int u0, nu;                      // the interval's units (MCUs of an interleaved scan, else blocks of the component)
  int pos, end;                    // its bit range
  int mask, ss, se, al, bw;
  int* state;
};

// block `n` of component c's own raster (bw blocks per row) → its block index in the MCU-ordered coefficient array
template <typename X>
__device__ __forceinline__ long raster_block(const X& x, int c, int n) {
  const int bx = n % x.bw, by = n / x.bw;
  const int hh = x.g.hh(c), vv = x.g.vv(c);
  const long mcu = (long)(by / vv) * x.mcus_x + bx / hh;
  return mcu * x.g.bpm + x.g.first(c) + (by % vv) * hh + bx % hh;
}

__device__ __forceinline__ unsigned bit_at(const unsigned* __restrict__ w, int pos) {
  return (__builtin_bswap32(w[pos >> 5]) >> (31 - (pos & 31))) & 1u;
}

// DC, first pass (G.1.2.1): difference coding, prediction reset at the interval's start, value << Al
template <typename X>
__device__ bool prog_dc_first(X& x, const PTab* T) {
  int pred[X::kComps] = {};
  Bits br{x.w, 0};
  bits_seek(br, x.pos);
  const bool single = (x.mask & (x.mask - 1)) == 0;
  for (int u = x.u0; u < x.u0 + x.nu; ++u) {
    int q = 0;
#pragma unroll
    for (int c = 0; c < X::kComps; ++c) {
      if (!((x.mask >> c) & 1)) continue;
      const int nb = single ? 1 : x.g.nb(c);
      for (int j = 0; j < nb; ++j) {
        if (x.pos > x.end) return false;
        const unsigned win = bits_peek(br, x.pos);
        int len;
        const int cat = huff(T[q], 0, win, len);
        if (cat < 0 || cat > 15) return false;
        const int diff = cat ? extend((win << len) >> (32 - cat), cat) : 0;
        x.pos += len + cat;
        pred[c] += diff;
        const int v = pred[c] * (1 << x.al);
        if (v < -32768 || v > 32767) atomicOr(&x.state[0], kErrRange);
        const long b = single ? raster_block(x, c, u) : (long)u * x.g.bpm + x.g.first(c) + j;
        if (b < 0 || b >= x.nblocks) return false;
        if (threadIdx.x == 0) x.coef[b * 64] = (short)v;
      }
      ++q;
    }
  }
  return x.pos <= x.end;
}

// DC, refinement (G.1.2.1): one raw bit per block, 64 blocks per step
template <typename X>
__device__ bool prog_dc_refine(X& x) {
  const bool single = (x.mask & (x.mask - 1)) == 0;
  int bps = 0;                                          // blocks per MCU of this scan
  for (int c = 0; c < X::kComps; ++c) bps += ((x.mask >> c) & 1) ? x.g.nb(c) : 0;
  if (single) bps = 1;
  const long nb = (long)x.nu * bps;
  if (x.pos + nb > x.end) return false;
  bool ok = true;
  for (long i = threadIdx.x; i < nb; i += 64) {
    long b;
    if (single) {
      b = raster_block(x, __builtin_ctz(x.mask), x.u0 + (int)i);
    } else {
      int idx = (int)(i % bps), j = 0;
      for (int c = 0; c < X::kComps; ++c) {
        if (!((x.mask >> c) & 1)) continue;
        const int n = x.g.nb(c);
        if (idx < n) {
          j = x.g.first(c) + idx;
          break;
        }
        idx -= n;
      }
      b = (long)(x.u0 + i / bps) * x.g.bpm + j;
    }
    if (b < 0 || b >= x.nblocks) {
      ok = false;
      continue;
    }
    if (bit_at(x.w, x.pos + (int)i)) x.coef[b * 64] |= (short)(1 << x.al);
  }
  x.pos += (int)nb;
  return __all(ok);
}

// AC, first pass (G.1.2.2): run/size symbols, ZRL, EOB runs carried across blocks (reset at the interval's start)
template <typename X>
__device__ bool prog_ac_first(X& x, const PTab& T) {
  const int c = __builtin_ctz(x.mask);
  Bits br{x.w, 0};
  bits_seek(br, x.pos);
  int eobrun = 0;
  const int nend = x.u0 + x.nu;
  for (int n = x.u0; n < nend; ++n) {
    if (eobrun > 0) {                                   // these blocks get nothing in this scan
      const int skip = min(eobrun, nend - n);
      eobrun -= skip;
      n += skip - 1;
      continue;
    }
    const long b = raster_block(x, c, n);
    if (b < 0 || b >= x.nblocks) return false;
    for (int k = x.ss; k <= x.se; ++k) {
      if (x.pos > x.end) return false;
      const unsigned win = bits_peek(br, x.pos);
      int len;
      const int rs = huff(T, 0, win, len);
      if (rs < 0) return false;
      const int r = rs >> 4, s = rs & 15;
      if (s) {
        k += r;
        if (k > x.se) return false;                     // libjpeg would write outside the band
        const int v = extend((win << len) >> (32 - s), s);
        x.pos += len + s;
        if (threadIdx.x == 0) x.coef[b * 64 + kNatural[k]] = (short)(v * (1 << x.al));
      } else if (r == 15) {
        k += 15;
        x.pos += len;
      } else {
        eobrun = 1 << r;
        if (r) eobrun += (int)((win << len) >> (32 - r));
        x.pos += len + r;
        --eobrun;                                       // this block is the run's first
        break;
      }
    }
  }
  return x.pos <= x.end;
}

// AC, refinement (G.1.2.3).  Lane i holds zig-zag coefficient i of the block.
template <typename X>
__device__ bool prog_ac_refine(X& x, const PTab& T) {
  const int c = __builtin_ctz(x.mask);
  const int lane = threadIdx.x;
  const int nat = kNatural[lane];
  const int p1 = 1 << x.al, m1 = -p1;
  const unsigned long long band = (x.se == 63 ? ~0ull : (1ull << (x.se + 1)) - 1) & ~((1ull << x.ss) - 1);
  const unsigned long long below = (1ull << lane) - 1;
  Bits br{x.w, 0};
  bits_seek(br, x.pos);
  int eobrun = 0;
  const int nend = x.u0 + x.nu;
  long b = raster_block(x, c, x.u0);
  if (b < 0 || b >= x.nblocks) return false;
  int v = x.coef[b * 64 + nat];
  for (int n = x.u0; n < nend; ++n) {
    long bn = b;
    int vn = 0;
    if (n + 1 < nend) {                                 // the next block's coefficients are on their way meanwhile
      bn = raster_block(x, c, n + 1);
      if (bn < 0 || bn >= x.nblocks) return false;
      vn = x.coef[bn * 64 + nat];
    }
    const unsigned long long nz = __ballot(v != 0) & band;
    int cpos = -1, newv = 0;                            // this lane's correction bit / newly nonzero value
    int k = x.ss;
    if (eobrun == 0) {
      while (k <= x.se) {
        if (x.pos > x.end) return false;
        const unsigned win = bits_peek(br, x.pos);
        int len;
        const int rs = huff(T, 0, win, len);
        if (rs < 0) return false;
        const int r = rs >> 4, s = rs & 15;
        x.pos += len;
        int sval = 0;
        if (s) {
          if (s != 1) return false;                     // libjpeg warns and carries on: the host's business
          sval = ((win << len) >> 31) ? p1 : m1;
          x.pos += 1;
        } else if (r != 15) {
          eobrun = 1 << r;
          if (r) eobrun += (int)((win << len) >> (32 - r));
          x.pos += r;
          break;                                        // the rest of the block is the run's first block
        }
        const unsigned long long from = ~0ull << k;
        unsigned long long z = ~nz & band & from;       // still-zero coefficients from k on
        for (int q = 0; q < r; ++q) z &= z - 1;         // r of them are skipped
        const int t = z ? __builtin_ctzll(z) : x.se + 1;
        const unsigned long long passed = nz & from & (t >= 64 ? ~0ull : (1ull << t) - 1);
        if ((passed >> lane) & 1) cpos = x.pos + __popcll(passed & below);
        x.pos += __popcll(passed);
        if (s) {
          if (t > x.se) return false;                   // libjpeg would write outside the band
          if (lane == t) newv = sval;
        }
        k = t + 1;
      }
    }
    if (eobrun > 0) {                                   // only correction bits for the rest of the band
      const unsigned long long passed = k <= 63 ? nz & (~0ull << k) : 0ull;
      if ((passed >> lane) & 1) cpos = x.pos + __popcll(passed & below);
      x.pos += __popcll(passed);
      --eobrun;
    }
    if (x.pos > x.end) return false;                    // every cpos < pos <= end
    if (cpos >= 0) {
      if (bit_at(x.w, cpos) && (v & p1) == 0) x.coef[b * 64 + nat] = (short)(v + (v >= 0 ? p1 : m1));
    } else if (newv) {
      x.coef[b * 64 + nat] = (short)newv;
    }
    b = bn;
    v = vn;
  }
  return true;
}

__global__ __launch_bounds__(256) void jpeg_prog_segment_kernel(const odic_jpeg_scan* __restrict__ scans,
                                                                const unsigned char* __restrict__ data, Ws ws,
                                                                int n_images) {
  const odic_jpeg_scan& sc = scans[blockIdx.x];
  if ((unsigned)sc.image >= (unsigned)n_images) return;
  long carry_data;
  int carry_marks;
  const int err = segment_bytes(data + sc.data_off, sc.data_end - sc.data_off, ws.scan + sc.scan_off,
                                ws.int_bits + sc.int_off, sc.n_intervals, false, carry_data, carry_marks);
  if (threadIdx.x == 0 && err) atomicOr(&ws.state[kStateWords * sc.image], kErrSegment);
}

template <typename Header>                                      // odic_jpeg_prog_header or odic_jpeg_prog_header_any
__global__ __launch_bounds__(64) void jpeg_prog_decode_kernel(const Header* __restrict__ hdrs,
                                                              const odic_jpeg_scan* __restrict__ scans,
                                                              const odic_jpeg_table* __restrict__ tables, Ws ws,
                                                              int first, int n_images, int n_tables) {
  const odic_jpeg_scan& sc = scans[first + blockIdx.y];
  const int k = blockIdx.x;
  if (k >= sc.n_intervals || (unsigned)sc.image >= (unsigned)n_images) return;
  const Header& h = hdrs[sc.image];
  int* state = ws.state + kStateWords * sc.image;
  constexpr int kC = ProgGeo<Header>::kComps, kMask = (1 << kC) - 1;
  __shared__ PTab T[kC];
  const bool dc = sc.ss == 0, first_pass = sc.ah == 0;
  const int ntab = dc ? (first_pass ? __popc(sc.comp_mask & kMask) : 0) : 1;
  ScanCtx<Header> x;
  bool ok = sc.restart > 0 && sc.n_units > 0 && (sc.comp_mask & kMask) != 0 && sc.ss >= 0 && sc.ss <= sc.se &&
            sc.se <= 63 && sc.al >= 0 && sc.al <= 13 && (dc || ((sc.comp_mask & (sc.comp_mask - 1)) == 0 && sc.blocks_w > 0));
  ok = x.g.set(h, sc.comp_mask & kMask, sc.blocks_w) && ok;
  for (int q = 0; q < ntab && ok; ++q) {
    const int ti = q < 3 ? sc.table[q] : sc.pad;        // the fourth index: four components only (kC = 4)
    if ((unsigned)ti >= (unsigned)n_tables) ok = false;
    else load_ptab(tables[ti], T[q]);
  }
  __syncthreads();
  if (ok) {
    const int* ib = ws.int_bits + sc.int_off;
    x.w = (const unsigned*)(ws.scan + sc.scan_off);
    x.coef = ws.coef + h.coef_off * 64;
    x.nblocks = (long)h.mcus_x * h.mcus_y * x.g.bpm;
    x.mcus_x = h.mcus_x;
    x.u0 = k * sc.restart;
    x.nu = min(sc.restart, sc.n_units - x.u0);
    x.pos = ib[k];
    x.end = ib[k + 1];
    x.mask = sc.comp_mask & kMask;
    x.ss = sc.ss;
    x.se = sc.se;
    x.al = sc.al;
    x.bw = max(sc.blocks_w, 1);
    x.state = state;
    if (dc) ok = first_pass ? prog_dc_first(x, T) : prog_dc_refine(x);
    else ok = first_pass ? prog_ac_first(x, T[0]) : prog_ac_refine(x, T[0]);
  }
  if (threadIdx.x == 0) {
    if (ok) atomicAdd(&state[1], 1);
    else atomicOr(&state[0], kErrDecode);
  }
}

bool prog_batch_ok(const odic_jpeg_prog_batch* b) {
  if (!batch_dims_ok(*b) || b->n_scans < b->n_images || (long)b->n_scans > (long)b->n_images * ODIC_JPEG_MAX_SCANS ||
      b->n_tables <= 0 || b->n_levels <= 0 || b->n_levels > ODIC_JPEG_MAX_SCANS || b->total_intervals > 0x7fffffffL)
    return false;
  if (b->level_first[0] != 0 || b->level_first[b->n_levels] != b->n_scans) return false;
  for (int l = 0; l < b->n_levels; ++l) {
    const int n = b->level_first[l + 1] - b->level_first[l];
    if (n <= 0 || n > 65535 || b->level_intervals[l] <= 0) return false;
  }
  return true;
}

}  // namespace

extern "C" size_t odic_jpeg_workspace_bytes(const odic_jpeg_batch* b) {
  if (!b || b->n_images <= 0 || b->max_sync_passes < 0 || b->total_scan_bytes < 0 || b->total_intervals < 0 ||
      b->total_units < 0 || b->total_blocks < 0 || b->total_plane_bytes < 0)
    return 0;
  return layout(*b).total;
}

namespace {

// The IDCT and colour launches both entry points of a file kind end with: full-size (scale_log2 == nullptr, the
// kernels of odic_jpeg_decode / odic_jpeg_decode_progressive) or per-image scales.
template <typename Header, typename Batch>
void launch_idct_color(const Batch* b, const Header* hdrs, const Ws& ws, const int32_t* scale_log2, hipStream_t s) {
  const dim3 igrid((unsigned)((b->max_blocks + 31) / 32), b->n_images);
  const dim3 cgrid((b->max_width + 63) / 64, (b->max_height + 3) / 4, b->n_images);
  if (scale_log2) {
    hipLaunchKernelGGL(jpeg_idct_scaled_kernel<Header>, igrid, dim3(256), 0, s, hdrs, ws, scale_log2);
    hipLaunchKernelGGL(jpeg_color_scaled_kernel<Header>, cgrid, dim3(64, 4), 0, s, hdrs, ws, scale_log2, b->out,
                       b->status);
  } else {
    hipLaunchKernelGGL(jpeg_idct_kernel<Header>, igrid, dim3(256), 0, s, hdrs, ws);
    hipLaunchKernelGGL(jpeg_color_kernel<Header>, cgrid, dim3(64, 4), 0, s, hdrs, ws, b->out, b->status);
  }
}

// The same for the per-component records: the per-component IDCT and the one colour kernel, four pixels per lane;
// max_width / max_height are those of the scaled sizes.
template <typename Header, typename Batch>
void launch_idct_color_own(const Batch* b, const Header* hdrs, const Ws& ws, const int32_t* scale_log2, hipStream_t s) {
  const int n = b->n_images;
  const long lanes = ((long)b->max_width * b->max_height + kColor4Pixels - 1) / kColor4Pixels;
  const dim3 igrid((unsigned)((b->max_blocks + 31) / 32), n), cgrid((unsigned)((lanes + 255) / 256), n);
  if (scale_log2) {
    hipLaunchKernelGGL(jpeg_idct_scaled_kernel<Header>, igrid, dim3(256), 0, s, hdrs, ws, scale_log2);
    hipLaunchKernelGGL(jpeg_color_own_scaled_kernel<Header>, cgrid, dim3(256), 0, s, hdrs, ws, scale_log2, b->out,
                       b->status);
  } else {
    hipLaunchKernelGGL(jpeg_idct_kernel<Header>, igrid, dim3(256), 0, s, hdrs, ws);
    hipLaunchKernelGGL(jpeg_color_own_kernel<Header>, cgrid, dim3(256), 0, s, hdrs, ws, b->out, b->status);
  }
}

// Header: odic_jpeg_header (common) or odic_jpeg_header_any (per-component)
template <typename Header>
int decode_baseline(const odic_jpeg_batch* b, void* workspace, size_t ws_bytes, void* stream,
                    const int32_t* scale_log2) {
  if (!b || !b->headers || !b->data || !b->out || !b->status || !workspace) return ODIC_ENULL;
  if (!batch_dims_ok(*b) || b->subseq_bits < 32 || b->subseq_bits > kMaxSubseqBits || b->max_sync_passes < 0 ||
      b->max_sync_passes > 64 || b->max_units <= 0 || b->max_intervals <= 0 || b->max_scan_bytes <= 0 ||
      b->max_scan_bytes > kMaxScanBytes || b->total_units <= 0)
    return ODIC_EINVAL;
  const size_t need = odic_jpeg_workspace_bytes(b);
  if (need == 0 || ws_bytes < need) return ODIC_EINVAL;
  const Layout L = layout(*b);
  const Ws ws = bind(workspace, L);
  hipStream_t s = (hipStream_t)stream;
  const auto* hdrs = (const Header*)b->headers;
  const int n = b->n_images, S = b->subseq_bits;
  hipError_t e = hipMemsetAsync(workspace, 0, L.scan, s);                 // state, flags, last_change
  if (e == hipSuccess) e = hipMemsetAsync(ws.coef, 0, L.planes - L.coef, s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(jpeg_segment_kernel<Header>, dim3(n), dim3(256), 0, s, hdrs, b->data, ws, S);
  const dim3 ugrid((b->max_units + kUnitLanes - 1) / kUnitLanes, n);
  const size_t lds = sizeof(unsigned) * stage_words(S);
  for (int p = 0; p <= b->max_sync_passes; ++p)                          // pass 0: speculative
    hipLaunchKernelGGL(jpeg_sync_kernel<Header>, ugrid, dim3(kUnitLanes), lds, s, hdrs, ws, S, p);
  hipLaunchKernelGGL(jpeg_serial_kernel<Header>, dim3(b->max_intervals, n), dim3(64), 0, s, hdrs, ws, S);
  hipLaunchKernelGGL(jpeg_block_scan_kernel<Header>, dim3(n), dim3(256), 0, s, hdrs, ws);
  hipLaunchKernelGGL(jpeg_writeout_kernel<Header>, ugrid, dim3(kUnitLanes), lds, s, hdrs, ws, S);
  hipLaunchKernelGGL(jpeg_dc_kernel<Header>, dim3(n), dim3(256), 0, s, hdrs, ws);
  if constexpr (kPerComponent<Header>) launch_idct_color_own(b, hdrs, ws, scale_log2, s);
  else launch_idct_color(b, hdrs, ws, scale_log2, s);
  return odic_launch_status();
}

// Header: odic_jpeg_prog_header (common) or odic_jpeg_prog_header_any (per-component)
template <typename Header>
int decode_progressive(const odic_jpeg_prog_batch* b, void* workspace, size_t ws_bytes, void* stream,
                       const int32_t* scale_log2) {
  if (!b || !b->headers || !b->scans || !b->tables || !b->data || !b->out || !b->status || !workspace)
    return ODIC_ENULL;
  if (!prog_batch_ok(b)) return ODIC_EINVAL;
  const Layout L = layout(*b);
  if (ws_bytes < L.total) return ODIC_EINVAL;
  const Ws ws = bind(workspace, L);
  hipStream_t s = (hipStream_t)stream;
  const auto* hdrs = (const Header*)b->headers;
  const auto* scans = (const odic_jpeg_scan*)b->scans;
  const auto* tables = (const odic_jpeg_table*)b->tables;
  const int n = b->n_images;
  hipError_t e = hipMemsetAsync(workspace, 0, L.scan, s);                 // state
  if (e == hipSuccess) e = hipMemsetAsync(ws.coef, 0, L.planes - L.coef, s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(jpeg_prog_segment_kernel, dim3(b->n_scans), dim3(256), 0, s, scans, b->data, ws, n);
  for (int l = 0; l < b->n_levels; ++l)
    hipLaunchKernelGGL(jpeg_prog_decode_kernel<Header>,
                       dim3(b->level_intervals[l], b->level_first[l + 1] - b->level_first[l]), dim3(64), 0, s, hdrs, scans,
                       tables, ws, b->level_first[l], n, b->n_tables);
  if constexpr (kPerComponent<Header>) launch_idct_color_own(b, hdrs, ws, scale_log2, s);
  else launch_idct_color(b, hdrs, ws, scale_log2, s);
  return odic_launch_status();
}

}  // namespace

extern "C" int odic_jpeg_decode(const odic_jpeg_batch* b, void* workspace, size_t ws_bytes, void* stream) {
  return decode_baseline<odic_jpeg_header>(b, workspace, ws_bytes, stream, nullptr);
}

extern "C" size_t odic_jpeg_any_workspace_bytes(const odic_jpeg_batch* b) { return odic_jpeg_workspace_bytes(b); }

extern "C" int odic_jpeg_any_decode(const odic_jpeg_batch* b, void* workspace, size_t ws_bytes, void* stream) {
  return decode_baseline<odic_jpeg_header_any>(b, workspace, ws_bytes, stream, nullptr);
}

extern "C" int odic_cmyk_to_rgb8(const uint8_t* cmyk, uint8_t* rgb, int64_t n_pixels, int invert, void* stream) {
  if (!cmyk || !rgb) return ODIC_ENULL;
  const int64_t blocks = (n_pixels + 256 * kColor4Pixels - 1) / (256 * kColor4Pixels);
  if (n_pixels < 0 || blocks > 0x7fffffffL) return ODIC_EINVAL;
  if (n_pixels == 0) return 0;
  hipLaunchKernelGGL(cmyk_to_rgb8_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, cmyk, rgb,
                     (long)n_pixels, invert);
  return odic_launch_status();
}

extern "C" int odic_jpeg_decode_scaled(const odic_jpeg_batch* b, const int32_t* scale_log2, void* workspace,
                                       size_t ws_bytes, void* stream) {
  if (!scale_log2) return ODIC_ENULL;
  return decode_baseline<odic_jpeg_header>(b, workspace, ws_bytes, stream, scale_log2);
}

extern "C" size_t odic_jpeg_progressive_workspace_bytes(const odic_jpeg_prog_batch* b) {
  if (!b || !prog_batch_ok(b)) return 0;
  return layout(*b).total;
}

extern "C" size_t odic_jpeg_progressive_coef_offset(const odic_jpeg_prog_batch* b) {
  if (!b || !prog_batch_ok(b)) return 0;
  return layout(*b).coef;
}

extern "C" int odic_jpeg_decode_progressive(const odic_jpeg_prog_batch* b, void* workspace, size_t ws_bytes,
                                            void* stream) {
  return decode_progressive<odic_jpeg_prog_header>(b, workspace, ws_bytes, stream, nullptr);
}

extern "C" size_t odic_jpeg_progressive_any_workspace_bytes(const odic_jpeg_prog_batch* b) {
  return odic_jpeg_progressive_workspace_bytes(b);
}

extern "C" int odic_jpeg_decode_progressive_any(const odic_jpeg_prog_batch* b, void* workspace, size_t ws_bytes,
                                                void* stream) {
  return decode_progressive<odic_jpeg_prog_header_any>(b, workspace, ws_bytes, stream, nullptr);
}

extern "C" int odic_jpeg_any_decode_scaled(const odic_jpeg_batch* b, const int32_t* scale_log2, void* workspace,
                                           size_t ws_bytes, void* stream) {
  if (!scale_log2) return ODIC_ENULL;
  return decode_baseline<odic_jpeg_header_any>(b, workspace, ws_bytes, stream, scale_log2);
}

extern "C" int odic_jpeg_decode_progressive_any_scaled(const odic_jpeg_prog_batch* b, const int32_t* scale_log2,
                                                       void* workspace, size_t ws_bytes, void* stream) {
  if (!scale_log2) return ODIC_ENULL;
  return decode_progressive<odic_jpeg_prog_header_any>(b, workspace, ws_bytes, stream, scale_log2);
}

extern "C" int odic_jpeg_decode_progressive_scaled(const odic_jpeg_prog_batch* b, const int32_t* scale_log2,
                                                   void* workspace, size_t ws_bytes, void* stream) {
  if (!scale_log2) return ODIC_ENULL;
  return decode_progressive<odic_jpeg_prog_header>(b, workspace, ws_bytes, stream, scale_log2);
}
