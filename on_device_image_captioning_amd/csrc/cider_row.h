// The workspace row odic_cider_vectorize writes (include/odic_hip.h has the layout) and the search in its sorted keys:
// shared by the kernels that read such rows, csrc/cider.hip and csrc/caption_metrics.hip.
#pragma once
#include "odic_common.h"

namespace {

constexpr int NK = ODIC_CIDER_MAX_KEYS;        // key slots per caption: 128 + 127 + 126 + 125 = 506 n-grams at most
constexpr int MAXLEN = ODIC_CIDER_MAX_LEN;
constexpr int ROW = ODIC_CIDER_ROW_WORDS;

// a workspace row, in 8-byte words: [keys NK | weights NK | norms 4 | {count, length}]
struct Row {
  unsigned long long* keys; double* w; double* norms; int* meta;
  __device__ __forceinline__ Row(unsigned long long* base) : keys(base), w((double*)(base + NK)),
      norms((double*)(base + 2 * NK)), meta((int*)(base + 2 * NK + 4)) {}
};

__device__ __forceinline__ int key_order(unsigned long long k) { return (k >> 48) ? 3 : (k >> 32) ? 2 : (k >> 16) ? 1 : 0; }

// index of `key` in the ascending array a[0, n), or -1
__device__ __forceinline__ int find_key(const unsigned long long* __restrict__ a, int n, unsigned long long key) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return (lo < n && a[lo] == key) ? lo : -1;
}

}  // namespace
