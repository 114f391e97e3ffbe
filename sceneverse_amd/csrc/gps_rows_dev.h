// gps_rows_dev.h -- what gps_obj_select.hip (one thread per position, 16 waves) and gps_obj_select_pred.hip (256 threads,
// positions strided) share: the clamp of a device-read range, the ordered compaction of up to GPS_OBJ_SELECT_MAX_SCAN
// positions, the seeded fill law of include/gps_hip.h.  (The fill as ONE helper measured slower: profiles/rows/NOTE.md.)
//
// Compaction.  The positions of a scan are cut into kSegs segments of 64; a wave holds one segment at a time, lane =
// position inside it.  seg_ballot() turns a flag into the lane's rank inside its segment (the popcount of the ballot
// below the lane) and leaves the segment's count in LDS; after ONE barrier seg_sums() adds up the segments before the
// caller's own (kSegs words per counter, the same address in every lane: broadcast reads) -- an exclusive scan in
// ascending position order without a second pass.  rank = before + rank inside the segment.
//
// Fill.  Entry r of remained has the 64-bit key (uint64(rng_u32(S + 3, b * 2^20 + r)) << 32) | r; the keys go to LDS
// (padded to a pair with an all-ones key, above every real one: the low word is below 1024) and key_ranks() counts the
// keys below the caller's own -- all lanes read the same 16 bytes, two keys per read, one 64-bit compare per key: a rank
// without a sort.  The low word makes the order total, so a numpy emulation is bit-equal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gps_dropout.h"
#include "gps_hip.h"

namespace gps_rows {

constexpr int kMaxScan = GPS_OBJ_SELECT_MAX_SCAN;   // 1024 positions
constexpr int kSegs = kMaxScan / 64;                // 16 segments, one wave ballot each

// a [first, last) range read from device memory, clamped into [0, n) -> its length (0 for an empty or reversed one)
__device__ __forceinline__ int clamp_range(int &first, int &last, int n) {
  first = first < 0 ? 0 : first;
  last = last > n ? n : last;
  return last > first ? last - first : 0;
}
// -> the lane's rank among the flagged lanes of segment `seg`; cnt[seg] = how many there are (read it after a barrier)
__device__ __forceinline__ int seg_ballot(bool flag, int *cnt, int seg, int lane) {
  const unsigned long long m = __ballot(flag);
  if (lane == 0) cnt[seg] = __popcll(m);
  return __popcll(m & ((1ull << lane) - 1ull));
}

// cnt[s]: one counter's count in segment s.  -> the sum over all segments; before = the sum over the segments below `seg`
__device__ __forceinline__ int seg_sums(const int (&cnt)[kSegs], int seg, int &before) {
  int total = 0, bef = 0;
#pragma unroll
  for (int s = 0; s < kSegs; ++s) {
    const int v = cnt[s];
    total += v;
    bef += s < seg ? v : 0;
  }
  before = bef;
  return total;
}
__device__ __forceinline__ int seg_total(const int (&cnt)[kSegs]) {
  int total = 0;
#pragma unroll
  for (int s = 0; s < kSegs; ++s) total += cnt[s];
  return total;
}

// the fill key of entry r of row b's remained; S = seed + *seed_dev (gps_dropout::effective_seed)
__device__ __forceinline__ unsigned long long fill_key(unsigned long long S, int b, int r) {
  return ((unsigned long long)gps_dropout::rng_u32(S + 3ull, ((unsigned long long)b << 20) + (unsigned long long)r) << 32) |
         (unsigned long long)r;
}
constexpr unsigned long long kPadKey = ~0ull;       // completes the last pair of s_key

// rank[i] = how many of the 2 * n_pairs keys of s_key (16-byte aligned) are below key[i]
template <int N>
__device__ __forceinline__ void key_ranks(const unsigned long long *s_key, int n_pairs, const unsigned long long (&key)[N],
                                          int (&rank)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) rank[i] = 0;
#pragma unroll 4
  for (int q = 0; q < n_pairs; ++q) {
    const ulonglong2 k2 = reinterpret_cast<const ulonglong2 *>(s_key)[q];      // the same 16 bytes in every lane
#pragma unroll
    for (int i = 0; i < N; ++i) {
      rank[i] += k2.x < key[i] ? 1 : 0;
      rank[i] += k2.y < key[i] ? 1 : 0;
    }
  }
}

}  // namespace gps_rows
