// gps_obj_select.hip -- which objects of a scan enter the batch, on MI355X (gfx950): background filter, target-first
// crop and the random fill, for a whole batch in one launch.
//
// Reference (what this one entry replaces on the data-loader workers, per sample):
//   ScanBase._getitem_pretrain      data/datasets/base.py:231-246  drop wall / floor / ceiling, shuffle, keep max_obj_len
//   ScanBase._getitem_obj_pretrain  data/datasets/base.py:275-289  the same behind the CLASS_LABELS_200 filter
//   ScanBase._getitem_refer         data/datasets/base.py:368-450  filter (the target stays), target first, its class,
//                                                                  random.shuffle of the rest; :485-488 is_multiple / is_hard
//   ScanBase._getitem_finalrefer    data/datasets/base.py:877-957, :992-994  the same, flags on the raw label
//   label counts                    data/datasets/scannet.py:70-76
//
// gps_obj_select   ONE launch, no atomics, no workspace, no scratch, no host sync; every element of every output is
//   written.  Grid: one workgroup of kBlock = GPS_OBJ_SELECT_MAX_SCAN threads (16 waves) per row, thread p = position p
//   of the row's scan.  The rule is stated in include/gps_hip.h; tests/rows_cases.py restates it in numpy.
//   The ballot compaction and the rank loop described below are csrc/gps_rows_dev.h's (seg_ballot / seg_sums, fill_key /
//   key_ranks), shared with the selection of predicted proposals (gps_obj_select_pred.hip); wave w is its segment w.
//   * One pass of five ballots per wave: kept, class-mate of the target, remained, same mapped label, same raw label.
//     A lane's rank inside its wave is the popcount of the ballot below it; lane 0 of each wave leaves the wave's five
//     counts in LDS, and after ONE barrier every thread adds up the waves before its own (16 words, the same address in
//     every lane: a broadcast read) -- an exclusive scan without a second pass.
//   * The row is assembled in LDS (s_row, O words, -1 everywhere first) and stored once, coalesced: the three writers
//     of a row -- sel or [target, class-mates], the fill, the padding -- never meet in global memory.
//   * remained lives in LDS as positions (s_rem).  Replay form: thread j < free slots reads order[b][j] and takes
//     s_rem[that].  Device law: thread r < n_rem hashes its own index, the 64-bit keys go to LDS (s_key), and each
//     thread counts the keys below its own -- all lanes read the same 16 bytes, two keys per read, at most 512 reads
//     per thread, one 64-bit compare per key -- a rank without a sort; a rank below the number of free slots is the
//     slot.  The low word r of the key makes the order total, so a numpy emulation is bit-equal.
//   * The loads form a chain (range and target -> the two labels -> the keep / map entries); each group is issued
//     together (GPS_LOADS_ISSUED), three trips to memory.  Measured: that grouping did not move the
//     launch's 14 us, the 64-bit compare in the rank loop did (10.4 us) -- the rank loop of the longest row is what
//     the launch waits for, not memory.
//   * Every index that comes from device memory (scan range, target id, label, order entry) is range-checked before it
//     becomes an address.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gps_dev.h"
#include "gps_dropout.h"
#include "gps_hip.h"
#include "gps_rows_dev.h"

namespace gps_obj_select_ns {

constexpr int kBlock = GPS_OBJ_SELECT_MAX_SCAN;  // 1024: one thread per scan position
constexpr int kWaves = kBlock / 64;
static_assert(kWaves == gps_rows::kSegs, "wave w holds segment w of csrc/gps_rows_dev.h");
constexpr int kMaxSlots = GPS_REFER_MAX_OBJ;    // O <= 512
enum Count { kKept = 0, kCls = 1, kRem = 2, kMulti = 3, kHard = 4, kCounts = 5 };

struct Params {
  int O, M, mode, n_objects, n_labels, keep_stride, R;
  unsigned long long seed;
  const unsigned long long *seed_dev;
  const int32_t *labels, *scan_range, *tgt_obj, *label_map, *order;
  const uint8_t *keep;
  int32_t *row_obj, *tgt_slot, *n_sel, *n_rem;
  uint8_t *is_multiple, *is_hard;
};

template <bool REPLAY>
__global__ __launch_bounds__(kBlock) void obj_select_kernel(const Params p) {
  __shared__ int s_cnt[kCounts][kWaves];
  __shared__ int s_row[kMaxSlots];
  __shared__ int s_rem[kBlock];
  __shared__ __attribute__((aligned(16))) unsigned long long s_key[kBlock];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int O = p.O, M = p.M;
  const bool refer = p.mode == GPS_OBJ_SELECT_REFER;

  int first = p.scan_range[2 * b], last = p.scan_range[2 * b + 1];
  const int len = gps_rows::clamp_range(first, last, p.n_objects);
  long long t_ll = -1;
  if (refer) t_ll = (long long)p.tgt_obj[b] - (long long)first;
  const bool tgt_in = t_ll >= 0 && t_ll < (long long)len;
  if (len > kBlock || (refer && !tgt_in)) {      // block-uniform: the empty row
    if (tid < O) p.row_obj[(size_t)b * O + tid] = -1;
    if (tid == 0) {
      p.tgt_slot[b] = -1;
      p.n_sel[b] = 0;
      p.n_rem[b] = 0;
      p.is_multiple[b] = 0;
      p.is_hard[b] = 0;
    }
    return;
  }
  const int t = refer ? (int)t_ll : -1;
  const int n_labels = p.n_labels;

  // ---- the position's own facts.  The launch is a chain of dependent loads (range -> label -> keep / map entry), each
  // a trip to memory: the two label loads go out together, then the three table loads, before any branch on a value
  const bool in_scan = tid < len;
  int l_t = -1, l = -1;
  if (refer) l_t = p.labels[first + t];          // the same address in every lane
  if (in_scan) l = p.labels[first + tid];
  unsigned long long S = 0;
  if (!REPLAY) S = gps_dropout::effective_seed(p.seed, p.seed_dev);
  GPS_LOADS_ISSUED();
  if (tid < O) s_row[tid] = -1;
  const bool lt_valid = refer && l_t >= 0 && l_t < n_labels;
  const bool valid = in_scan && l >= 0 && l < n_labels;
  int map_t = l_t, mapped = l;
  uint8_t keep_l = 0;
  if (lt_valid && p.label_map) map_t = p.label_map[l_t];
  if (valid) keep_l = p.keep[(size_t)b * p.keep_stride + l];
  if (valid && p.label_map) mapped = p.label_map[l];
  GPS_LOADS_ISSUED();
  const bool kept = valid && keep_l != 0;
  const bool same = refer && in_scan && l == l_t;           // raw labels, as `klabel == tgt_object_label`
  const bool is_cls = kept && same && tid != t;
  const bool is_rem = kept && !(refer && same);
  const bool multi = refer && lt_valid && valid && mapped == map_t;
  const bool hard = refer && lt_valid && valid && l == l_t;

  // the ordered compaction of csrc/gps_rows_dev.h: wave w is segment w
  const int in_kept = gps_rows::seg_ballot(kept, s_cnt[kKept], wave, lane);
  const int in_cls = gps_rows::seg_ballot(is_cls, s_cnt[kCls], wave, lane);
  const int in_rem = gps_rows::seg_ballot(is_rem, s_cnt[kRem], wave, lane);
  gps_rows::seg_ballot(multi, s_cnt[kMulti], wave, lane);
  gps_rows::seg_ballot(hard, s_cnt[kHard], wave, lane);
  __syncthreads();
  int before[3], total[kCounts];
  total[kKept] = gps_rows::seg_sums(s_cnt[kKept], wave, before[kKept]);
  total[kCls] = gps_rows::seg_sums(s_cnt[kCls], wave, before[kCls]);
  total[kRem] = gps_rows::seg_sums(s_cnt[kRem], wave, before[kRem]);
  total[kMulti] = gps_rows::seg_total(s_cnt[kMulti]);
  total[kHard] = gps_rows::seg_total(s_cnt[kHard]);
  const int rank_kept = before[kKept] + in_kept;
  const int rank_cls = before[kCls] + in_cls;
  const int rank_rem = before[kRem] + in_rem;
  const int n_kept = total[kKept], n_cls = total[kCls], n_remained = total[kRem];

  // kept_t is known to thread t only; n needs it everywhere: t is kept iff it counts among the kept of its class
  // (refer: the kept positions are class-mates + remained + t itself when kept)
  const bool tgt_appended = refer && (n_kept == n_cls + n_remained);
  const int n = n_kept + (tgt_appended ? 1 : 0);

  int row_len, n_rem_out = 0;
  if (n <= M) {
    if (kept) s_row[rank_kept] = first + tid;
    if (tid == t) {
      if (tgt_appended) s_row[n_kept] = first + tid;
      p.tgt_slot[b] = tgt_appended ? n_kept : rank_kept;
    }
    row_len = n;
  } else {
    if (refer) {
      if (tid == t) {
        s_row[0] = first + tid;
        p.tgt_slot[b] = 0;
      }
      if (is_cls && 1 + rank_cls < M) s_row[1 + rank_cls] = first + tid;
      row_len = 1 + n_cls < M ? 1 + n_cls : M;
    } else {
      row_len = 0;
    }
    const int n_free = M - row_len;              // block-uniform
    if (n_free > 0) {
      n_rem_out = n_remained;
      if (is_rem) s_rem[rank_rem] = tid;
      if (REPLAY) {
        __syncthreads();
        if (tid < n_free) {
          const int idx = p.order[(size_t)b * p.R + tid];
          if (idx >= 0 && idx < n_remained) s_row[row_len + tid] = first + s_rem[idx];
        }
      } else {
        // the 64-bit key itself goes to LDS: one 64-bit compare per pair of keys instead of three 32-bit ones.  The key
        // past n_rem that completes the last pair is all ones, above every real key (their low word is below 1024)
        const unsigned long long key[1] = {tid < n_remained ? gps_rows::fill_key(S, b, tid) : gps_rows::kPadKey};
        const int n_pairs = (n_remained + 1) >> 1;           // <= kBlock / 2
        if (tid < 2 * n_pairs) s_key[tid] = key[0];
        __syncthreads();
        if (tid < n_remained) {
          int rank[1];
          gps_rows::key_ranks(s_key, n_pairs, key, rank);
          if (rank[0] < n_free) s_row[row_len + rank[0]] = first + s_rem[tid];
        }
      }
      row_len = M;
    }
  }
  __syncthreads();
  if (tid < O) p.row_obj[(size_t)b * O + tid] = s_row[tid];
  if (tid == 0) {
    if (!refer) p.tgt_slot[b] = -1;
    p.n_sel[b] = row_len;
    p.n_rem[b] = n_rem_out;
    p.is_multiple[b] = total[kMulti] > 1 ? 1 : 0;
    p.is_hard[b] = total[kHard] > 2 ? 1 : 0;
  }
}

}  // namespace gps_obj_select_ns

extern "C" int gps_obj_select(int B, int O, int M, int mode, int n_objects, int n_labels, const int32_t *labels,
                              const int32_t *scan_range, const int32_t *tgt_obj, const uint8_t *keep, int keep_stride,
                              const int32_t *label_map, const int32_t *order, int R, uint64_t seed,
                              const uint64_t *seed_dev, int32_t *row_obj, int32_t *tgt_slot, int32_t *n_sel,
                              int32_t *n_rem, uint8_t *is_multiple, uint8_t *is_hard, gps_stream_t stream) {
  using namespace gps_obj_select_ns;
  if (B < 0 || O < 0 || n_objects < 0 || n_labels < 0 || R < 0) return GPS_ERR_INVALID_ARGUMENT;
  if (M < 1 || M > O) return GPS_ERR_INVALID_ARGUMENT;
  if (mode != GPS_OBJ_SELECT_REFER && mode != GPS_OBJ_SELECT_PRETRAIN) return GPS_ERR_INVALID_ARGUMENT;
  if (keep_stride != 0 && keep_stride != n_labels) return GPS_ERR_INVALID_ARGUMENT;
  if (order && R < M) return GPS_ERR_INVALID_ARGUMENT;
  if (mode == GPS_OBJ_SELECT_REFER && M < 2) return GPS_ERR_UNSUPPORTED;
  if (O > kMaxSlots) return GPS_ERR_UNSUPPORTED;
  if (B == 0) return GPS_OK;
  if (!scan_range || !row_obj || !tgt_slot || !n_sel || !n_rem || !is_multiple || !is_hard) return GPS_ERR_INVALID_ARGUMENT;
  if (mode == GPS_OBJ_SELECT_REFER && !tgt_obj) return GPS_ERR_INVALID_ARGUMENT;
  if (n_objects > 0 && !labels) return GPS_ERR_INVALID_ARGUMENT;
  if (n_labels > 0 && !keep) return GPS_ERR_INVALID_ARGUMENT;

  Params p;
  p.O = O; p.M = M; p.mode = mode; p.n_objects = n_objects; p.n_labels = n_labels; p.keep_stride = keep_stride; p.R = R;
  p.seed = seed; p.seed_dev = reinterpret_cast<const unsigned long long *>(seed_dev);
  p.labels = labels; p.scan_range = scan_range; p.tgt_obj = tgt_obj; p.label_map = label_map; p.order = order;
  p.keep = keep;
  p.row_obj = row_obj; p.tgt_slot = tgt_slot; p.n_sel = n_sel; p.n_rem = n_rem;
  p.is_multiple = is_multiple; p.is_hard = is_hard;
  const dim3 grid((unsigned int)B), block(kBlock);
  hipStream_t s = (hipStream_t)stream;
  if (order) hipLaunchKernelGGL(obj_select_kernel<true>, grid, block, 0, s, p);
  else hipLaunchKernelGGL(obj_select_kernel<false>, grid, block, 0, s, p);
  return gps_dev::launch_status();
}
