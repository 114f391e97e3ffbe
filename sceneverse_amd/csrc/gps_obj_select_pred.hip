// gps_obj_select_pred.hip -- which PROPOSALS of a scan enter a `pc_type: 'pred'` ScanRefer row, on MI355X (gfx950):
// the IoU-matched labels once per resident scene set, then per batch the IoU hits of the referred object, the crop and
// the random fill in one launch, with the target tensors of gps_refer_targets written from what the launch already holds.
//
// Reference (what the two entries replace on the data-loader workers, per sample):
//   ScanBase._getitem_refer  data/datasets/base.py:353-366  proposal labels by the first IoU >= 0.25 match
//                            data/datasets/base.py:396-417  tgt_object_id, tgt_object_id_iou25 / _iou50 lists
//                            data/datasets/base.py:420-450  the crop: hits first, the target's class, random.shuffle
//                            data/datasets/base.py:453-454, :478-488  target id, flag vectors, is_multiple / is_hard
//   ScanNetSpatialRefer      data/datasets/scannet.py:50, :70-76  max_obj_len - 1, the label counts
//
// gps_proposal_labels   one launch over all proposals, one thread per proposal, a serial walk over its scan's annotated
//   range; float64, this file is compiled -ffp-contract=off; Box / iou are those of gps_refer_targets (gps_box_dev.h).
// gps_obj_select_pred   ONE launch, no atomics, no workspace, no scratch, no host sync; every element of every output
//   is written.  Grid: one workgroup of 256 threads per row; position p of the row's proposals belongs to thread p % 256,
//   turn p / 256 (up to 4 turns = GPS_OBJ_SELECT_MAX_SCAN positions), so that a wave holds segment 4 * turn + wave of
//   csrc/gps_rows_dev.h in each turn.  The rule is stated in include/gps_hip.h; tests/pred_rows_cases.py restates it.
//   * The target's box is loaded once per workgroup (six lanes, LDS); each position loads its own box and matched label
//     once.  The two hit flags and the matched label of every position stay in LDS (s_flag, s_lab): the target outputs
//     of a slot are looked up there, nothing is computed twice.
//   * Three ballots per turn -- pinned (hit at 0.25), class-mate, remained -- give the ordered compaction of
//     gps_rows_dev.h; the label counts behind is_multiple / is_hard are two more ballots per 256 annotated objects.
//   * The row is assembled in LDS (s_row, -1 everywhere first) and stored once, coalesced.  The fill is the one of
//     gps_obj_select: replay reads order[b][j]; the device law ranks the 64-bit keys in LDS (key_ranks, four keys per
//     thread against each pair read).
//   * Every index that comes from device memory (the two ranges, the target id, a label, an order entry) is
//     range-checked before it becomes an address.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gps_box_dev.h"
#include "gps_dev.h"
#include "gps_dropout.h"
#include "gps_hip.h"
#include "gps_rows_dev.h"

namespace gps_obj_select_pred_ns {

using gps_box::Box;
using gps_box::iou;

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kTurns = gps_rows::kMaxScan / kBlock;        // 4 positions per thread
constexpr int kMaxSlots = GPS_REFER_MAX_OBJ;               // O <= 512
constexpr int kSlotTurns = kMaxSlots / kBlock;
enum Count { kPin = 0, kCls = 1, kRem = 2, kCounts = 3 };
enum Kind { kNone = 0, kPinned = 1, kMate = 2, kRest = 3 };   // of a position: outside the scan, hit at 0.25, of the target's class, the others
static_assert(kTurns * kWaves == gps_rows::kSegs, "a wave's turn is one segment of csrc/gps_rows_dev.h");

// ---- matched labels, once per PackedScans ------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void proposal_labels_kernel(int n_props, int n_objects, const double *__restrict__ boxes,
                                                                  const int32_t *__restrict__ labels,
                                                                  const int32_t *__restrict__ prop_id,
                                                                  const int32_t *__restrict__ ann_range,
                                                                  int32_t *__restrict__ match_labels) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n_props) return;
  const int g = prop_id[i];
  if (g < 0 || g >= n_objects) return;             // never an address
  int first = ann_range[2 * i], last = ann_range[2 * i + 1];
  gps_rows::clamp_range(first, last, n_objects);
  Box p, q;
  p.load(boxes + (size_t)g * 6);
  int label = labels[g];
  // the label of the FIRST annotated object of the scan that overlaps by >= 0.25 (base.py:359-366)
  for (int j = first; j < last; ++j) {
    q.load(boxes + (size_t)j * 6);
    if (iou(q, p) >= 0.25) {
      label = labels[j];
      break;
    }
  }
  match_labels[g] = label;
}

// ---- the row ---------------------------------------------------------------------------------------------------------
struct Params {
  int O, M, n_objects, n_labels, R;
  unsigned long long seed;
  const unsigned long long *seed_dev;
  const double *boxes;
  const int32_t *labels, *match_labels, *scan_range, *prop_range, *tgt_obj, *tgt_label, *label_map, *order;
  int32_t *row_obj, *tgt_slot, *n_sel, *n_rem;
  uint8_t *is_multiple, *is_hard;
  int64_t *iou25, *iou50, *tgt_id, *obj_labels;    // all or none
};

template <bool REPLAY>
__global__ __launch_bounds__(kBlock) void obj_select_pred_kernel(const Params p) {
  __shared__ int s_cnt[kCounts][gps_rows::kSegs];
  __shared__ int s_flags[2][kWaves];               // multi, hard
  __shared__ int s_real[kSlotTurns][kWaves];
  __shared__ double s_tbox[6];
  __shared__ int s_row[kMaxSlots];
  __shared__ int s_rem[gps_rows::kMaxScan];
  __shared__ int s_lab[gps_rows::kMaxScan];
  __shared__ uint8_t s_flag[gps_rows::kMaxScan];
  __shared__ __attribute__((aligned(16))) unsigned long long s_key[gps_rows::kMaxScan];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int O = p.O, M = p.M, n_objects = p.n_objects, n_labels = p.n_labels;
  const bool targets = p.iou25 != nullptr;

  int first = p.scan_range[2 * b], last = p.scan_range[2 * b + 1];
  int pf = p.prop_range[2 * b], pl = p.prop_range[2 * b + 1];
  const int tgt = p.tgt_obj[b];
  gps_rows::clamp_range(first, last, n_objects);
  const int P = gps_rows::clamp_range(pf, pl, n_objects);
  if (P > gps_rows::kMaxScan || tgt < first || tgt >= last) {     // block-uniform: the empty row
    for (int i = tid; i < O; i += kBlock) {
      p.row_obj[(size_t)b * O + i] = -1;
      if (targets) {
        p.iou25[(size_t)b * O + i] = 0;
        p.iou50[(size_t)b * O + i] = 0;
        p.obj_labels[(size_t)b * O + i] = -100;
      }
    }
    if (tid == 0) {
      p.tgt_slot[b] = -1;
      p.n_sel[b] = 0;
      p.n_rem[b] = 0;
      p.is_multiple[b] = 0;
      p.is_hard[b] = 0;
      if (targets) p.tgt_id[b] = 0;                // no hit: the row's length
    }
    return;
  }
  // tgt lies in [first, last) and that inside [0, n_objects)
  if (tid < 6) s_tbox[tid] = p.boxes[(size_t)tgt * 6 + tid];
  const int l_t = p.tgt_label ? p.tgt_label[b] : p.labels[tgt];
  unsigned long long S = 0;
  if (!REPLAY) S = gps_dropout::effective_seed(p.seed, p.seed_dev);
  for (int i = tid; i < O; i += kBlock) s_row[i] = -1;
  __syncthreads();
  Box q;
  q.load(s_tbox);

  // ---- is_multiple / is_hard over the scan's ANNOTATED objects (scannet.py:70-76, base.py:485-488) -----------------------
  const bool lt_valid = l_t >= 0 && l_t < n_labels;
  int map_t = l_t;
  if (lt_valid && p.label_map) map_t = p.label_map[l_t];
  int n_multi = 0, n_hard = 0;                     // wave-uniform
  for (int a0 = first; a0 < last; a0 += kBlock) {  // block-uniform trip count
    const int a = a0 + tid;
    int l = -1;
    if (a < last) l = p.labels[a];
    const bool valid = lt_valid && l >= 0 && l < n_labels;
    int mapped = l;
    if (valid && p.label_map) mapped = p.label_map[l];
    n_multi += __popcll(__ballot(valid && mapped == map_t));
    n_hard += __popcll(__ballot(valid && l == l_t));
  }
  if (lane == 0) {
    s_flags[0][wave] = n_multi;
    s_flags[1][wave] = n_hard;
  }

  // ---- the position's own facts: hit flags against the target, matched label --------------------------------------------
  int in_seg[kCounts][kTurns];
  int kind[kTurns];                                // kNone / kPinned / kMate / kRest: an integer per lane, not three lane masks
#pragma unroll
  for (int j = 0; j < kTurns; ++j) {
    const int pos = j * kBlock + tid;
    const bool in = pos < P;
    bool h25 = false, h50 = false;
    int m = -1;
    if (in) {
      Box pb;
      pb.load(p.boxes + (size_t)(pf + pos) * 6);
      m = p.match_labels[pf + pos];
      const double v = iou(pb, q);
      h25 = v >= 0.25;
      h50 = v >= 0.5;
      s_lab[pos] = m;
      s_flag[pos] = (uint8_t)((h25 ? 1 : 0) | (h50 ? 2 : 0));
    }
    kind[j] = !in ? kNone : (h25 ? kPinned : (m == l_t ? kMate : kRest));
    const int seg = j * kWaves + wave;
    in_seg[kPin][j] = gps_rows::seg_ballot(kind[j] == kPinned, s_cnt[kPin], seg, lane);
    in_seg[kCls][j] = gps_rows::seg_ballot(kind[j] == kMate, s_cnt[kCls], seg, lane);
    in_seg[kRem][j] = gps_rows::seg_ballot(kind[j] == kRest, s_cnt[kRem], seg, lane);
  }

  __syncthreads();

  int rank[kCounts][kTurns], total[kCounts];
#pragma unroll
  for (int j = 0; j < kTurns; ++j) {
#pragma unroll
    for (int c = 0; c < kCounts; ++c) {
      int before;
      total[c] = gps_rows::seg_sums(s_cnt[c], j * kWaves + wave, before);
      rank[c][j] = before + in_seg[c][j];
    }
  }
  const int k = total[kPin], n_cls = total[kCls], n_remained = total[kRem];

  int row_len, n_rem_out = 0, slot_t = -1;         // block-uniform, but for slot_t when P <= M
  if (P <= M) {
#pragma unroll
    for (int j = 0; j < kTurns; ++j) {
      const int pos = j * kBlock + tid;
      if (pos < P) s_row[pos] = pf + pos;
      if (kind[j] == kPinned && rank[kPin][j] == k - 1) p.tgt_slot[b] = pos;     // the largest pinned position: one thread
    }
    row_len = P;
  } else if (k >= M) {                             // the M largest of pinned
#pragma unroll
    for (int j = 0; j < kTurns; ++j) {
      const int slot = rank[kPin][j] - (k - M);
      if (kind[j] == kPinned && slot >= 0) s_row[slot] = pf + j * kBlock + tid;
    }
    row_len = M;
    slot_t = M - 1;
  } else {
#pragma unroll
    for (int j = 0; j < kTurns; ++j) {
      const int pos = j * kBlock + tid;
      if (kind[j] == kPinned) s_row[rank[kPin][j]] = pf + pos;
      if (kind[j] == kMate && k + rank[kCls][j] < M) s_row[k + rank[kCls][j]] = pf + pos;
    }
    row_len = k + n_cls < M ? k + n_cls : M;
    slot_t = k - 1;                                // -1 when nothing is pinned
    const int n_free = M - row_len;                // block-uniform; n_remained >= n_free because P > M
    if (n_free > 0) {
      n_rem_out = n_remained;
#pragma unroll
      for (int j = 0; j < kTurns; ++j)
        if (kind[j] == kRest) s_rem[rank[kRem][j]] = j * kBlock + tid;
      if (REPLAY) {
        __syncthreads();
        for (int s = tid; s < n_free; s += kBlock) {
          const int idx = p.order[(size_t)b * p.R + s];
          if (idx >= 0 && idx < n_remained) s_row[row_len + s] = pf + s_rem[idx];
        }
      } else {
        unsigned long long key[kTurns];
        const int n_pairs = (n_remained + 1) >> 1;           // <= kMaxScan / 2
#pragma unroll
        for (int j = 0; j < kTurns; ++j) {
          const int r = j * kBlock + tid;
          key[j] = r < n_remained ? gps_rows::fill_key(S, b, r) : gps_rows::kPadKey;
          if (r < 2 * n_pairs) s_key[r] = key[j];
        }
        __syncthreads();
        if (tid < n_remained) {                    // a thread's later entries exist only when its first does
          int kr[kTurns];
          gps_rows::key_ranks(s_key, n_pairs, key, kr);
#pragma unroll
          for (int j = 0; j < kTurns; ++j) {
            const int r = j * kBlock + tid;
            if (r < n_remained && kr[j] < n_free) s_row[row_len + kr[j]] = pf + s_rem[r];
          }
        }
      }
      row_len = M;
    }
  }
  __syncthreads();

  // ---- the row, and what gps_refer_targets('pred') would make of it -----------------------------------------------------
#pragma unroll
  for (int j = 0; j < kSlotTurns; ++j) {
    const int i = j * kBlock + tid;
    const int g = i < O ? s_row[i] : -1;
    const bool real = g >= 0;                      // g - pf is a position below P: this kernel wrote it
    if (i < O) {
      p.row_obj[(size_t)b * O + i] = g;
      if (targets) {
        const int f = real ? s_flag[g - pf] : 0;
        p.iou25[(size_t)b * O + i] = f & 1;
        p.iou50[(size_t)b * O + i] = (f >> 1) & 1;
        p.obj_labels[(size_t)b * O + i] = real ? (int64_t)s_lab[g - pf] : (int64_t)-100;
      }
    }
    if (targets) {                                 // block-uniform
      const unsigned long long mreal = __ballot(real);
      if (lane == 0) s_real[j][wave] = __popcll(mreal);
    }
  }
  if (targets) __syncthreads();
  if (tid == 0) {
    if (P > M) p.tgt_slot[b] = slot_t;
    else if (k == 0) p.tgt_slot[b] = -1;
    p.n_sel[b] = row_len;
    p.n_rem[b] = n_rem_out;
    int multi = 0, hard = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      multi += s_flags[0][w];
      hard += s_flags[1][w];
    }
    p.is_multiple[b] = multi > 1 ? 1 : 0;
    p.is_hard[b] = hard > 2 ? 1 : 0;
  }
  if (targets) {
    // tgt_id: the LARGEST slot with a hit at 0.25, else the number of real slots (base.py:410, :453-454)
    int n_b = 0;
#pragma unroll
    for (int j = 0; j < kSlotTurns; ++j)
#pragma unroll
      for (int w = 0; w < kWaves; ++w) n_b += s_real[j][w];
    if (P > M) {
      if (tid == 0) p.tgt_id[b] = slot_t >= 0 ? slot_t : n_b;
    } else {
      if (k == 0 && tid == 0) p.tgt_id[b] = n_b;
#pragma unroll
      for (int j = 0; j < kTurns; ++j)
        if (kind[j] == kPinned && rank[kPin][j] == k - 1) p.tgt_id[b] = j * kBlock + tid;
    }
  }
}

}  // namespace gps_obj_select_pred_ns

extern "C" int gps_proposal_labels(int n_props, int n_objects, const double *boxes, const int32_t *labels,
                                   const int32_t *prop_id, const int32_t *ann_range, int32_t *match_labels,
                                   gps_stream_t stream) {
  using namespace gps_obj_select_pred_ns;
  if (n_props < 0 || n_objects < 0) return GPS_ERR_INVALID_ARGUMENT;
  if (n_props == 0) return GPS_OK;
  if (!boxes || !labels || !prop_id || !ann_range || !match_labels) return GPS_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(proposal_labels_kernel, dim3((n_props + kBlock - 1) / kBlock), dim3(kBlock), 0, (hipStream_t)stream,
                     n_props, n_objects, boxes, labels, prop_id, ann_range, match_labels);
  return gps_dev::launch_status();
}

extern "C" int gps_obj_select_pred(int B, int O, int M, int n_objects, int n_labels, const double *boxes,
                                   const int32_t *labels, const int32_t *match_labels, const int32_t *scan_range,
                                   const int32_t *prop_range, const int32_t *tgt_obj, const int32_t *tgt_label,
                                   const int32_t *label_map, const int32_t *order, int R, uint64_t seed,
                                   const uint64_t *seed_dev, int32_t *row_obj, int32_t *tgt_slot, int32_t *n_sel,
                                   int32_t *n_rem, uint8_t *is_multiple, uint8_t *is_hard, int64_t *iou25,
                                   int64_t *iou50, int64_t *tgt_id, int64_t *obj_labels, gps_stream_t stream) {
  using namespace gps_obj_select_pred_ns;
  if (B < 0 || O < 0 || n_objects < 0 || n_labels < 0 || R < 0) return GPS_ERR_INVALID_ARGUMENT;
  if (M < 1 || M > O) return GPS_ERR_INVALID_ARGUMENT;
  if (order && R < M) return GPS_ERR_INVALID_ARGUMENT;
  const int n_tgt = (iou25 ? 1 : 0) + (iou50 ? 1 : 0) + (tgt_id ? 1 : 0) + (obj_labels ? 1 : 0);
  if (n_tgt != 0 && n_tgt != 4) return GPS_ERR_INVALID_ARGUMENT;
  if (M < 2) return GPS_ERR_UNSUPPORTED;
  if (O > kMaxSlots) return GPS_ERR_UNSUPPORTED;
  if (B == 0) return GPS_OK;
  if (!scan_range || !prop_range || !tgt_obj || !row_obj || !tgt_slot || !n_sel || !n_rem || !is_multiple || !is_hard)
    return GPS_ERR_INVALID_ARGUMENT;
  if (n_objects > 0 && (!boxes || !labels || !match_labels)) return GPS_ERR_INVALID_ARGUMENT;

  Params p;
  p.O = O; p.M = M; p.n_objects = n_objects; p.n_labels = n_labels; p.R = R;
  p.seed = seed; p.seed_dev = reinterpret_cast<const unsigned long long *>(seed_dev);
  p.boxes = boxes; p.labels = labels; p.match_labels = match_labels; p.scan_range = scan_range; p.prop_range = prop_range;
  p.tgt_obj = tgt_obj; p.tgt_label = tgt_label; p.label_map = label_map; p.order = order;
  p.row_obj = row_obj; p.tgt_slot = tgt_slot; p.n_sel = n_sel; p.n_rem = n_rem;
  p.is_multiple = is_multiple; p.is_hard = is_hard;
  p.iou25 = iou25; p.iou50 = iou50; p.tgt_id = tgt_id; p.obj_labels = obj_labels;
  const dim3 grid((unsigned int)B), block(kBlock);
  hipStream_t s = (hipStream_t)stream;
  if (order) hipLaunchKernelGGL(obj_select_pred_kernel<true>, grid, block, 0, s, p);
  else hipLaunchKernelGGL(obj_select_pred_kernel<false>, grid, block, 0, s, p);
  return gps_dev::launch_status();
}
