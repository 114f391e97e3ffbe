// gps_obj_select_qa.hip -- a ScanQA / SQA3D batch from one question id per row, on MI355X (gfx950): which objects (or
// proposals) of the question's scan enter the row, where its target objects sit in it, and the three multi-hot targets
// (tgt_object_id, tgt_object_label, answer_label) with the question's text id and type, in one launch.
//
// Reference (what this one entry replaces on the data-loader workers, per sample):
//   ScanNetScanQAOld.__getitem__  data/datasets/scannet_old.py:326-484  filter :373-392, targets :394-422, crop :425-443,
//                                                                       the pad slot :446-448, multi-hots :453-467
//   ScanNetSQA3D.__getitem__      data/datasets/scannet_old.py:94-232   random.choice of the situation :105-112, the same
//                                                                       selection :123-195, .long() multi-hots :199-213
//
// gps_obj_select_qa   ONE launch, no atomics, no workspace, no scratch, no host sync; every element of every output is
//   written.  Grid: one workgroup of 256 threads per row; position p of the row's scan belongs to thread p % 256, turn
//   p / 256 (up to 4 turns = GPS_OBJ_SELECT_MAX_SCAN positions), so that a wave holds segment 4 * turn + wave of
//   csrc/gps_rows_dev.h in each turn.  The rule is stated in include/gps_hip.h; tests/qa_rows_cases.py restates it.
//   * The question's target list (at most GPS_QA_MAX_TGT entries) lives in LDS: ids, labels and -- 'pred' -- the boxes as
//     gps_box::Box.  Wave 0 marks the first occurrence of every id with one ballot (a repeated entry counts once).  A
//     position finds ITS entry by a walk over the list (broadcast LDS reads): 'gt' by id, 'pred' by the first box it
//     overlaps at IoU >= 0.25 (float64, this file is compiled -ffp-contract=off; Box / iou are gps_box_dev.h's).
//   * Three ballots per turn -- in sel ('gt': kept) or hit ('pred'), class-mate, remained -- give the ordered compaction
//     of gps_rows_dev.h.  The class test needs every entry's `used` flag, so it follows the first barrier.
//   * The row is assembled in LDS (s_row, -1 everywhere first; s_mark = the targets' slots) and stored once, coalesced.
//     The fill is the one of gps_obj_select: replay reads order[b][j]; the device law ranks the 64-bit keys in LDS.
//   * The multi-hots: element a of a row belongs to thread a % 256, which writes its zero first thing (the stores drain
//     under the selection) and its one at the end, in program order, with the kernel's barriers between the two passes;
//     the answer ids are read straight from the CSR.
//   * Every index that comes from device memory (the question id, the ranges and CSR bounds, a target id, a label, an
//     answer id, a pick, an order entry) is range-checked before it becomes an address.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gps_box_dev.h"
#include "gps_dev.h"
#include "gps_dropout.h"
#include "gps_hip.h"
#include "gps_rows_dev.h"

namespace gps_obj_select_qa_ns {

using gps_box::Box;
using gps_box::iou;

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kTurns = gps_rows::kMaxScan / kBlock;        // 4 positions per thread
constexpr int kMaxSlots = GPS_REFER_MAX_OBJ;               // O <= 512
constexpr int kMaxTgt = GPS_QA_MAX_TGT;                    // 32 list entries, all held by wave 0
constexpr int kPadLabel = 5;                               // scannet_old.py:448: the class of the pad slot
enum Count { kSel = 0, kCls = 1, kRem = 2, kCounts = 3 };
static_assert(kTurns * kWaves == gps_rows::kSegs, "a wave's turn is one segment of csrc/gps_rows_dev.h");
static_assert(kMaxTgt <= 64, "wave 0 holds the target list");

struct Params {
  int O, M, A, n_objects, n_labels, keep_rows, R;
  bool matched, train;
  gps_qa_questions q;
  unsigned long long seed;
  const unsigned long long *seed_dev;
  const double *boxes;
  const int32_t *q_idx, *labels, *match_labels, *order, *pick;
  const uint8_t *keep;
  int32_t *row_obj, *n_sel, *n_rem, *n_tgt, *sent_idx;
  int64_t *sqa_type, *obj_labels;
  void *tgt_object_id, *tgt_object_label, *answer_label;
};

// element a of a multi-hot row belongs to thread a % kBlock: its zero and its one are stores of ONE thread, in order
template <typename T>
__device__ __forceinline__ void zero_row(T *row, int n, int tid) {
  for (int a = tid; a < n; a += kBlock) row[a] = (T)0;
}
template <typename T>
__device__ __forceinline__ void set_one(T *row, int n, int id, int tid) {
  if (id >= 0 && id < n && (id % kBlock) == tid) row[id] = (T)1;
}

template <bool PRED, bool REPLAY, typename T>
__global__ __launch_bounds__(kBlock) void obj_select_qa_kernel(const Params p) {
  __shared__ int s_cnt[kCounts][gps_rows::kSegs];
  __shared__ int s_row[kMaxSlots];
  __shared__ uint8_t s_mark[kMaxSlots];
  __shared__ int s_rem[gps_rows::kMaxScan];
  __shared__ __attribute__((aligned(16))) unsigned long long s_key[gps_rows::kMaxScan];
  __shared__ int s_tg[kMaxTgt], s_tlab[kMaxTgt], s_kdist;
  __shared__ uint8_t s_tfirst[kMaxTgt], s_tdist[kMaxTgt], s_tkept[kMaxTgt], s_used[kMaxTgt], s_labuse[kMaxTgt];
  __shared__ Box s_tb[kMaxTgt];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int O = p.O, M = p.M, A = p.A, n_objects = p.n_objects, n_labels = p.n_labels;
  T *const id_row = reinterpret_cast<T *>(p.tgt_object_id) + (size_t)b * O;
  T *const lab_row = reinterpret_cast<T *>(p.tgt_object_label) + (size_t)b * n_labels;
  T *const ans_row = reinterpret_cast<T *>(p.answer_label) + (size_t)b * A;
  // the zeros of the two wide multi-hots go out first: they depend on nothing, every row needs them (the empty one
  // too), and they drain while the selection runs; the ones follow at the end, behind the barriers in between
  zero_row(lab_row, n_labels, tid);
  zero_row(ans_row, A, tid);

  // ---- the question: every table entry is read behind the check of q, every CSR bound is clamped ------------------------
  const int q = p.q_idx[b];
  const bool q_ok = q >= 0 && q < p.q.nq;
  int first = 0, last = 0, sf = 0, sl = 0, tf = 0, tl = 0, af = 0, al = 0, vf = 0, vl = 0;
  if (q_ok) {
    first = p.q.ann_range[2 * q], last = p.q.ann_range[2 * q + 1];
    if (PRED) sf = p.q.prop_range[2 * q], sl = p.q.prop_range[2 * q + 1];
    tf = p.q.tgt_first[q], tl = p.q.tgt_first[q + 1];
    af = p.q.ans_first[q], al = p.q.ans_first[q + 1];
    vf = p.q.var_first[q], vl = p.q.var_first[q + 1];
  }
  int P = gps_rows::clamp_range(first, last, n_objects);   // 'gt': sel is taken from the annotated objects
  if (PRED) P = gps_rows::clamp_range(sf, sl, n_objects);
  else sf = first;
  int kT = gps_rows::clamp_range(tf, tl, p.q.n_tgt);
  kT = kT < kMaxTgt ? kT : kMaxTgt;
  const int nA = gps_rows::clamp_range(af, al, p.q.n_ans);
  const int nV = gps_rows::clamp_range(vf, vl, p.q.n_var);
  const bool skip = !q_ok || P > gps_rows::kMaxScan;       // block-uniform
  if (skip) kT = 0;

  bool bad = skip;
  if (tid < kMaxTgt) {
    s_tfirst[tid] = 0;
    s_tdist[tid] = 0;
    s_tkept[tid] = 0;
    s_used[tid] = 0;
    s_labuse[tid] = 0;
  }
  if (tid < kT) {
    const int g = p.q.tgt_id[tf + tid];
    s_tg[tid] = g;
    s_tlab[tid] = p.q.tgt_label[tf + tid];
    if (g < first || g >= last) {
      bad = true;                                  // a target outside its scan: never an address
    } else if (PRED) {
      Box t;
      t.load(p.boxes + (size_t)g * 6);
      s_tb[tid] = t;
    }
  }
  for (int i = tid; i < O; i += kBlock) {
    s_row[i] = -1;
    s_mark[i] = 0;
  }
  if (__syncthreads_or(bad ? 1 : 0)) {             // block-uniform: the empty row
    for (int i = tid; i < O; i += kBlock) {
      p.row_obj[(size_t)b * O + i] = -1;
      p.obj_labels[(size_t)b * O + i] = -100;
      id_row[i] = (T)0;
    }
    if (tid == 0) {
      p.n_sel[b] = 0;
      p.n_rem[b] = 0;
      p.n_tgt[b] = 0;
      p.sent_idx[b] = -1;
      p.sqa_type[b] = 0;
    }
    return;
  }

  // ---- the variant: a replayed random.choice, the device law (stream S + 4) or the first --------------------------------
  unsigned long long S = 0;
  if (!REPLAY || (p.train && !p.pick)) S = gps_dropout::effective_seed(p.seed, p.seed_dev);
  int pk = 0;
  if (p.pick) pk = p.pick[b];
  else if (p.train && nV > 0) pk = (int)(gps_dropout::rng_u32(S + 4ull, (unsigned long long)b) % (unsigned int)nV);
  if (pk < 0 || pk >= nV) pk = 0;
  const int var = vf + pk;                         // below n_var when nV > 0
  const bool keep_ok = p.keep_rows == 0 || (nV > 0 && var < p.keep_rows);
  const size_t keep_at = p.keep_rows == 0 ? 0 : (size_t)var * (size_t)n_labels;

  // ---- the list: first occurrences and their ranks, one ballot of wave 0 ------------------------------------------------
  if (wave == 0) {
    bool fst = lane < kT;
    if (fst) {
      const int g = s_tg[lane];
      for (int j = 0; j < lane; ++j) fst = fst && s_tg[j] != g;
    }
    const unsigned long long m = __ballot(fst);
    if (lane < kT) {
      s_tfirst[lane] = fst ? 1 : 0;
      s_tdist[lane] = (uint8_t)__popcll(m & ((1ull << lane) - 1ull));
    }
    if (lane == 0) s_kdist = __popcll(m);
  }

  // ---- the position's own facts: its label, kept or not, its entry of the list -------------------------------------------
  int in_seg[kCounts][kTurns];
  int tix[kTurns], lab[kTurns];
  bool insel[kTurns], kept[kTurns];
#pragma unroll
  for (int j = 0; j < kTurns; ++j) {
    const int pos = j * kBlock + tid;
    const bool in = pos < P;
    const int g = sf + pos;                        // in [0, n_objects) when `in`
    tix[j] = -1;
    lab[j] = -1;
    kept[j] = false;
    if (in) {
      const int l = p.labels[g];
      lab[j] = p.matched ? p.match_labels[g] : l;
      if (PRED) {
        Box pb;
        pb.load(p.boxes + (size_t)g * 6);
        for (int i = 0; i < kT; ++i)               // the FIRST target it hits (scannet_old.py:413-422)
          if (iou(pb, s_tb[i]) >= 0.25) {
            tix[j] = i;
            break;
          }
      } else {
        if (keep_ok && l >= 0 && l < n_labels) kept[j] = p.keep[keep_at + (size_t)l] != 0;
        for (int i = 0; i < kT; ++i)               // the first place of a repeated entry
          if (s_tg[i] == g) {
            tix[j] = i;
            break;
          }
        if (tix[j] >= 0) s_tkept[tix[j]] = kept[j] ? 1 : 0;
      }
      if (tix[j] >= 0) s_used[tix[j]] = 1;         // several positions may hit one box: the same byte, the same value
    }
    insel[j] = PRED ? in : kept[j];
    in_seg[kSel][j] = gps_rows::seg_ballot(PRED ? tix[j] >= 0 : kept[j], s_cnt[kSel], j * kWaves + wave, lane);
  }
  __syncthreads();

  // ---- class-mates and remained among the non-targets of sel -------------------------------------------------------------
  bool mate[kTurns], rest[kTurns];
#pragma unroll
  for (int j = 0; j < kTurns; ++j) {
    bool c = false;
    if (insel[j] && tix[j] < 0)
      for (int i = 0; i < kT; ++i) c = c || (s_used[i] != 0 && s_tlab[i] == lab[j]);
    mate[j] = insel[j] && tix[j] < 0 && c;
    rest[j] = insel[j] && tix[j] < 0 && !c;
    in_seg[kCls][j] = gps_rows::seg_ballot(mate[j], s_cnt[kCls], j * kWaves + wave, lane);
    in_seg[kRem][j] = gps_rows::seg_ballot(rest[j], s_cnt[kRem], j * kWaves + wave, lane);
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
  int n_unkept = 0;                                // 'gt': the targets appended behind the kept positions
  if (!PRED)
    for (int i = 0; i < kT; ++i) n_unkept += (s_tfirst[i] != 0 && s_tkept[i] == 0) ? 1 : 0;
  const int k = PRED ? total[kSel] : s_kdist;      // distinct targets
  const int n = PRED ? P : total[kSel] + n_unkept;
  const int kr = k < M ? k : M;                    // ... of which the row holds
  const int n_cls = total[kCls], n_remained = total[kRem];

  int row_len, n_rem_out = 0;                      // block-uniform
  if (n <= M) {
#pragma unroll
    for (int j = 0; j < kTurns; ++j) {
      const int pos = j * kBlock + tid;
      if (pos >= P) continue;
      int slot = PRED ? pos : rank[kSel][j];
      if (insel[j]) s_row[slot] = sf + pos;
      if (tix[j] >= 0) {
        if (!insel[j]) {                           // 'gt', not kept: behind the kept ones, in list order
          int u = 0;
          for (int i = 0; i < tix[j]; ++i) u += (s_tfirst[i] != 0 && s_tkept[i] == 0) ? 1 : 0;
          slot = total[kSel] + u;
          s_row[slot] = sf + pos;
        }
        s_mark[slot] = 1;
        s_labuse[tix[j]] = 1;
      }
    }
    row_len = n;
  } else {
#pragma unroll
    for (int j = 0; j < kTurns; ++j) {
      const int pos = j * kBlock + tid;
      if (tix[j] >= 0) {                           // 'gt': list order; 'pred': ascending.  The first M of them
        const int slot = PRED ? rank[kSel][j] : (int)s_tdist[tix[j]];
        if (slot < M) {
          s_row[slot] = sf + pos;
          s_mark[slot] = 1;
          s_labuse[tix[j]] = 1;
        }
      }
      if (mate[j] && kr + rank[kCls][j] < M) s_row[kr + rank[kCls][j]] = sf + pos;
    }
    row_len = kr + n_cls < M ? kr + n_cls : M;
    const int n_free = M - row_len;                // block-uniform; n_remained >= n_free because n > M
    if (n_free > 0) {
      n_rem_out = n_remained;
#pragma unroll
      for (int j = 0; j < kTurns; ++j)
        if (rest[j]) s_rem[rank[kRem][j]] = j * kBlock + tid;
      if (REPLAY) {
        __syncthreads();
        for (int s = tid; s < n_free; s += kBlock) {
          const int idx = p.order[(size_t)b * p.R + s];
          if (idx >= 0 && idx < n_remained) s_row[row_len + s] = sf + s_rem[idx];
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
          int kr_[kTurns];
          gps_rows::key_ranks(s_key, n_pairs, key, kr_);
#pragma unroll
          for (int j = 0; j < kTurns; ++j) {
            const int r = j * kBlock + tid;
            if (r < n_remained && kr_[j] < n_free) s_row[row_len + kr_[j]] = sf + s_rem[r];
          }
        }
      }
      row_len = M;
    }
  }
  __syncthreads();

  // ---- the row and the three multi-hots ---------------------------------------------------------------------------------
  for (int i = tid; i < O; i += kBlock) {
    const int g = s_row[i];                        // a real id is one this kernel wrote: inside the scan's range
    p.row_obj[(size_t)b * O + i] = g;
    p.obj_labels[(size_t)b * O + i] = g >= 0 ? (int64_t)(p.matched ? p.match_labels[g] : p.labels[g]) : (int64_t)-100;
    id_row[i] = (T)(k == 0 ? (i == row_len ? 1 : 0) : s_mark[i]);       // no target: the pad slot behind the row
  }
  for (int i = 0; i < kT; ++i)
    if (s_labuse[i] != 0) set_one(lab_row, n_labels, s_tlab[i], tid);
  if (k == 0) set_one(lab_row, n_labels, kPadLabel, tid);
  for (int i = 0; i < nA; ++i) set_one(ans_row, A, p.q.ans_id[af + i], tid);
  if (tid == 0) {
    p.n_sel[b] = row_len;
    p.n_rem[b] = n_rem_out;
    p.n_tgt[b] = kr;
    p.sent_idx[b] = nV > 0 ? p.q.var_text[var] : -1;
    p.sqa_type[b] = (int64_t)p.q.sqa_type[q];
  }
}

template <bool PRED, bool REPLAY>
void launch_typed(bool as_int64, const Params &p, int B, hipStream_t s) {
  const dim3 grid((unsigned int)B), block(kBlock);
  if (as_int64) hipLaunchKernelGGL((obj_select_qa_kernel<PRED, REPLAY, int64_t>), grid, block, 0, s, p);
  else hipLaunchKernelGGL((obj_select_qa_kernel<PRED, REPLAY, float>), grid, block, 0, s, p);
}

}  // namespace gps_obj_select_qa_ns

extern "C" int gps_obj_select_qa(int B, int O, int M, int A, int n_objects, int n_labels, int flags,
                                 const gps_qa_questions *questions, const int32_t *q_idx, const double *boxes,
                                 const int32_t *labels, const int32_t *match_labels, const uint8_t *keep, int keep_rows,
                                 const int32_t *order, int R, const int32_t *pick, uint64_t seed,
                                 const uint64_t *seed_dev, int32_t *row_obj, int32_t *n_sel, int32_t *n_rem,
                                 int32_t *n_tgt, int32_t *sent_idx, int64_t *sqa_type, int64_t *obj_labels,
                                 void *tgt_object_id, void *tgt_object_label, void *answer_label, gps_stream_t stream) {
  using namespace gps_obj_select_qa_ns;
  if (B < 0 || O < 0 || A < 0 || n_objects < 0 || n_labels < 0 || keep_rows < 0 || R < 0) return GPS_ERR_INVALID_ARGUMENT;
  if (M < 1 || M > O) return GPS_ERR_INVALID_ARGUMENT;
  if (order && R < M) return GPS_ERR_INVALID_ARGUMENT;
  if (flags & ~(GPS_QA_PRED | GPS_QA_MATCHED | GPS_QA_TRAIN | GPS_QA_INT64)) return GPS_ERR_INVALID_ARGUMENT;
  if (!questions) return GPS_ERR_INVALID_ARGUMENT;
  const gps_qa_questions &q = *questions;
  if (q.nq < 0 || q.n_tgt < 0 || q.n_ans < 0 || q.n_var < 0) return GPS_ERR_INVALID_ARGUMENT;
  if (O > kMaxSlots) return GPS_ERR_UNSUPPORTED;
  if (B == 0) return GPS_OK;
  const bool pred = (flags & GPS_QA_PRED) != 0, matched = (flags & GPS_QA_MATCHED) != 0;
  if (!q_idx || !row_obj || !n_sel || !n_rem || !n_tgt || !sent_idx || !sqa_type || !obj_labels || !tgt_object_id) return GPS_ERR_INVALID_ARGUMENT;
  if ((n_labels > 0 && !tgt_object_label) || (A > 0 && !answer_label)) return GPS_ERR_INVALID_ARGUMENT;
  if (q.nq > 0 && (!q.ann_range || !q.tgt_first || !q.ans_first || !q.sqa_type || !q.var_first || (pred && !q.prop_range)))
    return GPS_ERR_INVALID_ARGUMENT;
  if ((q.n_tgt > 0 && (!q.tgt_id || !q.tgt_label)) || (q.n_ans > 0 && !q.ans_id) || (q.n_var > 0 && !q.var_text))
    return GPS_ERR_INVALID_ARGUMENT;
  if (n_objects > 0 && (!labels || (matched && !match_labels) || (pred && !boxes))) return GPS_ERR_INVALID_ARGUMENT;
  if (!pred && n_labels > 0 && !keep) return GPS_ERR_INVALID_ARGUMENT;

  Params p;
  p.O = O; p.M = M; p.A = A; p.n_objects = n_objects; p.n_labels = n_labels; p.keep_rows = keep_rows; p.R = R;
  p.matched = matched; p.train = (flags & GPS_QA_TRAIN) != 0;
  p.q = q;
  p.seed = seed; p.seed_dev = reinterpret_cast<const unsigned long long *>(seed_dev);
  p.boxes = boxes; p.q_idx = q_idx; p.labels = labels; p.match_labels = match_labels; p.order = order; p.pick = pick;
  p.keep = keep;
  p.row_obj = row_obj; p.n_sel = n_sel; p.n_rem = n_rem; p.n_tgt = n_tgt; p.sent_idx = sent_idx; p.sqa_type = sqa_type;
  p.obj_labels = obj_labels;
  p.tgt_object_id = tgt_object_id; p.tgt_object_label = tgt_object_label; p.answer_label = answer_label;
  hipStream_t s = (hipStream_t)stream;
  const bool as_int64 = (flags & GPS_QA_INT64) != 0;
  if (pred) {
    if (order) launch_typed<true, true>(as_int64, p, B, s);
    else launch_typed<true, false>(as_int64, p, B, s);
  } else {
    if (order) launch_typed<false, true>(as_int64, p, B, s);
    else launch_typed<false, false>(as_int64, p, B, s);
  }
  return gps_dev::launch_status();
}
