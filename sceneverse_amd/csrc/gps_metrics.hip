// gps_metrics.hip -- accuracy counters of the pre-train, ReferIt3D and object-class evaluators on MI355X (gfx950).
//
// Reference (what these two entries replace):
//   PretrainEval.batch_metrics / update / record   evaluator/pretrain_eval.py:21-86
//   ReferIt3DEval.batch_metrics                    evaluator/referit3d_eval.py:14-83
//   PretrainObjEval.batch_metrics                  evaluator/objcls_eval.py:14-23
//   BaseEvaluator.update / record                  evaluator/build.py:26-54
// Every figure there is  (argmax(logits[row]) == label[row]) summed over the rows some mask selects, divided by the
// number of selected rows -- each with a `.item()` read-back.  Here the sums stay integers on the device:
//
// gps_cls_hits      up to GPS_CLS_HITS_MAX_PROBLEMS problems in ONE launch.  A workgroup finds its problem from the block
//   offsets the host computed (a wave-uniform search over at most 8 words) and takes
//     narrow rows (cols <= GPS_CLS_HITS_WAVE_MAX_COLS)  one wave per row, kBlock / 64 rows per workgroup;
//     wide rows                                         one workgroup per row, the per-wave candidates folded through LDS.
//   Either way a row is a scalar head up to its first 16-byte boundary, 16-byte loads (four in flight per lane where
//   the row is long enough) and a scalar tail; the per-lane candidates are folded by shuffles.
//   Rows that are not counted (past *rows_dev, sel false, ignored label) are not read.  No load leaves
//   [row * ld, row * ld + cols) of a counted row.  The counts leave a workgroup as one integer atomic per non-zero counter;
//   integer addition makes the result independent of the arrival order, and no workgroup reads what another wrote.
// gps_metrics_fold  one workgroup, one thread per term: the integer counts become the reference's float64 bookkeeping
//   (ratio, ratio * weight added to the running sum, the mean of the ratios), one rounding per operation -- this file is
//   compiled with -ffp-contract=off -- and the batch's counters go back to zero.
// gps_answer_hits   ScanQAEval / SQA3DEval.batch_metrics (evaluator/scanqa_eval.py:29-45, evaluator/sqa3d_eval.py:78-116):
//   a row's k best answers in the order of `Best::beats` extended to every place -- place j is the best candidate that
//   place j-1 beats, found by one more `scan_row` pass over the row (L2 re-reads: no sort, no per-thread array, no limit
//   on cols) -- then k label entries at the ranked ids, and integer words like the above.
// gps_answer_fold   the integer pairs of BaseEvaluator.update, or the float64 bookkeeping of SQA3DEval.update / record.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gps_hip.h"

namespace gps_metrics {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxProblems = GPS_CLS_HITS_MAX_PROBLEMS;
constexpr int kWaveMaxCols = GPS_CLS_HITS_WAVE_MAX_COLS;
constexpr int kMaxTerms = GPS_METRICS_MAX_TERMS;

// Candidate of torch.argmax: NaN is the greatest value, the first index among equals wins; idx < 0 = no candidate.
// `beats` is a strict total order on (value class, value, index), so candidates may be folded in any order.
struct Best {
  float v;
  int idx;
  __device__ __forceinline__ bool beats(const Best &o) const {
    if (idx < 0) return false;
    if (o.idx < 0) return true;
    const bool n = v != v, on = o.v != o.v;
    if (n != on) return n;
    if (n || v == o.v) return idx < o.idx;
    return v > o.v;
  }
  // BELOW: only candidates that `prev` beats (the places after `prev` in the order); prev.idx < 0 = no bound.
  template <bool BELOW = false>
  __device__ __forceinline__ void take(float x, int i, const Best &prev = Best{0.f, -1}) {
    const Best c{x, i};
    if (BELOW && prev.idx >= 0 && !prev.beats(c)) return;
    if (c.beats(*this)) *this = c;
  }
};

__device__ __forceinline__ float bf16_to_f32(uint32_t h) { return __uint_as_float(h << 16); }

__device__ __forceinline__ Best wave_fold(Best b) {
  for (int off = 32; off >= 1; off >>= 1) {
    const Best o{__shfl_xor(b.v, off, 64), __shfl_xor(b.idx, off, 64)};
    if (o.beats(b)) b = o;
  }
  return b;
}

struct Launch {
  gps_cls_hits_problem p[kMaxProblems];
  int first_block[kMaxProblems];                // block offset of each problem; unused entries hold INT_MAX
};

__device__ __forceinline__ bool mask_at(const void *m, int elem_bytes, size_t row) {
  if (!m) return true;
  return elem_bytes == 8 ? ((const int64_t *)m)[row] != 0 : ((const uint8_t *)m)[row] != 0;
}

// Is `row` counted?  (live, selected, label not ignored) -- reads three words of the row, never its logits.
__device__ __forceinline__ bool counted(const gps_cls_hits_problem &p, int row, int64_t &label) {
  if (row >= p.rows) return false;
  if (p.rows_dev && row >= *p.rows_dev) return false;
  if (!mask_at(p.sel, p.mask_elem_bytes, (size_t)row)) return false;
  label = p.labels[row];
  return !(p.use_ignore && label == (int64_t)p.ignore_index);
}

__device__ __forceinline__ uint32_t row_bits(const gps_cls_hits_problem &p, int row, int64_t label, const Best &best) {
  const int pred = best.idx < 0 ? 0 : best.idx;
  const bool hit = (int64_t)pred == label;                  // a label outside [0, cols) never equals an index
  const bool a = p.split_a && mask_at(p.split_a, p.mask_elem_bytes, (size_t)row);
  const bool b = p.split_b && mask_at(p.split_b, p.mask_elem_bytes, (size_t)row);
  return (hit ? 1u : 0u) | 2u | (hit && a ? 4u : 0u) | (a ? 8u : 0u) | (hit && b ? 16u : 0u) | (b ? 32u : 0u);
}

template <bool BF16, bool BELOW>
__device__ __forceinline__ void take_granule(Best &best, const uint4 &g, int first, const Best &prev) {
  const uint32_t w[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (BF16) {
      best.take<BELOW>(__uint_as_float(w[k] << 16), first + 2 * k, prev);   // little endian: the low half is the first element
      best.take<BELOW>(__uint_as_float(w[k] & 0xFFFF0000u), first + 2 * k + 1, prev);
    } else {
      best.take<BELOW>(__uint_as_float(w[k]), first + k, prev);
    }
  }
}

// One row scanned by NT threads (a wave: NT = 64, a workgroup: NT = kBlock), `tid` in [0, NT): the per-wave candidates
// (valid in every lane of the wave).  Rows start at any element boundary:
//   head  = the elements before the first 16-byte boundary of the row (fewer than one granule, at most cols)
//   body  = n_vec granules of 16 bytes, all inside [head, cols)
//   tail  = what is left, fewer than one granule
// BELOW: the best candidate among those `prev` beats -- the next place of the ranking after `prev`.
template <bool BF16, int NT, bool BELOW = false>
__device__ __forceinline__ Best scan_row(const void *__restrict__ row_ptr, int cols, int tid,
                                         const Best &prev = Best{0.f, -1}) {
  constexpr int kElem = BF16 ? 2 : 4, kPer = 16 / kElem;
  const uintptr_t a0 = (uintptr_t)row_ptr;
  int head = (int)(((16u - (uint32_t)(a0 & 15u)) & 15u) / kElem);       // the row starts on an element boundary (host-checked)
  head = head < cols ? head : cols;
  const int n_vec = (cols - head) / kPer;
  const int tail_first = head + n_vec * kPer;
  const uint4 *__restrict__ body = reinterpret_cast<const uint4 *>(a0 + (uintptr_t)head * kElem);
  Best best{0.f, -1};
  int g = tid;
  for (; g + 3 * NT < n_vec; g += 4 * NT) {                            // four independent 16-byte loads in flight
    const uint4 r0 = body[g], r1 = body[g + NT], r2 = body[g + 2 * NT], r3 = body[g + 3 * NT];
    take_granule<BF16, BELOW>(best, r0, head + g * kPer, prev);
    take_granule<BF16, BELOW>(best, r1, head + (g + NT) * kPer, prev);
    take_granule<BF16, BELOW>(best, r2, head + (g + 2 * NT) * kPer, prev);
    take_granule<BF16, BELOW>(best, r3, head + (g + 3 * NT) * kPer, prev);
  }
  for (; g < n_vec; g += NT) {
    const uint4 r = body[g];
    take_granule<BF16, BELOW>(best, r, head + g * kPer, prev);
  }
  // scalar head and tail, each shorter than one granule (8 elements at most): threads [0, head) and [8, 8 + tail)
  int e = -1;
  if (tid < head) e = tid;
  else if (tid >= 8 && tid - 8 < cols - tail_first) e = tail_first + (tid - 8);
  if (e >= 0) {
    if (BF16) best.take<BELOW>(bf16_to_f32(((const uint16_t *)row_ptr)[e]), e, prev);
    else best.take<BELOW>(((const float *)row_ptr)[e], e, prev);
  }
  return wave_fold(best);
}

__global__ __launch_bounds__(kBlock) void cls_hits_kernel(const Launch L) {
  __shared__ float s_v[kWaves];
  __shared__ int s_i[kWaves];
  __shared__ uint32_t s_bits[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // wave-uniform search: the last problem whose first block is not past this one
  int k = 0;
#pragma unroll
  for (int j = 1; j < kMaxProblems; ++j) k = (int)blockIdx.x >= L.first_block[j] ? j : k;
  const gps_cls_hits_problem &p = L.p[k];
  const int local = (int)blockIdx.x - L.first_block[k];
  unsigned long long *counters = reinterpret_cast<unsigned long long *>(p.counters);
  const size_t elem = p.logits_bf16 ? 2 : 4;
  if (p.cols > kWaveMaxCols) {
    const int row = local;
    int64_t label = 0;
    if (!counted(p, row, label)) return;                               // the same answer in every thread of the workgroup
    const void *x = (const char *)p.logits + (size_t)row * (size_t)p.ld * elem;
    const Best b = p.logits_bf16 ? scan_row<true, kBlock>(x, p.cols, tid) : scan_row<false, kBlock>(x, p.cols, tid);
    if (lane == 0) { s_v[wave] = b.v; s_i[wave] = b.idx; }
    __syncthreads();
    if (tid == 0) {
      Best best{s_v[0], s_i[0]};
#pragma unroll
      for (int w = 1; w < kWaves; ++w) {
        const Best o{s_v[w], s_i[w]};
        if (o.beats(best)) best = o;
      }
      s_bits[0] = row_bits(p, row, label, best);
    }
    __syncthreads();
    if (tid < 6 && ((s_bits[0] >> tid) & 1u)) atomicAdd(counters + tid, 1ull);
    return;
  }
  const int row = local * kWaves + wave;
  int64_t label = 0;
  uint32_t bits = 0;
  if (counted(p, row, label)) {                                        // wave-uniform
    const void *x = (const char *)p.logits + (size_t)row * (size_t)p.ld * elem;
    const Best b = p.logits_bf16 ? scan_row<true, 64>(x, p.cols, lane) : scan_row<false, 64>(x, p.cols, lane);
    bits = row_bits(p, row, label, b);
  }
  if (lane == 0) s_bits[wave] = bits;
  __syncthreads();
  if (tid < 6) {                                                       // counter `tid` of this workgroup's rows
    unsigned long long n = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) n += (s_bits[w] >> tid) & 1u;
    if (n) atomicAdd(counters + tid, n);
  }
}

struct FoldArgs {
  gps_metric_term t[kMaxTerms];
};

__global__ __launch_bounds__(64) void metrics_fold_kernel(const FoldArgs A, int n_terms, double weight, int n_mean,
                                                          double *__restrict__ last, double *__restrict__ acc,
                                                          double *__restrict__ total) {
  __shared__ double s_ratio[kMaxTerms];
  const int k = threadIdx.x;
  const bool mine = k < n_terms;
  if (mine) {
    const gps_metric_term &t = A.t[k];
    int64_t hits = *t.hits, count = t.count ? *t.count : 0;
    if (t.sub_hits) hits -= *t.sub_hits;
    if (t.sub_count) count -= *t.sub_count;
    const double den = t.use_const_denominator ? t.const_denominator : (double)count + t.eps;
    const double r = (double)hits / den;
    s_ratio[k] = r;
    last[k] = r;
    acc[k] = acc[k] + r * weight;
  }
  __syncthreads();                                                     // every term has read its words: they may be cleared
  if (mine) {
    const gps_metric_term &t = A.t[k];
    *t.hits = 0;
    if (t.count) *t.count = 0;
    if (t.sub_hits) *t.sub_hits = 0;
    if (t.sub_count) *t.sub_count = 0;
  }
  if (k == 0) {
    if (n_mean > 0) {
      double s = 0.0;
      for (int j = 0; j < n_mean; ++j) s = s + s_ratio[j];             // sum(all_acc): left to right from 0
      const double m = s / (double)n_mean;
      last[n_terms] = m;
      acc[n_terms] = acc[n_terms] + m * weight;
    }
    total[0] = total[0] + weight;
  }
}

// ---- gps_answer_hits: the k best answers of a row in rank order, and the hits among them ---------------------------------
constexpr int kMaxK = GPS_ANSWER_MAX_K;
constexpr int kMaxTypes = GPS_ANSWER_MAX_TYPES;
constexpr int kAnswerWords = GPS_ANSWER_WORDS;
constexpr int kAnswerWaveMaxCols = GPS_ANSWER_WAVE_MAX_COLS;
constexpr int kFoldMaxCls = GPS_ANSWER_FOLD_MAX_CLS;
static_assert(kAnswerWords == 3 + 2 * kMaxTypes, "hit1, hitk, count, type_hit1[], type_count[]");

__device__ __forceinline__ bool label_is_one(const void *label, int kind, size_t at) {
  if (kind == 0) return ((const int64_t *)label)[at] == 1;
  if (kind == 1) return ((const uint8_t *)label)[at] == 1;
  return ((const float *)label)[at] == 1.0f;
}

// The place after `prev` (prev.idx < 0: place 0) of the row at `x`, the same in every one of the NT threads that scan it;
// idx < 0 when `prev` was the last place.  NT = kBlock folds the per-wave candidates through s_v / s_i (one barrier; the
// caller alternates between two such buffers, so the next place may be written while a slow wave still reads this one).
template <int NT>
__device__ __forceinline__ Best next_place(const gps_answer_hits_args &a, const void *x, int t, const Best &prev,
                                           float *s_v, int *s_i) {
  Best b = a.scores_bf16 ? scan_row<true, NT, true>(x, a.cols, t, prev) : scan_row<false, NT, true>(x, a.cols, t, prev);
  if (NT == kBlock) {
    if ((t & 63) == 0) { s_v[t >> 6] = b.v; s_i[t >> 6] = b.idx; }
    __syncthreads();
    b = Best{s_v[0], s_i[0]};
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
      const Best o{s_v[w], s_i[w]};
      if (o.beats(b)) b = o;
    }
  }
  return b;
}

__global__ __launch_bounds__(kBlock) void answer_hits_kernel(const gps_answer_hits_args a) {
  __shared__ float s_v[2][kWaves];
  __shared__ int s_i[2][kWaves];
  __shared__ int s_ids[kWaves][kMaxK];
  __shared__ uint32_t s_row[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool wide = a.cols > kAnswerWaveMaxCols;
  const int row = wide ? (int)blockIdx.x : (int)blockIdx.x * kWaves + wave;
  const int slot = wide ? 0 : wave;                                    // the row's line of s_ids
  const int t = wide ? tid : lane;                                     // this thread among the row's
  // wave-uniform; the same in the whole workgroup of a wide row
  const bool live = row < a.rows && (!a.rows_dev || row < *a.rows_dev);
  if (live) {
    const void *x = (const char *)a.scores + (size_t)row * (size_t)a.ld * (a.scores_bf16 ? 2 : 4);
    Best prev{0.f, -1};
    for (int j = 0; j < a.k; ++j) {
      const Best b = wide ? next_place<kBlock>(a, x, t, prev, s_v[j & 1], s_i[j & 1])
                          : next_place<64>(a, x, t, prev, nullptr, nullptr);
      if (t == 0) s_ids[slot][j] = b.idx;
      if (b.idx >= 0) prev = b;                                        // past the last place every further one is empty too
    }
  }
  __syncthreads();
  // the row's first k threads: one label entry each, at the ranked id
  const bool mine = live && t < a.k;
  bool one = false;
  if (mine) {
    const int id = s_ids[slot][t];
    one = id >= 0 && label_is_one(a.label, a.label_kind, (size_t)row * (size_t)a.ld_label + (size_t)id);
    if (a.topk) a.topk[(size_t)row * a.k + t] = id;
  }
  const unsigned long long ones = __ballot(one);                       // k <= 16: the places sit in the wave's first lanes
  if (lane == 0) {
    uint32_t bits = 0;
    if (live && (!wide || wave == 0)) {
      bits = ((ones & 1ull) ? 1u : 0u) | (ones ? 2u : 0u) | 4u;
      if (a.type) {
        const int64_t ty = a.type[row];
        if (ty >= 0 && ty < (int64_t)a.n_types) bits |= 8u | ((uint32_t)ty << 4);
      }
    }
    s_row[wave] = bits;
  }
  __syncthreads();
  if (tid < kAnswerWords) {                                            // word `tid` of this workgroup's rows
    unsigned long long n = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const uint32_t bits = s_row[w];
      const bool typed = (bits & 8u) != 0;
      const int ty = (int)(bits >> 4);
      bool add;
      if (tid < 3) add = ((bits >> tid) & 1u) != 0;
      else if (tid < 3 + kMaxTypes) add = typed && ty == tid - 3 && (bits & 1u);
      else add = typed && ty == tid - 3 - kMaxTypes;
      n += add ? 1u : 0u;
    }
    if (n) atomicAdd(reinterpret_cast<unsigned long long *>(a.words) + tid, n);
  }
}

// One workgroup of 64 threads.  Every thread reads its words, computes, and only behind the barrier are the words cleared.
__global__ __launch_bounds__(64) void answer_fold_kernel(int64_t *__restrict__ words, int64_t *__restrict__ cls_words, int n_cls,
                                                         int n_types, double weight, int64_t *__restrict__ sums,
                                                         double *__restrict__ last, double *__restrict__ acc,
                                                         double *__restrict__ type_total, double *__restrict__ total) {
  const int k = threadIdx.x;
  if (sums) {                                                          // integer pairs: BaseEvaluator.update / record
    if (k < 2 + n_cls) {
      const int64_t h = k < 2 ? words[k] : cls_words[(k - 2) * 6], c = k < 2 ? words[2] : cls_words[(k - 2) * 6 + 1];
      sums[2 * k] += h;
      sums[2 * k + 1] += c;
      last[k] = (double)h / (double)(c > 1 ? c : 1);
    }
  } else if (k < 3) {                                                  // SQA3DEval: ans1 (and target_metric), ansk, obj_cls_raw
    double r;
    if (k < 2) {
      r = (double)words[k] / weight;
    } else {
      const int64_t h = n_cls ? cls_words[0] : 0, c = n_cls ? cls_words[1] : 0;
      r = c ? (double)h / (double)c : 0.0;
    }
    const int at = k == 2 ? 1 : 2 + k;
    last[at] = r;
    acc[at] = acc[at] + r * weight;
    if (k == 0) {
      last[0] = r;
      acc[0] = acc[0] + r * weight;
      total[0] = total[0] + weight;
    }
  } else if (k >= 4 && k < 4 + n_types) {
    const int ty = k - 4;
    const int64_t n = words[3 + kMaxTypes + ty];
    double ct = 1e-10;
    for (int64_t i = 0; i < n; ++i) ct = ct + 1.0;                    // count_type[t] += 1 per question
    const double r = (double)words[3 + ty] / ct;
    last[4 + ty] = r;
    last[4 + n_types + ty] = ct;
    acc[4 + ty] = acc[4 + ty] + r * ct;
    type_total[ty] = type_total[ty] + ct;
  }
  __syncthreads();
  if (k < kAnswerWords) words[k] = 0;
  if (k < n_cls * 6) cls_words[k] = 0;
}

inline int status() { return hipGetLastError() == hipSuccess ? GPS_OK : GPS_ERR_LAUNCH; }

}  // namespace gps_metrics

extern "C" int gps_cls_hits(const gps_cls_hits_problem *problems, int n_problems, gps_stream_t stream) {
  using namespace gps_metrics;
  if (n_problems < 0) return GPS_ERR_INVALID_ARGUMENT;
  if (n_problems > kMaxProblems) return GPS_ERR_UNSUPPORTED;
  if (n_problems == 0) return GPS_OK;
  if (!problems) return GPS_ERR_INVALID_ARGUMENT;
  Launch L;
  long long blocks = 0;
  int n = 0;
  for (int i = 0; i < n_problems; ++i) {
    const gps_cls_hits_problem &p = problems[i];
    if (p.rows < 0 || p.cols <= 0 || p.ld < p.cols) return GPS_ERR_INVALID_ARGUMENT;
    if (p.mask_elem_bytes != 1 && p.mask_elem_bytes != 8) return GPS_ERR_INVALID_ARGUMENT;
    if (p.rows == 0) continue;
    if (!p.logits || !p.labels || !p.counters) return GPS_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)p.logits & (p.logits_bf16 ? 1u : 3u)) != 0) return GPS_ERR_INVALID_ARGUMENT;   // element-aligned rows
    L.p[n] = p;
    L.first_block[n] = (int)blocks;
    blocks += p.cols > kWaveMaxCols ? (long long)p.rows : ((long long)p.rows + kWaves - 1) / kWaves;
    if (blocks > 0x7FFFFFFFll) return GPS_ERR_UNSUPPORTED;
    ++n;
  }
  if (n == 0) return GPS_OK;
  for (int i = n; i < kMaxProblems; ++i) {
    L.p[i] = L.p[0];
    L.first_block[i] = 0x7FFFFFFF;
  }
  hipLaunchKernelGGL(cls_hits_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, L);
  return status();
}

extern "C" int gps_metrics_fold(int n_terms, const gps_metric_term *terms, double weight, int n_mean, double *last,
                                double *acc, double *total, gps_stream_t stream) {
  using namespace gps_metrics;
  if (n_terms < 0 || n_mean < 0 || n_mean > n_terms) return GPS_ERR_INVALID_ARGUMENT;
  if (n_terms > kMaxTerms) return GPS_ERR_UNSUPPORTED;
  if (!last || !acc || !total) return GPS_ERR_INVALID_ARGUMENT;
  if (n_terms > 0 && !terms) return GPS_ERR_INVALID_ARGUMENT;
  FoldArgs A;
  for (int i = 0; i < kMaxTerms; ++i) {
    if (i < n_terms) {
      if (!terms[i].hits || (!terms[i].count && !terms[i].use_const_denominator)) return GPS_ERR_INVALID_ARGUMENT;
      A.t[i] = terms[i];
    } else {
      A.t[i] = gps_metric_term{};
    }
  }
  hipLaunchKernelGGL(metrics_fold_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, A, n_terms, weight, n_mean, last, acc,
                     total);
  return status();
}

extern "C" int gps_answer_hits(const gps_answer_hits_args *args, gps_stream_t stream) {
  using namespace gps_metrics;
  if (!args) return GPS_ERR_INVALID_ARGUMENT;
  const gps_answer_hits_args &a = *args;
  if (a.rows < 0 || a.cols <= 0 || a.ld < a.cols || a.ld_label < a.cols) return GPS_ERR_INVALID_ARGUMENT;
  if (a.k < 1 || a.k > kMaxK || a.n_types < 0 || a.n_types > kMaxTypes) return GPS_ERR_INVALID_ARGUMENT;
  if (a.label_kind < 0 || a.label_kind > 2) return GPS_ERR_INVALID_ARGUMENT;
  if (!a.scores || !a.label || !a.words) return GPS_ERR_INVALID_ARGUMENT;
  if (((uintptr_t)a.scores & (a.scores_bf16 ? 1u : 3u)) != 0) return GPS_ERR_INVALID_ARGUMENT;      // element-aligned rows
  if (a.rows == 0) return GPS_OK;
  const unsigned blocks = a.cols > kAnswerWaveMaxCols ? (unsigned)a.rows : ((unsigned)a.rows + kWaves - 1) / kWaves;
  hipLaunchKernelGGL(answer_hits_kernel, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, a);
  return status();
}

extern "C" int gps_answer_fold(int64_t *words, int64_t *cls_words, int n_cls, int n_types, double weight, int64_t *sums,
                               double *last, double *acc, double *type_total, double *total, gps_stream_t stream) {
  using namespace gps_metrics;
  if (!words || !last) return GPS_ERR_INVALID_ARGUMENT;
  if (n_cls < 0 || n_cls > kFoldMaxCls || (n_cls > 0 && !cls_words)) return GPS_ERR_INVALID_ARGUMENT;
  if (!sums) {
    if (!acc || !type_total || !total || n_cls > 1) return GPS_ERR_INVALID_ARGUMENT;
    if (n_types < 0 || n_types > kMaxTypes || !(weight > 0.0)) return GPS_ERR_INVALID_ARGUMENT;
  }
  hipLaunchKernelGGL(answer_fold_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, words, cls_words, n_cls, n_types, weight,
                     sums, last, acc, type_total, total);
  return status();
}
