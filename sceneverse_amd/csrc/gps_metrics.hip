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
  __device__ __forceinline__ void take(float x, int i) {
    const Best c{x, i};
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

template <bool BF16>
__device__ __forceinline__ void take_granule(Best &best, const uint4 &g, int first) {
  const uint32_t w[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (BF16) {
      best.take(__uint_as_float(w[k] << 16), first + 2 * k);            // little endian: the low half is the first element
      best.take(__uint_as_float(w[k] & 0xFFFF0000u), first + 2 * k + 1);
    } else {
      best.take(__uint_as_float(w[k]), first + k);
    }
  }
}

// One row scanned by NT threads (a wave: NT = 64, a workgroup: NT = kBlock), `tid` in [0, NT): the per-wave candidates
// (valid in every lane of the wave).  Rows start at any element boundary:
//   head  = the elements before the first 16-byte boundary of the row (fewer than one granule, at most cols)
//   body  = n_vec granules of 16 bytes, all inside [head, cols)
//   tail  = what is left, fewer than one granule
template <bool BF16, int NT>
__device__ __forceinline__ Best scan_row(const void *__restrict__ row_ptr, int cols, int tid) {
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
    take_granule<BF16>(best, r0, head + g * kPer);
    take_granule<BF16>(best, r1, head + (g + NT) * kPer);
    take_granule<BF16>(best, r2, head + (g + 2 * NT) * kPer);
    take_granule<BF16>(best, r3, head + (g + 3 * NT) * kPer);
  }
  for (; g < n_vec; g += NT) {
    const uint4 r = body[g];
    take_granule<BF16>(best, r, head + g * kPer);
  }
  // scalar head and tail, each shorter than one granule (8 elements at most): threads [0, head) and [8, 8 + tail)
  int e = -1;
  if (tid < head) e = tid;
  else if (tid >= 8 && tid - 8 < cols - tail_first) e = tail_first + (tid - 8);
  if (e >= 0) {
    if (BF16) best.take(bf16_to_f32(((const uint16_t *)row_ptr)[e]), e);
    else best.take(((const float *)row_ptr)[e], e);
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
