// gps_refer.hip -- the ScanRefer target path of the data loader and its evaluator on MI355X (gfx950).
//
// Reference (what these three entries replace):
//   convert_pc_to_box        data/data_utils.py:63-72      box of one object cloud (float64 rows -> float64 box)
//   ScanBase._getitem_refer  data/datasets/base.py:348-417 pc_type 'pred': proposal labels by first IoU >= 0.25 match,
//                                                          tgt_object_id_iou25 / _iou50 flags, tgt_object_id
//   box3d_iou                data/data_utils.py:212-234    via construct_bbox_corners :266-277, get_box3d_min_max :194-209
//   dataset wrapper padding  data/datasets/dataset_wrapper.py:164-191
//   ScanReferEval.batch_metrics  evaluator/scanrefer_eval.py:14-87
//
// gps_obj_boxes      min / max of x, y, z over every object's CSR segment, then centre and size in float64.
//   The segments are cut by the HOST into chunks of at most kChunk points (it knows the sizes): one workgroup per chunk,
//   so a 300 000-point floor is 74 workgroups and not one.  Every point is read once (one 16-byte load per point in the
//   record form, four in flight per lane); no LDS, no scratch.  A wave folds its 1024 points into six integers and adds
//   them to the object's six workspace words with vector atomic min / max on an ORDER-PRESERVING ENCODING of the
//   float32 bits:  key(u) = u ^ 0x80000000 for u >= 0 (sign bit clear), ~u otherwise.  Unsigned order of the keys is the
//   order of the floats, -inf and +inf included (-0 sorts below +0).  Integer min / max is associative and commutative,
//   so the result is bit-identical between runs and independent of the chunking.
//   NaN: a NaN coordinate is sent as key 0 to the minimum and as key 0xFFFFFFFF to the maximum -- the absorbing
//   elements of the two reductions.  Both decode to a NaN bit pattern, so centre and size of that coordinate come out
//   NaN like np.min / np.max give them.  The same two words are the identities of the opposite reduction (the minimum
//   starts at 0xFFFFFFFF, the maximum at 0): an object without points decodes to NaN as well.
//   The call itself sets the workspace to the identities (first launch) and decodes it (third launch).
//
// gps_refer_targets  one workgroup per batch item, one thread per object slot; float64, compiled -ffp-contract=off.
// gps_refer_metrics  one wave per batch item: arg-max with torch.argmax's rule, integer atomics into 8 counters.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gps_box_dev.h"
#include "gps_hip.h"

namespace gps_refer {

constexpr int kBlock = 256;
constexpr int kPerLane = 16;                    // points per lane and chunk
constexpr int kChunk = kBlock * kPerLane;       // GPS_OBJ_BOXES_CHUNK

static_assert(kChunk == GPS_OBJ_BOXES_CHUNK, "the host cuts the work list with the header's constant");

__device__ __forceinline__ uint32_t enc(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u ^ 0x80000000u);
}
__device__ __forceinline__ float dec(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

struct MinMax {
  uint32_t lo[3], hi[3];
  __device__ __forceinline__ void fold(float x, float y, float z) {
    const float v[3] = {x, y, z};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const bool nan = v[c] != v[c];
      const uint32_t k = enc(v[c]);
      lo[c] = min(lo[c], nan ? 0u : k);
      hi[c] = max(hi[c], nan ? 0xFFFFFFFFu : k);
    }
  }
};

__global__ __launch_bounds__(kBlock) void boxes_init_kernel(int n_words, uint32_t *__restrict__ ws) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n_words) ws[i] = (i % 6) < 3 ? 0xFFFFFFFFu : 0u;
}

// work (n_work, 3) int64: object, first point (global index), count <= kChunk.  An entry outside the arrays is skipped.
template <bool REC16>
__global__ __launch_bounds__(kBlock, 4) void boxes_chunk_kernel(int n_objects, long long n_points,
                                                                 const float *__restrict__ xyz,
                                                                 const int64_t *__restrict__ work,
                                                                 uint32_t *__restrict__ ws) {
  const int64_t *w = work + (size_t)blockIdx.x * 3;
  const int64_t obj = w[0], first = w[1], count = w[2];
  if (obj < 0 || obj >= n_objects || first < 0 || count <= 0 || count > kChunk || first + count > n_points) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t k = (uint32_t)count;
  MinMax m;
#pragma unroll
  for (int c = 0; c < 3; ++c) { m.lo[c] = 0xFFFFFFFFu; m.hi[c] = 0u; }
  // wave `wave` takes points [wave * 1024, wave * 1024 + 1024) of the chunk, lane-interleaved: 1 KiB per load instruction
  const uint32_t base = (uint32_t)wave * (64u * kPerLane) + (uint32_t)lane;
  if (REC16) {
    const float4 *p4 = reinterpret_cast<const float4 *>(xyz) + first;
#pragma unroll
    for (int t = 0; t < kPerLane; t += 4) {
      const uint32_t i0 = base + 64u * t, i1 = i0 + 64u, i2 = i0 + 128u, i3 = i0 + 192u;
      if (i3 < k) {                              // four independent 16-byte loads in flight
        const float4 r0 = p4[i0], r1 = p4[i1], r2 = p4[i2], r3 = p4[i3];
        m.fold(r0.x, r0.y, r0.z); m.fold(r1.x, r1.y, r1.z); m.fold(r2.x, r2.y, r2.z); m.fold(r3.x, r3.y, r3.z);
      } else {
        if (i0 < k) { const float4 r = p4[i0]; m.fold(r.x, r.y, r.z); }
        if (i1 < k) { const float4 r = p4[i1]; m.fold(r.x, r.y, r.z); }
        if (i2 < k) { const float4 r = p4[i2]; m.fold(r.x, r.y, r.z); }
      }
    }
  } else {
    const float *p = xyz + (size_t)first * 3;
#pragma unroll 4
    for (int t = 0; t < kPerLane; ++t) {
      const uint32_t i = base + 64u * t;
      if (i < k) m.fold(p[(size_t)i * 3], p[(size_t)i * 3 + 1], p[(size_t)i * 3 + 2]);
    }
  }
  if ((uint32_t)wave * (64u * kPerLane) >= k) return;              // wave-uniform: this wave had no point
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    for (int off = 32; off >= 1; off >>= 1) {
      m.lo[c] = min(m.lo[c], (uint32_t)__shfl_xor((int)m.lo[c], off, 64));
      m.hi[c] = max(m.hi[c], (uint32_t)__shfl_xor((int)m.hi[c], off, 64));
    }
  }
  if (lane < 6) {                                // one vector atomic instruction per kind and wave
    uint32_t *o = ws + (size_t)obj * 6 + lane;
    const uint32_t vlo = lane == 0 ? m.lo[0] : (lane == 1 ? m.lo[1] : m.lo[2]);
    const uint32_t vhi = lane == 3 ? m.hi[0] : (lane == 4 ? m.hi[1] : m.hi[2]);
    if (lane < 3) atomicMin(o, vlo); else atomicMax(o, vhi);
  }
}

__global__ __launch_bounds__(kBlock) void boxes_finish_kernel(int n_objects, const uint32_t *__restrict__ ws,
                                                               double *__restrict__ boxes) {
  const int i = blockIdx.x * kBlock + threadIdx.x;     // (object, coordinate)
  if (i >= n_objects * 3) return;
  const int obj = i / 3, c = i - obj * 3;
  const double lo = (double)dec(ws[(size_t)obj * 6 + c]), hi = (double)dec(ws[(size_t)obj * 6 + 3 + c]);
  boxes[(size_t)obj * 6 + c] = (lo + hi) / 2.0;        // convert_pc_to_box: (min + max) / 2, max - min
  boxes[(size_t)obj * 6 + 3 + c] = hi - lo;
}

// ---- targets ----------------------------------------------------------------------------------------------------------
using gps_box::Box;                             // the box and box3d_iou: csrc/gps_box_dev.h, shared with the
using gps_box::iou;                             // proposal selection (gps_obj_select_pred.hip)

constexpr int kMaxSlots = GPS_REFER_MAX_OBJ;    // 512: eight waves

__global__ __launch_bounds__(kMaxSlots) void refer_targets_kernel(
    int O, int n_objects, int mode, const double *__restrict__ boxes, const int32_t *__restrict__ labels,
    const int32_t *__restrict__ row_obj, const int32_t *__restrict__ tgt_obj, const int32_t *__restrict__ scan_range,
    int64_t *__restrict__ iou25, int64_t *__restrict__ iou50, int64_t *__restrict__ tgt_id,
    int64_t *__restrict__ obj_labels) {
  __shared__ int s_last[kMaxSlots / 64], s_real[kMaxSlots / 64];
  const int b = blockIdx.x, i = threadIdx.x, lane = i & 63, wave = i >> 6, n_waves = (int)blockDim.x >> 6;
  int g = i < O ? row_obj[(size_t)b * O + i] : -1;
  if (g >= n_objects) g = -1;                    // an id outside the packed arrays is a pad, never an address
  const bool real = g >= 0;
  const int tgt = tgt_obj[b];
  const bool tgt_ok = tgt >= 0 && tgt < n_objects;
  bool hit25 = false, hit50 = false;
  int label = -100;
  if (real) {
    label = labels[g];
    if (mode == 1) {                             // 'gt': one-hot at the referred object's slot
      hit25 = hit50 = tgt_ok && g == tgt;
    } else {
      Box p, q;
      p.load(boxes + (size_t)g * 6);
      if (tgt_ok) {
        q.load(boxes + (size_t)tgt * 6);
        const double v = iou(p, q);
        hit25 = v >= 0.25;
        hit50 = v >= 0.5;
      }
      // the label of the FIRST annotated object of the scan that overlaps by >= 0.25 (base.py:359-366)
      int first = scan_range[2 * b], last = scan_range[2 * b + 1];
      first = first < 0 ? 0 : first;
      last = last > n_objects ? n_objects : last;
      for (int j = first; j < last; ++j) {
        q.load(boxes + (size_t)j * 6);           // the same address in every lane: served from L2 / the scalar cache
        if (iou(q, p) >= 0.25) {
          label = labels[j];
          break;
        }
      }
    }
  }
  const unsigned long long m25 = __ballot(hit25), mreal = __ballot(real);
  if (lane == 0) {
    s_last[wave] = m25 ? wave * 64 + (63 - __clzll((long long)m25)) : -1;
    s_real[wave] = __popcll(mreal);
  }
  __syncthreads();
  if (i < O) {
    iou25[(size_t)b * O + i] = hit25 ? 1 : 0;
    iou50[(size_t)b * O + i] = hit50 ? 1 : 0;
    obj_labels[(size_t)b * O + i] = real ? (int64_t)label : (int64_t)-100;
  }
  if (i == 0) {
    int last = -1, n_b = 0;
    for (int w = 0; w < n_waves; ++w) {
      last = s_last[w] > last ? s_last[w] : last;
      n_b += s_real[w];
    }
    tgt_id[b] = last >= 0 ? last : n_b;          // the LAST hit wins; none: len(obj_pcds) (base.py:410, :453-454)
  }
}

// ---- metrics ----------------------------------------------------------------------------------------------------------
// Candidate of torch.argmax: NaN is the greatest value, the first index among equals wins; idx < 0 = no candidate.
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
};

constexpr int kRowsPerBlock = kBlock / 64;

template <bool BF16>
__global__ __launch_bounds__(kBlock) void refer_metrics_kernel(
    int B, int O, const void *__restrict__ logits, long long ld, const int64_t *__restrict__ iou25,
    const int64_t *__restrict__ iou50, const int64_t *__restrict__ tgt_id, const uint8_t *__restrict__ is_multiple,
    unsigned long long *__restrict__ counters) {
  __shared__ uint32_t s_bits[kRowsPerBlock];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * kRowsPerBlock + wave;
  uint32_t bits = 0;
  if (row < B) {
    Best best{0.f, -1};
    for (int i = lane; i < O; i += 64) {
      float v;
      if (BF16) v = __uint_as_float((uint32_t)((const uint16_t *)logits)[(size_t)row * ld + i] << 16);
      else v = ((const float *)logits)[(size_t)row * ld + i];
      const Best c{v, i};
      if (c.beats(best)) best = c;
    }
    for (int off = 32; off >= 1; off >>= 1) {
      const Best o{__shfl_xor(best.v, off, 64), __shfl_xor(best.idx, off, 64)};
      if (o.beats(best)) best = o;
    }
    if (lane == 0) {
      const int pred = best.idx < 0 ? 0 : best.idx;
      const bool h25 = iou25[(size_t)row * O + pred] != 0, h50 = iou50[(size_t)row * O + pred] != 0;
      const bool mult = is_multiple[row] != 0;
      bits = 1u | (mult ? 2u : 0u) | (h25 ? 4u : 0u) | (h50 ? 8u : 0u) | (h25 && mult ? 16u : 0u) |
             (h50 && mult ? 32u : 0u) | ((int64_t)pred == tgt_id[row] ? 64u : 0u);
    }
  }
  if (lane == 0) s_bits[wave] = bits;
  __syncthreads();
  if (threadIdx.x < 7) {                         // counter c of this block's rows: one vector atomic instruction
    unsigned long long n = 0;
#pragma unroll
    for (int w = 0; w < kRowsPerBlock; ++w) n += (s_bits[w] >> threadIdx.x) & 1u;
    if (n) atomicAdd(counters + threadIdx.x, n);
  }
}

inline int status() { return hipGetLastError() == hipSuccess ? GPS_OK : GPS_ERR_LAUNCH; }

}  // namespace gps_refer

extern "C" int gps_obj_boxes(int n_objects, long long n_points, int n_work, const float *xyz, int records,
                             const int64_t *work, uint32_t *workspace, double *boxes, gps_stream_t stream) {
  using namespace gps_refer;
  if (n_objects < 0 || n_points < 0 || n_work < 0) return GPS_ERR_INVALID_ARGUMENT;
  if (n_objects == 0) return GPS_OK;
  if (n_objects > (1 << 28)) return GPS_ERR_UNSUPPORTED;           // 6 * n_objects words are indexed with int
  if (!workspace || !boxes) return GPS_ERR_INVALID_ARGUMENT;
  if (n_work > 0 && (!xyz || !work)) return GPS_ERR_INVALID_ARGUMENT;
  if (records && ((uintptr_t)xyz & 15u) != 0) return GPS_ERR_INVALID_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  const int n_words = n_objects * 6;
  hipLaunchKernelGGL(boxes_init_kernel, dim3((n_words + kBlock - 1) / kBlock), dim3(kBlock), 0, s, n_words, workspace);
  if (n_work > 0) {
    if (records)
      hipLaunchKernelGGL(boxes_chunk_kernel<true>, dim3(n_work), dim3(kBlock), 0, s, n_objects, n_points, xyz, work,
                         workspace);
    else
      hipLaunchKernelGGL(boxes_chunk_kernel<false>, dim3(n_work), dim3(kBlock), 0, s, n_objects, n_points, xyz, work,
                         workspace);
  }
  hipLaunchKernelGGL(boxes_finish_kernel, dim3((n_objects * 3 + kBlock - 1) / kBlock), dim3(kBlock), 0, s, n_objects,
                     workspace, boxes);
  return status();
}

extern "C" int gps_refer_targets(int B, int O, int n_objects, int mode, const double *boxes, const int32_t *labels,
                                 const int32_t *row_obj, const int32_t *tgt_obj, const int32_t *scan_range,
                                 int64_t *iou25, int64_t *iou50, int64_t *tgt_id, int64_t *obj_labels,
                                 gps_stream_t stream) {
  using namespace gps_refer;
  if (B < 0 || O <= 0 || n_objects < 0 || (mode != 0 && mode != 1)) return GPS_ERR_INVALID_ARGUMENT;
  if (O > kMaxSlots) return GPS_ERR_UNSUPPORTED;
  if (B == 0) return GPS_OK;
  if (!row_obj || !tgt_obj || !scan_range || !iou25 || !iou50 || !tgt_id || !obj_labels) return GPS_ERR_INVALID_ARGUMENT;
  if (n_objects > 0 && (!boxes || !labels)) return GPS_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(refer_targets_kernel, dim3(B), dim3((O + 63) / 64 * 64), 0, (hipStream_t)stream, O, n_objects,
                     mode, boxes, labels, row_obj, tgt_obj, scan_range, iou25, iou50, tgt_id, obj_labels);
  return status();
}

extern "C" int gps_refer_metrics(int B, int O, const void *og3d_logits, long long ld, int logits_bf16,
                                 const int64_t *iou25, const int64_t *iou50, const int64_t *tgt_id,
                                 const uint8_t *is_multiple, int64_t *counters, gps_stream_t stream) {
  using namespace gps_refer;
  if (B < 0 || O <= 0 || ld < O) return GPS_ERR_INVALID_ARGUMENT;
  if (B == 0) return GPS_OK;
  if (!og3d_logits || !iou25 || !iou50 || !tgt_id || !is_multiple || !counters) return GPS_ERR_INVALID_ARGUMENT;
  const dim3 grid((B + kRowsPerBlock - 1) / kRowsPerBlock);
  auto *c = reinterpret_cast<unsigned long long *>(counters);
  if (logits_bf16)
    hipLaunchKernelGGL(refer_metrics_kernel<true>, grid, dim3(kBlock), 0, (hipStream_t)stream, B, O, og3d_logits, ld,
                       iou25, iou50, tgt_id, is_multiple, c);
  else
    hipLaunchKernelGGL(refer_metrics_kernel<false>, grid, dim3(kBlock), 0, (hipStream_t)stream, B, O, og3d_logits, ld,
                       iou25, iou50, tgt_id, is_multiple, c);
  return status();
}
