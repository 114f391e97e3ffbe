// gps_objects.hip -- per-object input processing of the GPS data loader on MI355X (gfx950).
//
// Reference: ScanBase._obj_processing_post, data/datasets/base.py:697-740 (rotate, centre/size ->
// obj_locs, box, subsample num_points, centre, scale to the unit ball), the loader's colour scaling
// base.py:74-76 and the padding to max_obj_len + obj_masks of data/datasets/dataset_wrapper.py:62-70.
// The reference does this per object in numpy on the data-loader workers and ships the result
// (126 MB/step/GPU at B=64) over PCIe; here the scenes stay resident in HBM in their RAW form
// (xyz f32 + rgb u8, as 16-byte records or as two arrays; objects contiguous, CSR offsets) and ONE launch produces the
// batch-ready (rows, num_points, 6) f32 tensor + obj_locs + obj_boxes + obj_masks.
//
// One workgroup (256 threads) per output row (= object slot of a scene, or a padding slot).
//   pass 1  all k points of the object: rotate, sum / min / max  -> centre, size, box
//   pass 2  the num_points sampled points (indices given, or drawn on the device) kept in VGPRs:
//           mean -> max norm -> (x - mean) / max_dist, colours, written as f32
// HBM-bound byte work: k*16 B streamed once (the gathers of pass 2 then hit lines the stream left in
// L2) + num_points*24 B written.
// Arithmetic is float64 like the reference (numpy promotes [xyz f32 | rgb u8 / 127.5 - 1] to f64)
// and rounded to f32 at the end like the loader's `.float()`; only the summation ORDER of the two
// means differs from numpy's pairwise sum (<= 1 f32 ulp after rounding, tests/test_gpu_objects.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gps_hip.h"

namespace gps_obj {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxPer = 8;                      // sampled points per thread: num_points <= 2048

__device__ __forceinline__ uint64_t mix64(uint64_t z) {          // splitmix64 finaliser
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// The seed of a launch: `seed` plus the optional device word, read here so that a captured launch redraws when the word
// is advanced between replays (effective_seed of gps_dropout.h: unsigned wrap).
__device__ __forceinline__ uint64_t row_seed(uint64_t seed, const uint64_t *seed_dev) {
  return seed + (seed_dev ? *seed_dev : 0ull);
}

// Device sampler.  k < num_points: WITH replacement (np.random.choice(..., replace=True) semantics):
// an independent uniform index per draw.  k >= num_points: WITHOUT replacement: the first num_points
// images of a keyed pseudo-random PERMUTATION of [0, k) -- a 4-round Feistel network on the smallest
// even-width domain 2^(2h) >= k, cycle-walked back into [0, k) (a permutation of the domain restricted
// to a subset by cycle-walking is a permutation of the subset), so indices are distinct by construction.
__device__ __forceinline__ uint32_t sample_index(uint64_t key, uint32_t j, uint32_t k, bool replace) {
  if (replace) return (uint32_t)(((mix64(key ^ ((uint64_t)j << 1 | 1)) >> 32) * (uint64_t)k) >> 32);
  int bits = 32 - __clz((int)(k - 1) | 1);                       // bits needed for k-1 (>= 1)
  const int h = (bits + 1) >> 1;
  const uint32_t mask = (1u << h) - 1u;
  uint32_t x = j;
  do {
    uint32_t l = x >> h, r = x & mask;
#pragma unroll
    for (int round = 0; round < 4; ++round) {
      const uint32_t f = (uint32_t)mix64(key + 0xD1B54A32D192ED03ull * (uint64_t)(round + 1) + r) & mask;
      const uint32_t nl = r;
      r = l ^ f;
      l = nl;
    }
    x = (l << h) | r;
  } while (x >= k);
  return x;
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ double wave_min(double v) {
  for (int off = 32; off >= 1; off >>= 1) v = fmin(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
  for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}

struct Rot {
  double m[9];
  bool on;
  __device__ __forceinline__ void apply(double &x, double &y, double &z) const {
    if (!on) return;
    // obj_pcd[:, :3] @ rot.T  (base.py:708): out_j = sum_c p_c * R[j][c]
    const double a = (x * m[0] + y * m[1]) + z * m[2];
    const double b = (x * m[3] + y * m[4]) + z * m[5];
    const double c = (x * m[6] + y * m[7]) + z * m[8];
    x = a; y = b; z = c;
  }
};

// REC16: `xyz` is an array of 16-byte records {f32 x, y, z; u8 r, g, b, pad} (one aligned 16-B load per
// point in the stream, and the sampled points -- colours included -- are gathered from lines the stream
// just pulled through L2); otherwise xyz (N,3) and the colours are separate arrays.
template <bool REC16>
__global__ __launch_bounds__(kBlock) void obj_processing_post_kernel(
    int n_points, const float *__restrict__ xyz, const uint8_t *__restrict__ rgb_u8,
    const float *__restrict__ rgb_f32, const int64_t *__restrict__ obj_offsets,
    const int32_t *__restrict__ row_obj, const int32_t *__restrict__ sample_idx, uint64_t seed,
    const uint64_t *__restrict__ seed_dev, const float *__restrict__ rot, const int32_t *__restrict__ row_rot,
    float *__restrict__ obj_fts,
    float *__restrict__ obj_locs, float *__restrict__ obj_boxes, uint8_t *__restrict__ obj_masks) {
  __shared__ double s_red[kWaves][9];
  __shared__ double s_out[9];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int obj = row_obj[row];
  float *fts = obj_fts + (size_t)row * n_points * 6;
  int64_t begin = 0, k64 = 0;
  if (obj >= 0) {
    begin = obj_offsets[obj];
    k64 = obj_offsets[obj + 1] - begin;
  }
  if (obj < 0 || k64 <= 0) {                    // padding slot: features 1.0, locations 0.0, mask off
    for (int i = tid; i < n_points * 6; i += kBlock) fts[i] = 1.0f;
    if (tid < 6) {
      obj_locs[(size_t)row * 6 + tid] = 0.0f;
      if (obj_boxes) obj_boxes[(size_t)row * 6 + tid] = 0.0f;
    }
    if (tid == 0 && obj_masks) obj_masks[row] = 0;
    return;
  }
  const uint32_t k = (uint32_t)k64;
  Rot R;
  R.on = rot != nullptr && row_rot != nullptr && row_rot[row] >= 0;
  if (R.on) {
    const float *r = rot + (size_t)row_rot[row] * 9;
#pragma unroll
    for (int i = 0; i < 9; ++i) R.m[i] = (double)r[i];
  }
  const float *p = xyz + (size_t)begin * (REC16 ? 4 : 3);
  const float4 *p4 = reinterpret_cast<const float4 *>(xyz) + begin;

  // ---- pass 1: centre / size / box over ALL points of the (rotated) object --------------------
  double sx = 0, sy = 0, sz = 0;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  auto fold = [&](double x, double y, double z) {
    R.apply(x, y, z);
    sx += x; sy += y; sz += z;
    lo[0] = fmin(lo[0], x); lo[1] = fmin(lo[1], y); lo[2] = fmin(lo[2], z);
    hi[0] = fmax(hi[0], x); hi[1] = fmax(hi[1], y); hi[2] = fmax(hi[2], z);
  };
  uint32_t i = tid;
  if (REC16) {
    // four independent 16-byte loads in flight per thread: a 20 000-point object is 20 trips, not 79
    for (; i + 3u * kBlock < k; i += 4u * kBlock) {
      const float4 r0 = p4[i], r1 = p4[i + kBlock], r2 = p4[i + 2u * kBlock], r3 = p4[i + 3u * kBlock];
      fold(r0.x, r0.y, r0.z); fold(r1.x, r1.y, r1.z); fold(r2.x, r2.y, r2.z); fold(r3.x, r3.y, r3.z);
    }
    for (; i < k; i += kBlock) {
      const float4 r = p4[i];
      fold(r.x, r.y, r.z);
    }
  } else {
    for (; i < k; i += kBlock) fold(p[(size_t)i * 3], p[(size_t)i * 3 + 1], p[(size_t)i * 3 + 2]);
  }
  sx = wave_sum(sx); sy = wave_sum(sy); sz = wave_sum(sz);
#pragma unroll
  for (int c = 0; c < 3; ++c) { lo[c] = wave_min(lo[c]); hi[c] = wave_max(hi[c]); }
  if (lane == 0) {
    s_red[wave][0] = sx; s_red[wave][1] = sy; s_red[wave][2] = sz;
#pragma unroll
    for (int c = 0; c < 3; ++c) { s_red[wave][3 + c] = lo[c]; s_red[wave][6 + c] = hi[c]; }
  }
  __syncthreads();
  if (tid < 9) {
    double v = s_red[0][tid];
    for (int w = 1; w < kWaves; ++w)
      v = tid < 3 ? v + s_red[w][tid] : (tid < 6 ? fmin(v, s_red[w][tid]) : fmax(v, s_red[w][tid]));
    s_out[tid] = v;
  }
  __syncthreads();
  if (tid < 3) {
    const double mn = s_out[3 + tid], mx = s_out[6 + tid];
    obj_locs[(size_t)row * 6 + tid] = (float)(s_out[tid] / (double)k);
    obj_locs[(size_t)row * 6 + 3 + tid] = (float)(mx - mn);
    if (obj_boxes) {
      obj_boxes[(size_t)row * 6 + tid] = (float)((mx + mn) / 2.0);
      obj_boxes[(size_t)row * 6 + 3 + tid] = (float)(mx - mn);
    }
  }
  if (tid == 0 && obj_masks) obj_masks[row] = 1;
  __syncthreads();                               // s_red / s_out are reused below

  // ---- pass 2: the sampled points, held in registers -----------------------------------------
  const bool replace = k < (uint32_t)n_points;
  const uint64_t key = mix64(row_seed(seed, seed_dev) ^ mix64((uint64_t)row));   // per output row: a scene drawn twice differs
  double px[kMaxPer], py[kMaxPer], pz[kMaxPer];
  uint32_t src[kMaxPer];                         // sampled index, or (REC16) the record's colour word
  sx = sy = sz = 0;
#pragma unroll
  for (int i = 0; i < kMaxPer; ++i) {
    const int j = tid + i * kBlock;
    if (j < n_points) {
      uint32_t s = sample_idx ? (uint32_t)sample_idx[(size_t)row * n_points + j]
                              : sample_index(key, (uint32_t)j, k, replace);
      s = s < k ? s : k - 1;                     // a caller-supplied index is clamped, never trusted
      double x, y, z;
      if (REC16) {
        const float4 r = p4[s];
        x = r.x; y = r.y; z = r.z;
        src[i] = __float_as_uint(r.w);
      } else {
        x = p[(size_t)s * 3]; y = p[(size_t)s * 3 + 1]; z = p[(size_t)s * 3 + 2];
        src[i] = s;
      }
      R.apply(x, y, z);
      px[i] = x; py[i] = y; pz[i] = z;
      sx += x; sy += y; sz += z;
    }
  }
  sx = wave_sum(sx); sy = wave_sum(sy); sz = wave_sum(sz);
  if (lane == 0) { s_red[wave][0] = sx; s_red[wave][1] = sy; s_red[wave][2] = sz; }
  __syncthreads();
  if (tid < 3) {
    double v = s_red[0][tid];
    for (int w = 1; w < kWaves; ++w) v += s_red[w][tid];
    s_out[tid] = v / (double)n_points;
  }
  __syncthreads();
  const double mx_ = s_out[0], my_ = s_out[1], mz_ = s_out[2];
  double far = 0.0;
#pragma unroll
  for (int i = 0; i < kMaxPer; ++i) {
    const int j = tid + i * kBlock;
    if (j < n_points) {
      px[i] -= mx_; py[i] -= my_; pz[i] -= mz_;
      far = fmax(far, sqrt((px[i] * px[i] + py[i] * py[i]) + pz[i] * pz[i]));
    }
  }
  far = wave_max(far);
  if (lane == 0) s_red[wave][3] = far;
  __syncthreads();
  if (tid == 0) {
    double v = s_red[0][3];
    for (int w = 1; w < kWaves; ++w) v = fmax(v, s_red[w][3]);
    s_out[3] = v < 1e-6 ? 1.0 : v;               // tiny point clouds, i.e. padding (base.py:726-727)
  }
  __syncthreads();
  const double max_dist = s_out[3];
#pragma unroll
  for (int i = 0; i < kMaxPer; ++i) {
    const int j = tid + i * kBlock;
    if (j < n_points) {
      float *o = fts + (size_t)j * 6;
      o[0] = (float)(px[i] / max_dist);
      o[1] = (float)(py[i] / max_dist);
      o[2] = (float)(pz[i] / max_dist);
      const size_t c = ((size_t)begin + src[i]) * 3;
      if (REC16) {                               // colours came with the record (little-endian r, g, b)
        o[3] = (float)((double)(src[i] & 255u) / 127.5 - 1.0);
        o[4] = (float)((double)((src[i] >> 8) & 255u) / 127.5 - 1.0);
        o[5] = (float)((double)((src[i] >> 16) & 255u) / 127.5 - 1.0);
      } else if (rgb_u8) {                       // colors / 127.5 - 1 in f64 (uint8 promotes), then .float()
        o[3] = (float)((double)rgb_u8[c] / 127.5 - 1.0);
        o[4] = (float)((double)rgb_u8[c + 1] / 127.5 - 1.0);
        o[5] = (float)((double)rgb_u8[c + 2] / 127.5 - 1.0);
      } else {                                   // float32 colours stay float32 under numpy's rules
        o[3] = rgb_f32[c] / 127.5f - 1.0f;
        o[4] = rgb_f32[c + 1] / 127.5f - 1.0f;
        o[5] = rgb_f32[c + 2] / 127.5f - 1.0f;
      }
    }
  }
}

}  // namespace gps_obj

// One body for the by-value entry (seed_dev NULL) and the seed-word entry.
static int obj_processing_post_launch(int n_rows, int n_points, const float *xyz, const void *rgb, int rgb_is_u8,
                                      const int64_t *obj_offsets, const int32_t *row_obj, const int32_t *sample_idx,
                                      uint64_t seed, const uint64_t *seed_dev, const float *rot, const int32_t *row_rot,
                                      float *obj_fts, float *obj_locs, float *obj_boxes, uint8_t *obj_masks,
                                      gps_stream_t stream) {
  if (n_rows < 0 || n_points <= 0) return GPS_ERR_INVALID_ARGUMENT;
  if (n_points > gps_obj::kBlock * gps_obj::kMaxPer) return GPS_ERR_UNSUPPORTED;
  if (n_rows == 0) return GPS_OK;
  if (!xyz || !obj_offsets || !row_obj || !obj_fts || !obj_locs) return GPS_ERR_INVALID_ARGUMENT;
  if ((rot == nullptr) != (row_rot == nullptr)) return GPS_ERR_INVALID_ARGUMENT;
  if (!rgb) {                                    // 16-byte records: colours travel in the 4th word
    if (((uintptr_t)xyz & 15u) != 0) return GPS_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(gps_obj::obj_processing_post_kernel<true>, dim3(n_rows), dim3(gps_obj::kBlock), 0,
                       (hipStream_t)stream, n_points, xyz, nullptr, nullptr, obj_offsets, row_obj, sample_idx, seed,
                       seed_dev, rot, row_rot, obj_fts, obj_locs, obj_boxes, obj_masks);
  } else {
    hipLaunchKernelGGL(gps_obj::obj_processing_post_kernel<false>, dim3(n_rows), dim3(gps_obj::kBlock), 0,
                       (hipStream_t)stream, n_points, xyz, rgb_is_u8 ? (const uint8_t *)rgb : nullptr,
                       rgb_is_u8 ? nullptr : (const float *)rgb, obj_offsets, row_obj, sample_idx, seed, seed_dev, rot,
                       row_rot, obj_fts, obj_locs, obj_boxes, obj_masks);
  }
  return hipGetLastError() == hipSuccess ? GPS_OK : GPS_ERR_LAUNCH;
}

extern "C" int gps_obj_processing_post(int n_rows, int n_points, const float *xyz, const void *rgb, int rgb_is_u8,
                                       const int64_t *obj_offsets, const int32_t *row_obj,
                                       const int32_t *sample_idx, uint64_t seed, const float *rot,
                                       const int32_t *row_rot, float *obj_fts, float *obj_locs, float *obj_boxes,
                                       uint8_t *obj_masks, gps_stream_t stream) {
  return obj_processing_post_launch(n_rows, n_points, xyz, rgb, rgb_is_u8, obj_offsets, row_obj, sample_idx, seed,
                                    nullptr, rot, row_rot, obj_fts, obj_locs, obj_boxes, obj_masks, stream);
}

extern "C" int gps_obj_processing_post_sw(int n_rows, int n_points, const float *xyz, const void *rgb, int rgb_is_u8,
                                          const int64_t *obj_offsets, const int32_t *row_obj,
                                          const int32_t *sample_idx, uint64_t seed, const uint64_t *seed_dev,
                                          const float *rot, const int32_t *row_rot, float *obj_fts, float *obj_locs,
                                          float *obj_boxes, uint8_t *obj_masks, gps_stream_t stream) {
  return obj_processing_post_launch(n_rows, n_points, xyz, rgb, rgb_is_u8, obj_offsets, row_obj, sample_idx, seed,
                                    seed_dev, rot, row_rot, obj_fts, obj_locs, obj_boxes, obj_masks, stream);
}

// ---- the augmented path ------------------------------------------------------------------------------
// Reference: ScanBase._obj_processing_aug, data/datasets/base.py:742-776, fed by DataAugmentor.update_data_dict,
// data/datasets/data_augmentor.py:156-215 -- the branch every config with a `data_aug:` block takes (train AND val).
// It is a different function from _post: it subsamples FIRST, takes the object size from the (jittered) sample before
// any translation / rotation, centre and box from the transformed sample, rotates as x @ R (not x @ R.T) and clamps
// max_dist at 1e-6.  Order per object: flip, scale about the mean of ALL points, subsample, jitter, size, scene +
// object translation, scene rotation, object rotation about the sample mean, colour delta, centre, unit ball.
//
// One workgroup per output row, the sampled points in VGPRs as above.  Only a row whose scale is on walks all k points
// of its object, and then only to sum them (flip is linear: the mean of the flipped points is the flipped mean);
// every other row touches the num_points gathered records alone.  The point shuffle (data_augmentor.py:211-212) needs
// no work here: every later step is a per-point map or an order-free reduction, so a permutation of the sample rows
// is a permutation of the (sample_idx, jitter_noise) the caller passes; device-drawn samples are already in random order.
// Arithmetic in float64 with block reductions, the sizes rounded from their float64 value, everything else rounded to
// f32 at the end (the reference rounds to f32 earlier -- at the scene rotation or at the tensor conversion; the
// difference is its rounding noise, tests/test_gpu_objects_aug.py).
namespace gps_obj {

// Components [0, NS) are summed, [NS, NS + NMIN) minimised, the rest maximised; every thread gets the results.
template <int NS, int NMIN, int NMAX>
__device__ __forceinline__ void block_reduce(double *v, double (*s_red)[9], double *s_out, int tid) {
  constexpr int N = NS + NMIN + NMAX;
  static_assert(N <= 9, "s_red / s_out hold nine components");
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int c = 0; c < N; ++c) v[c] = c < NS ? wave_sum(v[c]) : (c < NS + NMIN ? wave_min(v[c]) : wave_max(v[c]));
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < N; ++c) s_red[wave][c] = v[c];
  }
  __syncthreads();
  if (tid < N) {
    double r = s_red[0][tid];
    for (int w = 1; w < kWaves; ++w)
      r = tid < NS ? r + s_red[w][tid] : (tid < NS + NMIN ? fmin(r, s_red[w][tid]) : fmax(r, s_red[w][tid]));
    s_out[tid] = r;
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < N; ++c) v[c] = s_out[c];
}

// x @ M for a row-major 3x3 (np.matmul(x, mat), data_augmentor.py:245-251): out_j = sum_c p_c * M[c][j]
__device__ __forceinline__ void mul_right(const double *__restrict__ m, double &x, double &y, double &z) {
  const double a = (x * m[0] + y * m[3]) + z * m[6];
  const double b = (x * m[1] + y * m[4]) + z * m[7];
  const double c = (x * m[2] + y * m[5]) + z * m[8];
  x = a; y = b; z = c;
}

// Standard normal for (row key, point, coordinate): Box-Muller on two words of the mix64 stream.
__device__ __forceinline__ double normal_draw(uint64_t key, uint32_t j, uint32_t c) {
  const uint64_t h1 = mix64(key ^ (((uint64_t)j << 2 | c) << 1));
  const uint64_t h2 = mix64(h1 ^ 0xC2B2AE3D27D4EB4Full);
  const double u1 = (double)((h1 >> 11) + 1ull) * 0x1.0p-53;          // (0, 1]
  const double u2 = (double)(h2 >> 11) * 0x1.0p-53;                   // [0, 1)
  return sqrt(-2.0 * log(u1)) * cospi(2.0 * u2);
}

// layout of one entry of the parameter table (doubles), include/gps_hip.h
constexpr int kAugStride = GPS_OBJ_AUG_STRIDE;
constexpr int kAugScale = 1, kAugJitter = 2, kAugSceneTrans = 5, kAugObjTrans = 8, kAugRgb = 11, kAugFlip = 14,
              kAugSceneRot = 23, kAugObjRot = 32;

template <bool REC16>
__global__ __launch_bounds__(kBlock) void obj_processing_aug_kernel(
    int n_points, const float *__restrict__ xyz, const uint8_t *__restrict__ rgb_u8,
    const float *__restrict__ rgb_f32, const int64_t *__restrict__ obj_offsets,
    const int32_t *__restrict__ row_obj, const int32_t *__restrict__ sample_idx,
    const float *__restrict__ noise_f32, const double *__restrict__ noise_f64, uint64_t seed,
    const uint64_t *__restrict__ seed_dev, const double *__restrict__ aug, const int32_t *__restrict__ row_aug, int n_aug,
    float *__restrict__ obj_fts,
    float *__restrict__ obj_locs, float *__restrict__ obj_boxes, uint8_t *__restrict__ obj_masks) {
  __shared__ double s_red[kWaves][9];
  __shared__ double s_out[9];
  const int row = blockIdx.x, tid = threadIdx.x;
  const int obj = row_obj[row];
  float *fts = obj_fts + (size_t)row * n_points * 6;
  int64_t begin = 0, k64 = 0;
  if (obj >= 0) {
    begin = obj_offsets[obj];
    k64 = obj_offsets[obj + 1] - begin;
  }
  if (obj < 0 || k64 <= 0) {                    // padding slot: features 1.0, locations 0.0, mask off
    for (int i = tid; i < n_points * 6; i += kBlock) fts[i] = 1.0f;
    if (tid < 6) {
      obj_locs[(size_t)row * 6 + tid] = 0.0f;
      if (obj_boxes) obj_boxes[(size_t)row * 6 + tid] = 0.0f;
    }
    if (tid == 0 && obj_masks) obj_masks[row] = 0;
    return;
  }
  const uint32_t k = (uint32_t)k64;
  const int set = aug != nullptr ? row_aug[row] : -1;
  const double *A = aug + (size_t)(set >= 0 && set < n_aug ? set : 0) * kAugStride;
  const uint32_t flags = set >= 0 && set < n_aug ? (uint32_t)A[0] : 0u;
  const float *p = xyz + (size_t)begin * (REC16 ? 4 : 3);
  const float4 *p4 = reinterpret_cast<const float4 *>(xyz) + begin;

  // ---- scale only: the mean of ALL points (a sum; flip is applied to the mean) ----------------
  double cs[3] = {0, 0, 0};
  if (flags & GPS_OBJ_AUG_SCALE) {
    uint32_t i = tid;
    if (REC16) {
      for (; i + 3u * kBlock < k; i += 4u * kBlock) {
        const float4 r0 = p4[i], r1 = p4[i + kBlock], r2 = p4[i + 2u * kBlock], r3 = p4[i + 3u * kBlock];
        cs[0] += ((double)r0.x + (double)r1.x) + ((double)r2.x + (double)r3.x);
        cs[1] += ((double)r0.y + (double)r1.y) + ((double)r2.y + (double)r3.y);
        cs[2] += ((double)r0.z + (double)r1.z) + ((double)r2.z + (double)r3.z);
      }
      for (; i < k; i += kBlock) {
        const float4 r = p4[i];
        cs[0] += r.x; cs[1] += r.y; cs[2] += r.z;
      }
    } else {
      for (; i < k; i += kBlock) {
        cs[0] += p[(size_t)i * 3]; cs[1] += p[(size_t)i * 3 + 1]; cs[2] += p[(size_t)i * 3 + 2];
      }
    }
    block_reduce<3, 0, 0>(cs, s_red, s_out, tid);
    cs[0] /= (double)k; cs[1] /= (double)k; cs[2] /= (double)k;
    if (flags & GPS_OBJ_AUG_FLIP) mul_right(A + kAugFlip, cs[0], cs[1], cs[2]);
  }

  // ---- the sampled points, held in registers: flip, scale, jitter -> size ---------------------
  const bool replace = k < (uint32_t)n_points;
  const uint64_t key = mix64(row_seed(seed, seed_dev) ^ mix64((uint64_t)row));   // per output row: a scene drawn twice differs
  const uint64_t nkey = mix64(key ^ 0x6A09E667F3BCC909ull);  // the jitter stream, independent of the sampler's
  double px[kMaxPer], py[kMaxPer], pz[kMaxPer];
  uint32_t src[kMaxPer];                         // sampled index, or (REC16) the record's colour word
  double mm[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
  for (int i = 0; i < kMaxPer; ++i) {
    const int j = tid + i * kBlock;
    if (j < n_points) {
      uint32_t s = sample_idx ? (uint32_t)sample_idx[(size_t)row * n_points + j]
                              : sample_index(key, (uint32_t)j, k, replace);
      s = s < k ? s : k - 1;                     // a caller-supplied index is clamped, never trusted
      double x, y, z;
      if (REC16) {
        const float4 r = p4[s];
        x = r.x; y = r.y; z = r.z;
        src[i] = __float_as_uint(r.w);
      } else {
        x = p[(size_t)s * 3]; y = p[(size_t)s * 3 + 1]; z = p[(size_t)s * 3 + 2];
        src[i] = s;
      }
      if (flags & GPS_OBJ_AUG_FLIP) mul_right(A + kAugFlip, x, y, z);
      if (flags & GPS_OBJ_AUG_SCALE) {           // (x - c) * s + c, data_augmentor.py:254-256
        const double sc = A[kAugScale];
        x = (x - cs[0]) * sc + cs[0]; y = (y - cs[1]) * sc + cs[1]; z = (z - cs[2]) * sc + cs[2];
      }
      if (flags & GPS_OBJ_AUG_JITTER) {          // x + (randn - 0.5) * scale, data_augmentor.py:259-260
        double nx, ny, nz;
        const size_t q = ((size_t)row * n_points + j) * 3;
        if (noise_f64) {
          nx = noise_f64[q]; ny = noise_f64[q + 1]; nz = noise_f64[q + 2];
        } else if (noise_f32) {
          nx = noise_f32[q]; ny = noise_f32[q + 1]; nz = noise_f32[q + 2];
        } else {
          nx = normal_draw(nkey, (uint32_t)j, 0); ny = normal_draw(nkey, (uint32_t)j, 1);
          nz = normal_draw(nkey, (uint32_t)j, 2);
        }
        x += (nx - 0.5) * A[kAugJitter]; y += (ny - 0.5) * A[kAugJitter + 1]; z += (nz - 0.5) * A[kAugJitter + 2];
      }
      px[i] = x; py[i] = y; pz[i] = z;
      mm[0] = fmin(mm[0], x); mm[1] = fmin(mm[1], y); mm[2] = fmin(mm[2], z);
      mm[3] = fmax(mm[3], x); mm[4] = fmax(mm[4], y); mm[5] = fmax(mm[5], z);
    }
  }
  block_reduce<0, 3, 3>(mm, s_red, s_out, tid);
  const double size[3] = {mm[3] - mm[0], mm[4] - mm[1], mm[5] - mm[2]};   // before translation and rotation

  // ---- translate, scene rotation -> sample mean ------------------------------------------------
  double ctr[3] = {0, 0, 0};
#pragma unroll
  for (int i = 0; i < kMaxPer; ++i) {
    const int j = tid + i * kBlock;
    if (j < n_points) {
      if (flags & GPS_OBJ_AUG_SCENE_TRANS) {
        px[i] += A[kAugSceneTrans]; py[i] += A[kAugSceneTrans + 1]; pz[i] += A[kAugSceneTrans + 2];
      }
      if (flags & GPS_OBJ_AUG_OBJ_TRANS) {
        px[i] += A[kAugObjTrans]; py[i] += A[kAugObjTrans + 1]; pz[i] += A[kAugObjTrans + 2];
      }
      if (flags & GPS_OBJ_AUG_SCENE_ROT) mul_right(A + kAugSceneRot, px[i], py[i], pz[i]);
      ctr[0] += px[i]; ctr[1] += py[i]; ctr[2] += pz[i];
    }
  }
  block_reduce<3, 0, 0>(ctr, s_red, s_out, tid);
  ctr[0] /= (double)n_points; ctr[1] /= (double)n_points; ctr[2] /= (double)n_points;

  // ---- centre (the object rotation turns about it and so leaves it in place), box, farthest point ---
  double bx[7] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY, 0.0};
#pragma unroll
  for (int i = 0; i < kMaxPer; ++i) {
    const int j = tid + i * kBlock;
    if (j < n_points) {
      px[i] -= ctr[0]; py[i] -= ctr[1]; pz[i] -= ctr[2];
      if (flags & GPS_OBJ_AUG_OBJ_ROT) mul_right(A + kAugObjRot, px[i], py[i], pz[i]);
      bx[0] = fmin(bx[0], px[i]); bx[1] = fmin(bx[1], py[i]); bx[2] = fmin(bx[2], pz[i]);
      bx[3] = fmax(bx[3], px[i]); bx[4] = fmax(bx[4], py[i]); bx[5] = fmax(bx[5], pz[i]);
      bx[6] = fmax(bx[6], sqrt((px[i] * px[i] + py[i] * py[i]) + pz[i] * pz[i]));
    }
  }
  block_reduce<0, 3, 4>(bx, s_red, s_out, tid);
  if (tid < 3) {
    obj_locs[(size_t)row * 6 + tid] = (float)ctr[tid];
    obj_locs[(size_t)row * 6 + 3 + tid] = (float)size[tid];
    if (obj_boxes) {
      obj_boxes[(size_t)row * 6 + tid] = (float)((bx[tid] + bx[3 + tid]) / 2.0 + ctr[tid]);
      obj_boxes[(size_t)row * 6 + 3 + tid] = (float)size[tid];
    }
  }
  if (tid == 0 && obj_masks) obj_masks[row] = 1;
  const double max_dist = fmax(bx[6], 1e-6);     // clamp_(min=1e-6), base.py:768 -- not "-> 1" as in _post
  double dr = 0, dg = 0, db = 0;
  if (flags & GPS_OBJ_AUG_RGB) { dr = A[kAugRgb]; dg = A[kAugRgb + 1]; db = A[kAugRgb + 2]; }
#pragma unroll
  for (int i = 0; i < kMaxPer; ++i) {
    const int j = tid + i * kBlock;
    if (j < n_points) {
      float *o = fts + (size_t)j * 6;
      o[0] = (float)(px[i] / max_dist);
      o[1] = (float)(py[i] / max_dist);
      o[2] = (float)(pz[i] / max_dist);
      const size_t c = ((size_t)begin + src[i]) * 3;
      double r, g, b;
      if (REC16) {                               // colours came with the record (little-endian r, g, b)
        r = (double)(src[i] & 255u) / 127.5 - 1.0;
        g = (double)((src[i] >> 8) & 255u) / 127.5 - 1.0;
        b = (double)((src[i] >> 16) & 255u) / 127.5 - 1.0;
      } else if (rgb_u8) {                       // colors / 127.5 - 1 in f64 (uint8 promotes)
        r = (double)rgb_u8[c] / 127.5 - 1.0;
        g = (double)rgb_u8[c + 1] / 127.5 - 1.0;
        b = (double)rgb_u8[c + 2] / 127.5 - 1.0;
      } else {                                   // float32 colours are scaled in float32 by the loader (numpy's rules)
        r = rgb_f32[c] / 127.5f - 1.0f;
        g = rgb_f32[c + 1] / 127.5f - 1.0f;
        b = rgb_f32[c + 2] / 127.5f - 1.0f;
      }
      o[3] = (float)(r + dr); o[4] = (float)(g + dg); o[5] = (float)(b + db);
    }
  }
}

}  // namespace gps_obj

static int obj_processing_aug_launch(int n_rows, int n_points, const float *xyz, const void *rgb, int rgb_is_u8,
                                     const int64_t *obj_offsets, const int32_t *row_obj, const int32_t *sample_idx,
                                     const void *jitter_noise, int noise_is_f64, uint64_t seed, const uint64_t *seed_dev,
                                     const double *aug, const int32_t *row_aug, int n_aug, float *obj_fts,
                                     float *obj_locs, float *obj_boxes, uint8_t *obj_masks, gps_stream_t stream) {
  if (n_rows < 0 || n_points <= 0) return GPS_ERR_INVALID_ARGUMENT;
  if (n_points > gps_obj::kBlock * gps_obj::kMaxPer) return GPS_ERR_UNSUPPORTED;
  if (n_rows == 0) return GPS_OK;
  if (!xyz || !obj_offsets || !row_obj || !obj_fts || !obj_locs) return GPS_ERR_INVALID_ARGUMENT;
  if ((aug == nullptr) != (row_aug == nullptr)) return GPS_ERR_INVALID_ARGUMENT;
  if (aug && n_aug <= 0) return GPS_ERR_INVALID_ARGUMENT;
  const float *n32 = noise_is_f64 ? nullptr : (const float *)jitter_noise;
  const double *n64 = noise_is_f64 ? (const double *)jitter_noise : nullptr;
  if (!rgb) {                                    // 16-byte records: colours travel in the 4th word
    if (((uintptr_t)xyz & 15u) != 0) return GPS_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(gps_obj::obj_processing_aug_kernel<true>, dim3(n_rows), dim3(gps_obj::kBlock), 0,
                       (hipStream_t)stream, n_points, xyz, nullptr, nullptr, obj_offsets, row_obj, sample_idx, n32, n64,
                       seed, seed_dev, aug, row_aug, n_aug, obj_fts, obj_locs, obj_boxes, obj_masks);
  } else {
    hipLaunchKernelGGL(gps_obj::obj_processing_aug_kernel<false>, dim3(n_rows), dim3(gps_obj::kBlock), 0,
                       (hipStream_t)stream, n_points, xyz, rgb_is_u8 ? (const uint8_t *)rgb : nullptr,
                       rgb_is_u8 ? nullptr : (const float *)rgb, obj_offsets, row_obj, sample_idx, n32, n64, seed,
                       seed_dev, aug, row_aug, n_aug, obj_fts, obj_locs, obj_boxes, obj_masks);
  }
  return hipGetLastError() == hipSuccess ? GPS_OK : GPS_ERR_LAUNCH;
}

extern "C" int gps_obj_processing_aug(int n_rows, int n_points, const float *xyz, const void *rgb, int rgb_is_u8,
                                      const int64_t *obj_offsets, const int32_t *row_obj,
                                      const int32_t *sample_idx, const void *jitter_noise, int noise_is_f64,
                                      uint64_t seed, const double *aug, const int32_t *row_aug, int n_aug,
                                      float *obj_fts, float *obj_locs, float *obj_boxes, uint8_t *obj_masks,
                                      gps_stream_t stream) {
  return obj_processing_aug_launch(n_rows, n_points, xyz, rgb, rgb_is_u8, obj_offsets, row_obj, sample_idx, jitter_noise,
                                   noise_is_f64, seed, nullptr, aug, row_aug, n_aug, obj_fts, obj_locs, obj_boxes,
                                   obj_masks, stream);
}

extern "C" int gps_obj_processing_aug_sw(int n_rows, int n_points, const float *xyz, const void *rgb, int rgb_is_u8,
                                         const int64_t *obj_offsets, const int32_t *row_obj,
                                         const int32_t *sample_idx, const void *jitter_noise, int noise_is_f64,
                                         uint64_t seed, const uint64_t *seed_dev, const double *aug,
                                         const int32_t *row_aug, int n_aug, float *obj_fts, float *obj_locs,
                                         float *obj_boxes, uint8_t *obj_masks, gps_stream_t stream) {
  return obj_processing_aug_launch(n_rows, n_points, xyz, rgb, rgb_is_u8, obj_offsets, row_obj, sample_idx, jitter_noise,
                                   noise_is_f64, seed, seed_dev, aug, row_aug, n_aug, obj_fts, obj_locs, obj_boxes,
                                   obj_masks, stream);
}
