// gps_aug_draw.hip -- the draws of DataAugmentor and build_rotate_mat for a whole batch in one launch (gfx950).
//
// Reference: DataAugmentor.scene_aug / obj_aug, data/datasets/data_augmentor.py:39-154 (what is drawn, under which
// knob, in which form) and build_rotate_mat, data/data_utils.py:163-178.  The reference draws per sample on the
// data-loader workers from numpy's global stream; here one thread per output row draws from the counter stream of
// gps_dropout.h and writes the parameter table gps_obj_processing_aug reads (or the rotation table of
// gps_obj_processing_post), so a captured loader chain redraws on every replay from one device word.  The law is
// stated in include/gps_hip.h; tests/augdraw_cases.py restates it in numpy / math.
//
// Compiled with -ffp-contract=off: the scale (one multiply, one add), the angles and the 3x3 products are the IEEE
// operations the law names, in its order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gps_dropout.h"
#include "gps_hip.h"

namespace gps_aug_draw_ns {

constexpr int kBlock = 64;

// math.cos / math.sin (and np.cos / np.sin) of 0, pi/2, pi, 3 pi/2 as float64: what the reference's axis-aligned
// rotations are built from (6.1e-17, not 0)
__device__ const double kCos4[4] = {0x1.0p+0, 0x1.1a62633145c07p-54, -0x1.0p+0, -0x1.a79394c9e8a0ap-53};
__device__ const double kSin4[4] = {0x0.0p+0, 0x1.0p+0, 0x1.1a62633145c07p-53, -0x1.0p+0};
__device__ const double kAngle4[4] = {0.0, 0x1.921fb54442d18p+0, 0x1.921fb54442d18p+1, 0x1.2d97c7f3321d2p+2};
// the six permutations of (0, 1, 2) in lexicographic order
__device__ const int kPerm6[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};

struct Stream {
  uint64_t seed;   // S + 6
  uint64_t base;   // (b * (O + 1) + slot) * 64
  __device__ __forceinline__ uint32_t u32(int k) const { return gps_dropout::rng_u32(seed, base + (uint64_t)k); }
  // fires iff u32 < T(p), T(p) = floor(p * 2^32) as a 64-bit number
  __device__ __forceinline__ bool fires(int k, double p) const {
    return (uint64_t)u32(k) < (uint64_t)(p * 4294967296.0);
  }
  __device__ __forceinline__ int choice(int k, int n) const { return (int)(((uint64_t)u32(k) * (uint64_t)n) >> 32); }
  __device__ __forceinline__ double uniform(int k) const { return (double)u32(k) * 0x1.0p-32; }
  // Box-Muller on the words k, k + 1: u1 in (0, 1], u2 in [0, 1)
  __device__ __forceinline__ double normal(int k) const {
    const double u1 = ((double)u32(k) + 1.0) * 0x1.0p-32;
    const double u2 = (double)u32(k + 1) * 0x1.0p-32;
    return sqrt(-2.0 * log(u1)) * cospi(2.0 * u2);
  }
};

// C = A . B, row-major 3x3, every element ((a0 * b0 + a1 * b1) + a2 * b2)
__device__ __forceinline__ void mat3_mul(const double *a, const double *b, double *c) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) c[i * 3 + j] = (a[i * 3] * b[j] + a[i * 3 + 1] * b[3 + j]) + a[i * 3 + 2] * b[6 + j];
}

// data_augmentor.py:69-93 / :120-144 under the law of the header -> out (9 doubles, row-major)
__device__ void draw_rotation(const Stream &st, const gps_aug_knob &kn, double *out) {
  double c[3], s[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double v = kn.value[i];
    if (kn.axis_align) {
      const int a = st.choice(GPS_AUG_K_ROT_ANGLE + i, 4);
      if (v == 0.0) {
        c[i] = kCos4[0]; s[i] = kSin4[0];
      } else if (v == 1.0) {
        c[i] = kCos4[a]; s[i] = kSin4[a];
      } else {
        const double th = kAngle4[a] * v;
        c[i] = cos(th); s[i] = sin(th);
      }
    } else {
      const double th = ((st.uniform(GPS_AUG_K_ROT_ANGLE + i) * 2.0) * 0x1.921fb54442d18p+1 - 0x1.921fb54442d18p+1) * v;
      c[i] = cos(th); s[i] = sin(th);
    }
  }
  double m[3][9] = {{1, 0, 0, 0, c[0], -s[0], 0, s[0], c[0]},
                    {c[1], 0, s[1], 0, 1, 0, -s[1], 0, c[1]},
                    {c[2], s[2], 0, -s[2], c[2], 0, 0, 0, 1}};
  const int pi = kn.shuffle ? st.choice(GPS_AUG_K_ROT_PERM, 6) : 0;
  double t[9];
  mat3_mul(m[kPerm6[pi][0]], m[kPerm6[pi][1]], t);
  mat3_mul(t, m[kPerm6[pi][2]], out);
}

__device__ __forceinline__ void draw_translation(const Stream &st, const gps_aug_knob &kn, double *out) {
#pragma unroll
  for (int i = 0; i < 3; ++i) out[i] = st.normal(GPS_AUG_K_TRANS + 2 * i) * kn.value[i];
}

// One thread per output row (b, o).  The scene's draws are recomputed by each of its O threads (some twenty hashes):
// no shared state, no second launch.
__global__ __launch_bounds__(kBlock) void aug_table_kernel(gps_aug_draw_args a, int per_obj, double *__restrict__ aug,
                                                           int32_t *__restrict__ row_aug) {
  const int row = blockIdx.x * kBlock + threadIdx.x;
  if (row >= a.B * a.O) return;
  const int b = row / a.O, o = row - b * a.O;
  const uint64_t S = (a.seed + (a.seed_dev ? *a.seed_dev : 0ull)) + 6ull;
  double e[GPS_OBJ_AUG_STRIDE];
#pragma unroll
  for (int i = 0; i < GPS_OBJ_AUG_STRIDE; ++i) e[i] = 0.0;
  uint32_t flags = 0;
  if (a.scene_on) {
    const Stream st{S, ((uint64_t)b * (uint64_t)(a.O + 1)) * 64ull};
    if (a.scene_trans.enabled && st.fires(GPS_AUG_K_TRANS_P, a.scene_trans.p)) {
      draw_translation(st, a.scene_trans, e + 5);
      flags |= GPS_OBJ_AUG_SCENE_TRANS;
    }
    if (a.scene_scale.enabled && st.fires(GPS_AUG_K_SCALE_P, a.scene_scale.p)) {
      e[1] = st.uniform(GPS_AUG_K_SCALE) * (a.scene_scale.value[1] - a.scene_scale.value[0]) + a.scene_scale.value[0];
      flags |= GPS_OBJ_AUG_SCALE;
    }
    if (a.scene_flip.enabled && st.fires(GPS_AUG_K_FLIP_P, a.scene_flip.p)) {
      const int kind = st.choice(GPS_AUG_K_FLIP, 4);          // x, y, x + y, or none at all
      e[14] = (kind == 0 || kind == 2) ? -1.0 : 1.0;
      e[18] = (kind == 1 || kind == 2) ? -1.0 : 1.0;
      e[22] = 1.0;
      flags |= GPS_OBJ_AUG_FLIP;
    }
    if (a.scene_rot.enabled && st.fires(GPS_AUG_K_ROT_P, a.scene_rot.p)) {
      draw_rotation(st, a.scene_rot, e + 23);
      flags |= GPS_OBJ_AUG_SCENE_ROT;
    }
    if (a.color_jitter) {
#pragma unroll
      for (int i = 0; i < 3; ++i) e[11 + i] = st.normal(GPS_AUG_K_RGB + 2 * i) * 0.1;
      flags |= GPS_OBJ_AUG_RGB;
    }
  }
  if (a.obj_on) {
    const Stream st{S, ((uint64_t)b * (uint64_t)(a.O + 1) + 1ull + (uint64_t)o) * 64ull};
    if (a.obj_trans.enabled && st.fires(GPS_AUG_K_TRANS_P, a.obj_trans.p)) {
      draw_translation(st, a.obj_trans, e + 8);
      flags |= GPS_OBJ_AUG_OBJ_TRANS;
    }
    if (a.obj_rot.enabled && st.fires(GPS_AUG_K_ROT_P, a.obj_rot.p)) {
      draw_rotation(st, a.obj_rot, e + 32);
      flags |= GPS_OBJ_AUG_OBJ_ROT;
    }
    if (a.jitter_on) {
      e[2] = a.jitter_value[0]; e[3] = a.jitter_value[1]; e[4] = a.jitter_value[2];
      flags |= GPS_OBJ_AUG_JITTER;
    }
  }
  e[0] = (double)flags;
  const int entry = per_obj ? row : b;
  row_aug[row] = flags ? entry : -1;
  if (per_obj || o == 0) {                       // every element of the table is written, a silent entry as zeros
    double *dst = aug + (size_t)entry * GPS_OBJ_AUG_STRIDE;
#pragma unroll
    for (int i = 0; i < GPS_OBJ_AUG_STRIDE; ++i) dst[i] = e[i];
  }
}

// build_rotate_mat (data/data_utils.py:163-178), rand_angle 'axis': one of four angles per scene, index 0 = no matrix
__global__ __launch_bounds__(kBlock) void rot_table_kernel(int B, int O, uint64_t seed, const uint64_t *seed_dev,
                                                           float *__restrict__ rot, int32_t *__restrict__ row_rot) {
  const int row = blockIdx.x * kBlock + threadIdx.x;
  if (row >= B * O) return;
  const int b = row / O, o = row - b * O;
  const uint64_t S = (seed + (seed_dev ? *seed_dev : 0ull)) + 7ull;
  const int a = (int)(((uint64_t)gps_dropout::rng_u32(S, (uint64_t)b) * 4ull) >> 32);
  row_rot[row] = a ? b : -1;
  if (o == 0) {
    const float c = (float)kCos4[a], s = (float)kSin4[a];
    float *m = rot + (size_t)b * 9;
    m[0] = c; m[1] = -s; m[2] = 0.f;
    m[3] = s; m[4] = c; m[5] = 0.f;
    m[6] = 0.f; m[7] = 0.f; m[8] = 1.f;
  }
}

static bool knob_ok(const gps_aug_knob &k) {
  return k.p >= 0.0 && k.p <= 1.0;               // false for a NaN
}

}  // namespace gps_aug_draw_ns

extern "C" int gps_aug_draw(const gps_aug_draw_args *args, double *aug, int32_t *row_aug, float *rot, int32_t *row_rot,
                            gps_stream_t stream) {
  using namespace gps_aug_draw_ns;
  if (!args) return GPS_ERR_INVALID_ARGUMENT;
  const gps_aug_draw_args &a = *args;
  if (a.B < 0 || a.O < 0) return GPS_ERR_INVALID_ARGUMENT;
  if (a.mode != GPS_AUG_DRAW_TABLE && a.mode != GPS_AUG_DRAW_ROT) return GPS_ERR_INVALID_ARGUMENT;
  if (a.mode == GPS_AUG_DRAW_TABLE && !(knob_ok(a.scene_trans) && knob_ok(a.scene_scale) && knob_ok(a.scene_flip) &&
                                        knob_ok(a.scene_rot) && knob_ok(a.obj_trans) && knob_ok(a.obj_rot)))
    return GPS_ERR_INVALID_ARGUMENT;
  if ((long long)a.B * (long long)a.O > 0x7fffffffll / GPS_OBJ_AUG_STRIDE) return GPS_ERR_UNSUPPORTED;
  const int n_rows = a.B * a.O;
  if (n_rows == 0) return GPS_OK;
  const int grid = (n_rows + kBlock - 1) / kBlock;
  if (a.mode == GPS_AUG_DRAW_TABLE) {
    if (!aug || !row_aug) return GPS_ERR_INVALID_ARGUMENT;
    const int per_obj = a.obj_on && (a.obj_trans.enabled || a.obj_rot.enabled);
    hipLaunchKernelGGL(aug_table_kernel, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, a, per_obj, aug, row_aug);
  } else {
    if (!rot || !row_rot) return GPS_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(rot_table_kernel, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, a.B, a.O, a.seed, a.seed_dev,
                       rot, row_rot);
  }
  return hipGetLastError() == hipSuccess ? GPS_OK : GPS_ERR_LAUNCH;
}
