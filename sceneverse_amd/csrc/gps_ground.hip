// gps_ground.hip -- the grounding fine-tune step above the encoders (gfx950): the tail of a `get_mlp_head` stack behind
// its first Linear, and the og3d cross entropy.
//
// Reference: modules/utils.py get_mlp_head = Linear -> ReLU -> LayerNorm(eps 1e-12) -> Dropout -> Linear
//            modules/heads/grounding_head.py:20-27  og3d_head(obj).squeeze(2), masked_fill_(~obj_masks, -inf); three
//                                                   class heads of the same shape with 607 outputs
//            optim/loss/loss.py:8-9                 og3d_loss = F.cross_entropy(og3d_logits, tgt_object_id.squeeze(1))
// torch: relu, layer_norm, dropout, linear, squeeze, logical_not, masked_fill_ per head forward, about three times that
// backward; log_softmax + nll_loss and their backwards for the loss.
// Here: `mlp_tail_fwd_kernel` reads the first Linear's output h once and writes the bf16 input of a following class
// Linear (z16) and / or the 1-output last Linear as a dot product with the -inf fill (logit); `mlp_tail_bwd_kernel`
// reads h once more and writes the gradient of the first Linear's output plus the four parameter gradients;
// `og3d_ce_kernel` writes the loss and its unit logit gradient in one launch.
//
// One wave per row, the row (<= 1024 elements, 8 consecutive elements per lane and step, 16-byte loads) stays in VGPRs:
// mean and variance two-pass from registers, row reductions are wave shuffles, no LDS in the forward, every load of a row
// is issued before its first use.  ReLU is applied here (idempotent: h may be the output of a bias + ReLU GEMM epilogue).
//
// Dropout index law: element (row r, column c) of the (n_rows, d) LayerNorm output draws
//     rng_u32(effective_seed(seed, seed_dev), r * d + c)          (gps_dropout.h, the library's one element stream)
// -- the LOGICAL index, whatever the pitch of h --, is kept iff that value is >= drop_threshold(p) and then scaled by
// 1 / (1 - p).  The backward kernel recomputes the mask from the same law; it is never stored.
//
// Parameter gradients: every workgroup reduces its waves' register accumulators through LDS into one partial row
// (dgamma | dbeta | dw2 | db2), the last workgroup to arrive (gps_dev.h: arrive_and_last) adds the partial rows in index
// order: no float atomics, run-to-run identical for a given n_rows.  Row access (Raw8, store8) and the wave reductions are
// gps_dev.h's, Drop / drop_factor are gps_dropout.h's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gps_dev.h"
#include "gps_dropout.h"
#include "gps_hip.h"

namespace gps_ground {

using namespace gps_dev;
using gps_dropout::Drop;
using gps_dropout::drop_factor;
using gps_dropout::effective_seed;

constexpr int kFwdBlock = 256, kFwdWaves = 4, kFwdMaxBlocks = 2048;
constexpr int kBwdBlock = 512, kBwdWaves = 8, kBwdMaxParts = 256, kBwdRowsPerBlock = 32;
constexpr int kCeBlock = 256, kCeWaves = 4, kCeMaxO = 512;
constexpr int kMaxD = 1024;

// ---------------------------------------------------------------------------------------------------------------------
// forward.  grid-stride over the rows, one wave per row; lane l of step i holds columns (i 64 + l) 8 .. + 7 (idle past d).
// ---------------------------------------------------------------------------------------------------------------------
template <bool HB, int ITERS>
__global__ __launch_bounds__(kFwdBlock) void mlp_tail_fwd_kernel(
    int n_rows, int d, const void *__restrict__ h, long long ld_h, const float *__restrict__ gamma,
    const float *__restrict__ beta, float eps, float p_drop, unsigned int thr, unsigned long long seed,
    const unsigned long long *__restrict__ seed_dev, const float *__restrict__ w2, const float *__restrict__ b2,
    const uint8_t *__restrict__ keep, uint16_t *__restrict__ z16, float *__restrict__ logit,
    float *__restrict__ mean_out, float *__restrict__ rstd_out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long *const sd = seed_dev;
  const Drop dr{thr, thr ? 1.f / (1.f - p_drop) : 1.f, thr ? effective_seed(seed, sd) : 0ull};
  const float inv_d = 1.f / (float)d;
  int col[ITERS];
  bool live[ITERS];
  float gm[ITERS][8], bt[ITERS][8], wv[ITERS][8];
#pragma unroll
  for (int i = 0; i < ITERS; ++i) {
    const int c = (i * 64 + lane) * 8;
    live[i] = c < d;
    col[i] = live[i] ? c : 0;                    // idle lanes re-read column 0 and drop the values
    load8<false>(gamma + col[i], 0, gm[i]);
    load8<false>(beta + col[i], 0, bt[i]);
#pragma unroll
    for (int k = 0; k < 8; ++k) wv[i][k] = 0.f;
    if (logit) load8<false>(w2 + col[i], 0, wv[i]);
  }
  const float bias2 = logit ? b2[0] : 0.f;
  for (int row = blockIdx.x * kFwdWaves + wave; row < n_rows; row += gridDim.x * kFwdWaves) {
    Raw8<HB> raw[ITERS];
#pragma unroll
    for (int i = 0; i < ITERS; ++i) raw[i].load(h, (size_t)row * ld_h + col[i]);
    const bool kept = !keep || keep[row] != 0;
    GPS_LOADS_ISSUED();
    float x[ITERS][8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
      raw[i].get(x[i]);
#pragma unroll
      for (int k = 0; k < 8; ++k) x[i][k] = live[i] ? fmaxf(x[i][k], 0.f) : 0.f;
      s += ((x[i][0] + x[i][1]) + (x[i][2] + x[i][3])) + ((x[i][4] + x[i][5]) + (x[i][6] + x[i][7]));
    }
    const float mean = wave_sum(s) * inv_d;
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
      float q = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float c = x[i][k] - mean;
        q += c * c;
      }
      v += live[i] ? q : 0.f;
    }
    const float rstd = rsqrtf(wave_sum(v) * inv_d + eps);
    if (lane == 0) {
      mean_out[row] = mean;
      rstd_out[row] = rstd;
    }
    float dot = 0.f;
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
      const unsigned long long e0 = (unsigned long long)row * (unsigned long long)d + (unsigned long long)col[i];
      float z[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        z[k] = ((x[i][k] - mean) * rstd * gm[i][k] + bt[i][k]) * drop_factor(dr, e0 + k);
        if (logit) dot += live[i] ? z[k] * wv[i][k] : 0.f;
      }
      if (z16 && live[i]) store8<true>(z16, (size_t)row * d + col[i], z);
    }
    if (logit) {
      dot = wave_sum(dot);
      if (lane == 0) logit[row] = kept ? dot + bias2 : -INFINITY;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// backward.  grid = gps_mlp_tail_partial_rows(n_rows) workgroups of 8 waves, grid-stride over the rows.
//   gz = dlogit[r] w2 (kept rows only) + dz16[r];  gy = gz * dropout factor;  a = gy gamma
//   dx = rstd (a - mean(a) - xhat mean(a xhat));  dpre = dx [h > 0]
//   dgamma += gy xhat;  dbeta += gy;  dw2 += dlogit[r] z;  db2 += dlogit[r]       (z = the forward's dropped output)
//   LDS: 8 x d floats (one quantity at a time) | 8 floats (db2) | 1 int
//   partial row of a workgroup: dgamma (d) | dbeta (d) | dw2 (d) | db2 | 3 pad   (stride 3 d + 4)
// ---------------------------------------------------------------------------------------------------------------------
template <bool HB, int ITERS>
__global__ __launch_bounds__(kBwdBlock) void mlp_tail_bwd_kernel(
    int n_rows, int d, const void *__restrict__ h, long long ld_h, const float *__restrict__ gamma,
    const float *__restrict__ beta, const float *__restrict__ mean_in, const float *__restrict__ rstd_in, float p_drop,
    unsigned int thr, unsigned long long seed, const unsigned long long *__restrict__ seed_dev,
    const float *__restrict__ w2, const uint8_t *__restrict__ keep, const float *__restrict__ dlogit,
    const uint16_t *__restrict__ dz16, void *__restrict__ dpre, long long ld_dpre, float *__restrict__ dgamma,
    float *__restrict__ dbeta, float *__restrict__ dw2, float *__restrict__ db2, float *partial,
    unsigned int *__restrict__ ticket) {
  extern __shared__ __attribute__((aligned(16))) float red[];
  float *red_b2 = red + kBwdWaves * d;
  int *flag = reinterpret_cast<int *>(red_b2 + kBwdWaves);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long *const sd = seed_dev;
  const Drop dr{thr, thr ? 1.f / (1.f - p_drop) : 1.f, thr ? effective_seed(seed, sd) : 0ull};
  const float inv_d = 1.f / (float)d;
  int col[ITERS];
  bool live[ITERS];
  float gm[ITERS][8], bt[ITERS][8], wv[ITERS][8];
  float gacc[ITERS][8] = {}, bacc[ITERS][8] = {}, wacc[ITERS][8] = {};
  float b2acc = 0.f;
#pragma unroll
  for (int i = 0; i < ITERS; ++i) {
    const int c = (i * 64 + lane) * 8;
    live[i] = c < d;
    col[i] = live[i] ? c : 0;
    load8<false>(gamma + col[i], 0, gm[i]);
    load8<false>(beta + col[i], 0, bt[i]);
#pragma unroll
    for (int k = 0; k < 8; ++k) wv[i][k] = 0.f;
    if (dlogit) load8<false>(w2 + col[i], 0, wv[i]);
  }
  for (int row = blockIdx.x * kBwdWaves + wave; row < n_rows; row += gridDim.x * kBwdWaves) {
    Raw8<HB> raw[ITERS];
    Raw8<true> graw[ITERS];
#pragma unroll
    for (int i = 0; i < ITERS; ++i) raw[i].load(h, (size_t)row * ld_h + col[i]);
    if (dz16) {
#pragma unroll
      for (int i = 0; i < ITERS; ++i) graw[i].load(dz16, (size_t)row * d + col[i]);
    }
    const float mean = mean_in[row], rstd = rstd_in[row];
    float dl = dlogit ? dlogit[row] : 0.f;
    const bool kept = !keep || keep[row] != 0;
    GPS_LOADS_ISSUED();
    if (!kept) dl = 0.f;                          // masked_fill passes no gradient, whatever dlogit holds there
    float xh[ITERS][8], a[ITERS][8];
    unsigned int pos = 0u;                        // bit (8 i + k): h > 0
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
      const unsigned long long e0 = (unsigned long long)row * (unsigned long long)d + (unsigned long long)col[i];
      float hv[8], gz[8] = {};
      raw[i].get(hv);
      if (dz16) graw[i].get(gz);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (hv[k] > 0.f) pos |= 1u << (8 * i + k);
        const float xk = live[i] ? fmaxf(hv[k], 0.f) : 0.f;
        const float f = drop_factor(dr, e0 + k);
        xh[i][k] = (xk - mean) * rstd;
        const float y = xh[i][k] * gm[i][k] + bt[i][k];
        const float gy = live[i] ? (gz[k] + dl * wv[i][k]) * f : 0.f;
        a[i][k] = gy * gm[i][k];
        s1 += a[i][k];
        s2 += a[i][k] * xh[i][k];
        gacc[i][k] += gy * xh[i][k];
        bacc[i][k] += gy;
        wacc[i][k] += live[i] ? dl * (y * f) : 0.f;
      }
    }
    b2acc += dl;
    s1 = wave_sum(s1) * inv_d;
    s2 = wave_sum(s2) * inv_d;
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
      float o[8];
#pragma unroll
      for (int k = 0; k < 8; ++k)
        o[k] = (pos >> (8 * i + k)) & 1u ? rstd * (a[i][k] - s1 - xh[i][k] * s2) : 0.f;
      if (live[i]) store8<HB>(dpre, (size_t)row * ld_dpre + col[i], o);
    }
  }
  // the waves' accumulators -> one partial row of this workgroup, one quantity at a time through LDS
  const int stride = 3 * d + 4;
  float *out = partial + (size_t)blockIdx.x * stride;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
      if (live[i]) {
#pragma unroll
        for (int k = 0; k < 8; ++k) red[wave * d + col[i] + k] = q == 0 ? gacc[i][k] : q == 1 ? bacc[i][k] : wacc[i][k];
      }
    }
    if (q == 0 && lane == 0) red_b2[wave] = b2acc;
    __syncthreads();
    for (int c = threadIdx.x; c < d; c += kBwdBlock) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < kBwdWaves; ++w) s += red[w * d + c];
      publish(out + q * d + c, s);
    }
    if (q == 0 && threadIdx.x < 4) {
      float s = 0.f;
      if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < kBwdWaves; ++w) s += red_b2[w];
      }
      publish(out + 3 * d + threadIdx.x, s);
    }
  }
  if (!arrive_and_last(ticket, gridDim.x, flag)) return;
  // the last workgroup: partial rows added in index order, a thread per 4 columns, 8 rows requested together
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  const int nparts = (int)gridDim.x, groups = stride >> 2;
  for (int g4 = threadIdx.x; g4 < groups; g4 += kBwdBlock) {
    const float *src = partial + (size_t)g4 * 4;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    int p = 0;
    for (; p + 8 <= nparts; p += 8) {
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const float4 *>(src + (size_t)(p + u) * stride);
#pragma unroll
      for (int u = 0; u < 8; ++u) { s.x += v[u].x; s.y += v[u].y; s.z += v[u].z; s.w += v[u].w; }
    }
    for (; p < nparts; ++p) {
      const float4 v = *reinterpret_cast<const float4 *>(src + (size_t)p * stride);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    const int c = g4 * 4;
    if (c < d) *reinterpret_cast<float4 *>(dgamma + c) = s;
    else if (c < 2 * d) *reinterpret_cast<float4 *>(dbeta + (c - d)) = s;
    else if (c < 3 * d) { if (dw2) *reinterpret_cast<float4 *>(dw2 + (c - 2 * d)) = s; }
    else if (db2) db2[0] = s.x;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// og3d cross entropy.  grid = ceil(B / 4) workgroups, one wave per scene row; lane l holds entries l, l + 64, ...
//   n_valid = #{target != ignore};  loss = sum_valid (lse(x_b) - x_b[t_b]) / n_valid
//   dlogits[b][o] = (softmax(x_b)[o] - [o == t_b]) / n_valid, 0 at -inf entries and in ignored rows
// Every wave counts n_valid itself from the B targets (integers: exact).  A target outside [0, O) counts as ignored.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCeBlock) void og3d_ce_kernel(int B, int O, const float *__restrict__ logits, long long ld,
                                                           const long long *__restrict__ target, float *__restrict__ loss,
                                                           float *__restrict__ dlogits, float *partial,
                                                           unsigned int *__restrict__ ticket) {
  __shared__ float red[kCeWaves];
  __shared__ int flag;
  constexpr int kPer = kCeMaxO / 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x * kCeWaves + wave;
  float x[kPer];
  long long t = -1;
  if (b < B) {
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int o = lane + 64 * j;
      x[j] = o < O ? logits[(size_t)b * ld + o] : -INFINITY;
    }
    t = target[b];
  }
  int cnt = 0;
  for (int i = lane; i < B; i += 64) {
    const long long ti = target[i];
    cnt += (ti >= 0 && ti < O) ? 1 : 0;
  }
  GPS_LOADS_ISSUED();
  const float inv_n = 1.f / (float)wave_sum(cnt);              // no valid row: inf here, NaN loss below, like torch's mean
  float row_loss = 0.f;
  if (b < B) {                                                      // wave-uniform
    const bool valid = t >= 0 && t < O;
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < kPer; ++j) m = fmaxf(m, x[j]);
    m = wave_max(m);
    float e[kPer], s = 0.f, xt = 0.f;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      e[j] = expf(x[j] - m);                                        // all -inf: NaN, as torch's log_softmax
      s += lane + 64 * j < O ? e[j] : 0.f;
      if ((long long)(lane + 64 * j) == t) xt = x[j];
    }
    s = wave_sum(s);
    xt = wave_sum(xt);
    if (valid) row_loss = (m + logf(s)) - xt;
    const float inv_s = 1.f / s;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int o = lane + 64 * j;
      if (o < O) {
        float g = 0.f;
        if (valid && x[j] != -INFINITY) g = (e[j] * inv_s - ((long long)o == t ? 1.f : 0.f)) * inv_n;
        dlogits[(size_t)b * O + o] = g;
      }
    }
  }
  if (lane == 0) red[wave] = row_loss;
  __syncthreads();
  if (threadIdx.x == 0) publish(partial + blockIdx.x, (red[0] + red[1]) + (red[2] + red[3]));
  if (!arrive_and_last(ticket, gridDim.x, &flag)) return;
  if (threadIdx.x >= 64) return;
  float s = 0.f;
  for (int i = threadIdx.x; i < (int)gridDim.x; i += 64) s += peek(partial + i);
  s = wave_sum(s);
  if (threadIdx.x == 0) loss[0] = s * inv_n;
}

}  // namespace gps_ground

using gps_dev::aligned16;
using gps_dev::launch_status;
static inline int tail_shape_status(int n_rows, int d) {
  if (n_rows < 0 || d < 1) return GPS_ERR_INVALID_ARGUMENT;
  if ((d & 7) || d < 8 || d > gps_ground::kMaxD) return GPS_ERR_UNSUPPORTED;
  return GPS_OK;
}

extern "C" {

int gps_mlp_tail_partial_rows(int n_rows) {
  if (n_rows < 1) return 1;
  const int want = (n_rows + gps_ground::kBwdRowsPerBlock - 1) / gps_ground::kBwdRowsPerBlock;
  return want < gps_ground::kBwdMaxParts ? want : gps_ground::kBwdMaxParts;
}

int gps_mlp_tail_forward(int n_rows, int d, int h_bf16, const void *h, long long ld_h, const float *gamma,
                         const float *beta, float eps, float p_drop, unsigned long long seed,
                         const unsigned long long *seed_dev, const float *w2, const float *b2, const unsigned char *keep,
                         void *z16, float *logit, float *mean, float *rstd, gps_stream_t stream) {
  const int st = tail_shape_status(n_rows, d);
  if (st != GPS_OK) return st;
  if (n_rows == 0) return GPS_OK;
  if (!h || !gamma || !beta || !mean || !rstd || (!z16 && !logit) || (logit && (!w2 || !b2)) || ld_h < d ||
      !(p_drop >= 0.f && p_drop < 1.f))
    return GPS_ERR_INVALID_ARGUMENT;
  if ((ld_h & 7) || !aligned16(h) || !aligned16(gamma) || !aligned16(beta) || (logit && !aligned16(w2)) ||
      (z16 && !aligned16(z16)))
    return GPS_ERR_UNSUPPORTED;
  const unsigned int thr = gps_dropout::drop_threshold(p_drop);
  const int want = (n_rows + gps_ground::kFwdWaves - 1) / gps_ground::kFwdWaves;
  const dim3 grid(want < gps_ground::kFwdMaxBlocks ? want : gps_ground::kFwdMaxBlocks);
#define GPS_GROUND_FWD(HB, IT)                                                                                         \
  hipLaunchKernelGGL((gps_ground::mlp_tail_fwd_kernel<HB, IT>), grid, dim3(gps_ground::kFwdBlock), 0,                  \
                     (hipStream_t)stream, n_rows, d, h, ld_h, gamma, beta, eps, p_drop, thr, seed, seed_dev, w2, b2,   \
                     keep, reinterpret_cast<uint16_t *>(z16), logit, mean, rstd)
  if (d <= 512) {
    if (h_bf16) GPS_GROUND_FWD(true, 1);
    else GPS_GROUND_FWD(false, 1);
  } else {
    if (h_bf16) GPS_GROUND_FWD(true, 2);
    else GPS_GROUND_FWD(false, 2);
  }
#undef GPS_GROUND_FWD
  return launch_status();
}

int gps_mlp_tail_backward(int n_rows, int d, int h_bf16, const void *h, long long ld_h, const float *gamma,
                          const float *beta, const float *mean, const float *rstd, float p_drop, unsigned long long seed,
                          const unsigned long long *seed_dev, const float *w2, const unsigned char *keep,
                          const float *dlogit, const void *dz16, void *dpre, long long ld_dpre, float *dgamma,
                          float *dbeta, float *dw2, float *db2, float *partial, unsigned int *ticket,
                          gps_stream_t stream) {
  const int st = tail_shape_status(n_rows, d);
  if (st != GPS_OK) return st;
  if (n_rows == 0) return GPS_OK;
  if (!h || !gamma || !beta || !mean || !rstd || (!dlogit && !dz16) || (dlogit && (!w2 || !dw2 || !db2)) || !dpre ||
      !dgamma || !dbeta || !partial || !ticket || ld_h < d || ld_dpre < d || !(p_drop >= 0.f && p_drop < 1.f))
    return GPS_ERR_INVALID_ARGUMENT;
  if ((ld_h & 7) || (ld_dpre & 7) || !aligned16(h) || !aligned16(dpre) || !aligned16(gamma) || !aligned16(beta) ||
      (dlogit && !aligned16(w2)) || (dz16 && !aligned16(dz16)) || !aligned16(partial) || !aligned16(dgamma) ||
      !aligned16(dbeta) || (dw2 && !aligned16(dw2)))
    return GPS_ERR_UNSUPPORTED;
  const unsigned int thr = gps_dropout::drop_threshold(p_drop);
  const dim3 grid(gps_mlp_tail_partial_rows(n_rows));
  const size_t lds = (size_t)(gps_ground::kBwdWaves * d + gps_ground::kBwdWaves + 1) * sizeof(float);
#define GPS_GROUND_BWD(HB, IT)                                                                                         \
  hipLaunchKernelGGL((gps_ground::mlp_tail_bwd_kernel<HB, IT>), grid, dim3(gps_ground::kBwdBlock), lds,                \
                     (hipStream_t)stream, n_rows, d, h, ld_h, gamma, beta, mean, rstd, p_drop, thr, seed, seed_dev, w2, \
                     keep, dlogit, reinterpret_cast<const uint16_t *>(dz16), dpre, ld_dpre, dgamma, dbeta, dw2, db2,   \
                     partial, ticket)
  if (d <= 512) {
    if (h_bf16) GPS_GROUND_BWD(true, 1);
    else GPS_GROUND_BWD(false, 1);
  } else {
    if (h_bf16) GPS_GROUND_BWD(true, 2);
    else GPS_GROUND_BWD(false, 2);
  }
#undef GPS_GROUND_BWD
  return launch_status();
}

int gps_og3d_ce_partial_floats(int B) {
  return B < 1 ? 1 : (B + gps_ground::kCeWaves - 1) / gps_ground::kCeWaves;
}

int gps_og3d_ce_forward(int B, int O, const float *logits, long long ld, const long long *target, float *loss,
                        float *dlogits, float *partial, unsigned int *ticket, gps_stream_t stream) {
  if (B < 0 || O < 1) return GPS_ERR_INVALID_ARGUMENT;
  if (O > gps_ground::kCeMaxO) return GPS_ERR_UNSUPPORTED;
  if (B == 0) return GPS_OK;
  if (!logits || !target || !loss || !dlogits || !partial || !ticket || ld < O) return GPS_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(gps_ground::og3d_ce_kernel, dim3(gps_og3d_ce_partial_floats(B)), dim3(gps_ground::kCeBlock), 0,
                     (hipStream_t)stream, B, O, logits, ld, target, loss, dlogits, partial, ticket);
  return launch_status();
}

}  // extern "C"
