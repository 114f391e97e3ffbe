// gps_qa.hip -- the question-answering fine-tune step above the encoders (gfx950): the attention-flatten pooling of
// the QA head and the multi-label answer loss.
//
// Reference: modules/heads/qa_head.py
//   :56-67  AttFlat.forward after the first Linear + GELU: Linear(M -> G), masked_fill(-1e9), softmax over the tokens,
//           G weighted sums of x, cat.  torch: linear, masked_fill, softmax, G x (slice, mul, sum), cat = 6 + 3 G
//           launches forward and about twice that backward for a (B, T, D) tensor of a few MB.
//           optim/loss/loss.py
//   :50-53  answer_loss: binary_cross_entropy_with_logits(sum) / B over (B, 8864) int64 labels cast to float every step.
// Here: one forward launch (logits, softmax and pooling; grid = column slices of D x scenes, every slice workgroup
// recomputes the small T x M logit product and pools its own 128 columns, so B = 64 scenes fill the chip), two backward
// launches (x is read once: dx and d att together; then the softmax Jacobian, dh and the per-workgroup partial sums of
// dw2 / db2, which the last workgroup to arrive adds in a fixed order: no float atomics, run-to-run identical).
// The BCE loss is one launch per direction, workgroup partials + the same ticket finish.  Memory-bound throughout:
// 16-byte loads (8 bf16 or 2 x 4 fp32 per thread and trip), fp32 accumulation.  Row access (load8 / store8, bf16 stores
// by f2bf), wave reductions and the ticket (publish / arrive_and_last / peek) are gps_dev.h's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gps_bce_dev.h"
#include "gps_dev.h"
#include "gps_hip.h"

namespace gps_qa {

constexpr int kBlock = 256, kWaves = 4;
constexpr int kSlice = 128;        // columns of D per forward workgroup: 16 column threads x 8
constexpr int kRowsDx = 16;        // token rows per workgroup of the dx / d att kernel (4 per wave)
constexpr int kRowsDh = 32;        // token rows per workgroup of the dh / dw2 kernel
constexpr int kMaxG = 4;
constexpr int kBceMaxBlocks = 1024;

using namespace gps_dev;

// ---------------------------------------------------------------------------------------------------------------------
// AttFlat forward.  grid (ceil(D / 128), B), 256 threads.
//   LDS: w2 (G M) | att (G T, glimpse-major, padded to 4 floats) | 16 x 128 partial sums
// ---------------------------------------------------------------------------------------------------------------------
template <bool XB, bool HB>
__global__ __launch_bounds__(kBlock) void attflat_fwd_kernel(int T, int G, int D, int M, const void *__restrict__ x,
                                                             long long ldx, const void *__restrict__ h,
                                                             const float *__restrict__ w2, const float *__restrict__ b2,
                                                             const uint8_t *__restrict__ keep, float *__restrict__ pooled,
                                                             float *__restrict__ att) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float *w2s = sm, *lg = sm + G * M, *part = lg + ((G * T + 3) & ~3);      // every carve 16-byte aligned
  const int b = blockIdx.y, c0 = blockIdx.x * kSlice, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < G * M; i += kBlock) w2s[i] = w2[i];
  __syncthreads();
  const int M8 = M >> 3;
  // logits: two token rows per wave and trip, their loads requested together
  for (int t0 = w; t0 < T; t0 += 2 * kWaves) {
    float acc[2][kMaxG] = {};
    for (int i = lane; i < M8; i += 64) {
      float hv[2][8];
#pragma unroll
      for (int u = 0; u < 2; ++u) load8<HB>(h, ((size_t)b * T + min(t0 + u * kWaves, T - 1)) * M + (size_t)i * 8, hv[u]);
#pragma unroll
      for (int g = 0; g < kMaxG; ++g) {
        if (g < G) {
          const float4 wa = *reinterpret_cast<const float4 *>(w2s + g * M + i * 8);
          const float4 wb = *reinterpret_cast<const float4 *>(w2s + g * M + i * 8 + 4);
#pragma unroll
          for (int u = 0; u < 2; ++u)
            acc[u][g] += (hv[u][0] * wa.x + hv[u][1] * wa.y) + (hv[u][2] * wa.z + hv[u][3] * wa.w) +
                         (hv[u][4] * wb.x + hv[u][5] * wb.y) + (hv[u][6] * wb.z + hv[u][7] * wb.w);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int t = t0 + u * kWaves;
#pragma unroll
      for (int g = 0; g < kMaxG; ++g) {
        if (g < G) {
          const float a = wave_sum(acc[u][g]);
          if (lane == 0 && t < T) lg[g * T + t] = (keep && !keep[(size_t)b * T + t]) ? -1e9f : a + b2[g];
        }
      }
    }
  }
  __syncthreads();
  if (w < G) {                                                      // wave g: softmax over the tokens of glimpse g
    float *l = lg + w * T;
    float m = -INFINITY;
    for (int t = lane; t < T; t += 64) m = fmaxf(m, l[t]);
    m = wave_max(m);
    float s = 0.f;
    for (int t = lane; t < T; t += 64) s += expf(l[t] - m);
    s = wave_sum(s);
    const float inv = 1.f / s;
    for (int t = lane; t < T; t += 64) {
      const float p = expf(l[t] - m) * inv;
      l[t] = p;
      if (blockIdx.x == 0) att[((size_t)b * T + t) * G + w] = p;
    }
  }
  __syncthreads();
  // pooling: thread = 8 columns x every 16th token, four rows in flight
  const int ct = threadIdx.x & 15, tl = threadIdx.x >> 4, col = c0 + ct * 8;
  float acc[kMaxG][8] = {};
  if (col < D) {
    for (int t0 = tl; t0 < T; t0 += 64) {
      float xv[4][8];
#pragma unroll
      for (int u = 0; u < 4; ++u) load8<XB>(x, ((size_t)b * T + min(t0 + 16 * u, T - 1)) * ldx + col, xv[u]);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int t = t0 + 16 * u;
#pragma unroll
        for (int g = 0; g < kMaxG; ++g) {
          if (g < G) {
            const float a = t < T ? lg[g * T + min(t, T - 1)] : 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[g][k] += a * xv[u][k];
          }
        }
      }
    }
  }
#pragma unroll
  for (int g = 0; g < kMaxG; ++g) {
    if (g < G) {
      __syncthreads();
#pragma unroll
      for (int k = 0; k < 8; ++k) part[tl * kSlice + ct * 8 + k] = acc[g][k];
      __syncthreads();
      if (threadIdx.x < kSlice && c0 + (int)threadIdx.x < D) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) s += part[j * kSlice + threadIdx.x];
        pooled[(size_t)b * G * D + (size_t)g * D + c0 + threadIdx.x] = s;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// AttFlat backward, first launch.  grid (ceil(T / 16), B): a wave reads a row of x once and produces
//   datt[b][t][g] = <dpooled[b][g], x[b][t]>      dx[b][t] = sum_g att[b][t][g] dpooled[b][g]
//   LDS: dpooled[b] (G D)
// ---------------------------------------------------------------------------------------------------------------------
template <bool XB>
__global__ __launch_bounds__(kBlock) void attflat_bwd_x_kernel(int T, int G, int D, const void *__restrict__ x,
                                                               long long ldx, const float *__restrict__ att,
                                                               const float *__restrict__ dpooled, void *__restrict__ dx,
                                                               long long lddx, float *__restrict__ datt) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int b = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int GD4 = (G * D) >> 2;
  const float4 *dp4 = reinterpret_cast<const float4 *>(dpooled + (size_t)b * G * D);
  for (int i = threadIdx.x; i < GD4; i += kBlock) reinterpret_cast<float4 *>(sm)[i] = dp4[i];
  __syncthreads();
  const int D8 = D >> 3;
  for (int r = 0; r < kRowsDx / kWaves; ++r) {
    const int t = blockIdx.x * kRowsDx + w * (kRowsDx / kWaves) + r;
    if (t >= T) break;                                              // wave-uniform
    const size_t row = (size_t)b * T + t;
    float a[kMaxG], dacc[kMaxG] = {};
#pragma unroll
    for (int g = 0; g < kMaxG; ++g) a[g] = g < G ? att[row * G + g] : 0.f;
    for (int i = lane; i < D8; i += 64) {
      float xv[8], dv[8] = {};
      load8<XB>(x, row * ldx + (size_t)i * 8, xv);
#pragma unroll
      for (int g = 0; g < kMaxG; ++g) {
        if (g < G) {
          const float4 pa = *reinterpret_cast<const float4 *>(sm + g * D + i * 8);
          const float4 pb = *reinterpret_cast<const float4 *>(sm + g * D + i * 8 + 4);
          const float p[8] = {pa.x, pa.y, pa.z, pa.w, pb.x, pb.y, pb.z, pb.w};
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            dacc[g] += p[k] * xv[k];
            dv[k] += a[g] * p[k];
          }
        }
      }
      if (dx) store8<XB>(dx, row * lddx + (size_t)i * 8, dv);
    }
#pragma unroll
    for (int g = 0; g < kMaxG; ++g) {
      if (g < G) {
        const float s = wave_sum(dacc[g]);
        if (lane == 0) datt[row * G + g] = s;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// AttFlat backward, second launch.  grid (ceil(T / 32), B).
//   s_g = sum_t att datt;  dl[t][g] = keep[t] ? att (datt - s_g) : 0  (masked_fill passes no gradient)
//   dh[t][m] = sum_g dl[t][g] w2[g][m];  partial[(b, chunk)] = (sum_t dl[t][g] h[t][m],  sum_t dl[t][g])
//   the last workgroup to arrive adds the partials in (b, chunk) order -> dw2, db2.
//   LDS: w2 (G M) | row-group partials (RG G M, RG = min(32, 256 / (M / 8))) | dl (32 x 4) | s (4) | 1 int
// ---------------------------------------------------------------------------------------------------------------------
template <bool HB>
__global__ __launch_bounds__(kBlock) void attflat_bwd_h_kernel(int T, int G, int M, const void *__restrict__ h,
                                                               const float *__restrict__ w2,
                                                               const uint8_t *__restrict__ keep,
                                                               const float *__restrict__ att,
                                                               const float *__restrict__ datt, void *__restrict__ dh,
                                                               float *__restrict__ dw2, float *__restrict__ db2,
                                                               float *__restrict__ partial, unsigned int *__restrict__ ticket) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int M8 = M >> 3;
  const int RG = min(kRowsDh, kBlock / M8);
  float *w2s = sm, *pr = sm + G * M, *dl = pr + RG * G * M, *sg = dl + kRowsDh * kMaxG;
  int *flag = reinterpret_cast<int *>(sg + kMaxG);
  const int b = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int t_lo = blockIdx.x * kRowsDh, rows = min(kRowsDh, T - t_lo);
  for (int i = threadIdx.x; i < G * M; i += kBlock) w2s[i] = w2[i];
  if (w < G) {
    float s = 0.f;
    for (int t = lane; t < T; t += 64) s += att[((size_t)b * T + t) * G + w] * datt[((size_t)b * T + t) * G + w];
    s = wave_sum(s);
    if (lane == 0) sg[w] = s;
  }
  __syncthreads();
  if (threadIdx.x < kRowsDh * kMaxG) {
    const int r = threadIdx.x >> 2, g = threadIdx.x & 3;
    float v = 0.f;
    if (r < rows && g < G) {
      const size_t row = (size_t)b * T + t_lo + r;
      if (!keep || keep[row]) v = att[row * G + g] * (datt[row * G + g] - sg[g]);
    }
    dl[threadIdx.x] = v;
  }
  __syncthreads();
  const int rg = threadIdx.x / M8, m8 = threadIdx.x - rg * M8;
  if (rg < RG) {
    float acc[kMaxG][8] = {};
    for (int r = rg; r < rows; r += RG) {
      const size_t at = ((size_t)b * T + t_lo + r) * M + (size_t)m8 * 8;
      float hv[8], dv[8] = {};
      load8<HB>(h, at, hv);
#pragma unroll
      for (int g = 0; g < kMaxG; ++g) {
        if (g < G) {
          const float c = dl[r * kMaxG + g];
          const float4 wa = *reinterpret_cast<const float4 *>(w2s + g * M + m8 * 8);
          const float4 wb = *reinterpret_cast<const float4 *>(w2s + g * M + m8 * 8 + 4);
          const float wv[8] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            acc[g][k] += c * hv[k];
            dv[k] += c * wv[k];
          }
        }
      }
      if (dh) store8<HB>(dh, at, dv);
    }
#pragma unroll
    for (int g = 0; g < kMaxG; ++g) {
      if (g < G) {
#pragma unroll
        for (int k = 0; k < 8; ++k) pr[(rg * G + g) * M + m8 * 8 + k] = acc[g][k];
      }
    }
  }
  __syncthreads();
  const int GM = G * M, stride = GM + G;
  const int nparts = gridDim.x * gridDim.y, mine = blockIdx.y * gridDim.x + blockIdx.x;
  float *out = partial + (size_t)mine * stride;
  for (int i = threadIdx.x; i < GM; i += kBlock) {
    float s = 0.f;
    for (int j = 0; j < RG; ++j) s += pr[j * GM + i];
    publish(out + i, s);
  }
  if (threadIdx.x < G) {
    float s = 0.f;
    for (int r = 0; r < kRowsDh; ++r) s += dl[r * kMaxG + threadIdx.x];
    publish(out + GM + threadIdx.x, s);
  }
  if (!arrive_and_last(ticket, (unsigned int)nparts, flag)) return;
  for (int i = threadIdx.x; i < stride; i += kBlock) {
    float s = 0.f;
    int p = 0;
    for (; p + 4 <= nparts; p += 4) {                               // four partials requested together, added in order
      const float v0 = peek(partial + (size_t)p * stride + i), v1 = peek(partial + (size_t)(p + 1) * stride + i);
      const float v2 = peek(partial + (size_t)(p + 2) * stride + i), v3 = peek(partial + (size_t)(p + 3) * stride + i);
      s += v0; s += v1; s += v2; s += v3;
    }
    for (; p < nparts; ++p) s += peek(partial + (size_t)p * stride + i);
    if (i < GM) dw2[i] = s;
    else db2[i - GM] = s;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// scale * sum w BCEWithLogits(x, y) and its gradient.  A chunk = 8 consecutive columns of one row; chunk c belongs to
// workgroup c / chunks_per_block (a fixed assignment: the partial sums do not depend on the schedule).
// VEC: cols, both pitches multiples of 8 and 16-byte aligned bases -> 16-byte accesses; else element accesses.
// ---------------------------------------------------------------------------------------------------------------------
using gps_bce::bce_term;
using gps_bce::sigmoidf;
template <bool YF>
__device__ __forceinline__ void load_y8(const void *y, size_t idx, float v[8]) {
  if constexpr (YF) load8<false>(y, idx, v);
  else {
    const longlong2 *p = reinterpret_cast<const longlong2 *>(reinterpret_cast<const long long *>(y) + idx);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const longlong2 q = p[k];
      v[2 * k] = (float)q.x;
      v[2 * k + 1] = (float)q.y;
    }
  }
}
template <bool YF>
__device__ __forceinline__ float load_y1(const void *y, size_t idx) {
  if constexpr (YF) return reinterpret_cast<const float *>(y)[idx];
  else return (float) reinterpret_cast<const long long *>(y)[idx];
}

template <bool XB, bool YF, bool VEC, bool BWD>
__global__ __launch_bounds__(kBlock) void bce_kernel(int rows, int cols, const void *__restrict__ x, long long ldx,
                                                     const void *__restrict__ y, const uint8_t *__restrict__ wgt,
                                                     float scale, long long chunks_per_block,
                                                     float *__restrict__ partial, float *__restrict__ loss,
                                                     unsigned int *__restrict__ ticket, const float *__restrict__ gout,
                                                     void *__restrict__ dx, long long lddx) {
  __shared__ float red[kWaves];
  __shared__ int flag;
  const int C8 = (cols + 7) >> 3;
  const long long total = (long long)rows * C8;
  const long long lo = (long long)blockIdx.x * chunks_per_block, hi = min(total, lo + chunks_per_block);
  const float gs = BWD ? gout[0] * scale : 0.f;
  float sum = 0.f;
  for (long long c = lo + threadIdx.x; c < hi; c += kBlock) {
    const int r = (int)(c / C8), c8 = (int)(c - (long long)r * C8) * 8;
    const size_t xi = (size_t)r * ldx + c8, yi = (size_t)r * cols + c8;
    if constexpr (VEC) {
      float xv[8], yv[8], ov[8];
      load8<XB>(x, xi, xv);
      load_y8<YF>(y, yi, yv);
      uint2 wq = make_uint2(0x01010101u, 0x01010101u);
      if (wgt) wq = *reinterpret_cast<const uint2 *>(wgt + yi);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float wk = (((k < 4 ? wq.x : wq.y) >> (8 * (k & 3))) & 0xffu) ? 1.f : 0.f;
        if constexpr (BWD) ov[k] = gs * wk * (sigmoidf(xv[k]) - yv[k]);
        else sum += wk * bce_term(xv[k], yv[k]);
      }
      if constexpr (BWD) store8<XB>(dx, (size_t)r * lddx + c8, ov);
    } else {
      for (int k = 0; k < 8 && c8 + k < cols; ++k) {
        const float xv = load1<XB>(x, xi + k), yv = load_y1<YF>(y, yi + k);
        const float wk = (!wgt || wgt[yi + k]) ? 1.f : 0.f;
        if constexpr (BWD) store1<XB>(dx, (size_t)r * lddx + c8 + k, gs * wk * (sigmoidf(xv) - yv));
        else sum += wk * bce_term(xv, yv);
      }
    }
  }
  if constexpr (!BWD) {
    sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) publish(partial + blockIdx.x, (red[0] + red[1]) + (red[2] + red[3]));
    if (!arrive_and_last(ticket, gridDim.x, &flag)) return;
    if (threadIdx.x >= 64) return;
    float s = 0.f;
    for (int i = threadIdx.x; i < (int)gridDim.x; i += 64) s += peek(partial + i);
    s = wave_sum(s);
    if (threadIdx.x == 0) loss[0] = s * scale;
  }
}

}  // namespace gps_qa

using gps_dev::aligned16;
using gps_dev::launch_status;
static inline int attflat_shape_status(int B, int T, int G, int D, int M) {
  if (B < 0 || T < 1 || G < 1 || D < 1 || M < 1) return GPS_ERR_INVALID_ARGUMENT;
  if (T > 512 || G > gps_qa::kMaxG || (D & 7) || (M & 7) || D > 2048 || M > 1024) return GPS_ERR_UNSUPPORTED;
  return GPS_OK;
}
static inline long long bce_blocks(long long chunks) {
  const long long per = (chunks + gps_qa::kBceMaxBlocks - 1) / gps_qa::kBceMaxBlocks;
  const long long per_block = per < gps_qa::kBlock ? gps_qa::kBlock : per;      // at least one chunk per thread
  return (chunks + per_block - 1) / per_block;
}

extern "C" {

long long gps_attflat_backward_ws_floats(int B, int T, int G, int M) {
  if (B < 0 || T < 1 || G < 1 || M < 1) return 0;
  const long long chunks = (T + gps_qa::kRowsDh - 1) / gps_qa::kRowsDh;
  return (long long)B * T * G + (long long)B * chunks * ((long long)G * M + G);
}

int gps_attflat_forward(int B, int T, int G, int D, int M, int x_bf16, const void *x, long long ld_x, int h_bf16,
                        const void *h, const float *w2, const float *b2, const unsigned char *keep, float *pooled,
                        float *att, gps_stream_t stream) {
  const int st = attflat_shape_status(B, T, G, D, M);
  if (st != GPS_OK) return st;
  if (B == 0) return GPS_OK;
  if (!x || !h || !w2 || !b2 || !pooled || !att || ld_x < D) return GPS_ERR_INVALID_ARGUMENT;
  if ((ld_x & 7) || !aligned16(x) || !aligned16(h) || B > 65535) return GPS_ERR_UNSUPPORTED;
  const size_t lds = (size_t)(G * M + ((G * T + 3) & ~3) + 16 * gps_qa::kSlice) * sizeof(float);
  const dim3 grid((D + gps_qa::kSlice - 1) / gps_qa::kSlice, B);
#define GPS_QA_FWD(XB, HB)                                                                                             \
  hipLaunchKernelGGL((gps_qa::attflat_fwd_kernel<XB, HB>), grid, dim3(gps_qa::kBlock), lds, (hipStream_t)stream, T, G, \
                     D, M, x, ld_x, h, w2, b2, keep, pooled, att)
  if (x_bf16 && h_bf16) GPS_QA_FWD(true, true);
  else if (x_bf16) GPS_QA_FWD(true, false);
  else if (h_bf16) GPS_QA_FWD(false, true);
  else GPS_QA_FWD(false, false);
#undef GPS_QA_FWD
  return launch_status();
}

int gps_attflat_backward(int B, int T, int G, int D, int M, int x_bf16, const void *x, long long ld_x, int h_bf16,
                         const void *h, const float *w2, const unsigned char *keep, const float *att,
                         const float *dpooled, void *dx, long long ld_dx, void *dh, float *dw2, float *db2,
                         float *workspace, unsigned int *ticket, gps_stream_t stream) {
  const int st = attflat_shape_status(B, T, G, D, M);
  if (st != GPS_OK) return st;
  if (B == 0) return GPS_OK;
  if (!x || !h || !w2 || !att || !dpooled || !dw2 || !db2 || !workspace || !ticket || ld_x < D || (dx && ld_dx < D))
    return GPS_ERR_INVALID_ARGUMENT;
  if ((ld_x & 7) || (dx && (ld_dx & 7)) || !aligned16(x) || !aligned16(h) || !aligned16(dpooled) ||
      (dx && !aligned16(dx)) || (dh && !aligned16(dh)) || B > 65535)
    return GPS_ERR_UNSUPPORTED;
  float *datt = workspace, *partial = workspace + (size_t)B * T * G;
  {
    const size_t lds = (size_t)G * D * sizeof(float);
    const dim3 grid((T + gps_qa::kRowsDx - 1) / gps_qa::kRowsDx, B);
    if (x_bf16)
      hipLaunchKernelGGL(gps_qa::attflat_bwd_x_kernel<true>, grid, dim3(gps_qa::kBlock), lds, (hipStream_t)stream, T, G, D,
                         x, ld_x, att, dpooled, dx, ld_dx, datt);
    else
      hipLaunchKernelGGL(gps_qa::attflat_bwd_x_kernel<false>, grid, dim3(gps_qa::kBlock), lds, (hipStream_t)stream, T, G, D,
                         x, ld_x, att, dpooled, dx, ld_dx, datt);
    if (launch_status() != GPS_OK) return GPS_ERR_LAUNCH;
  }
  const int M8 = M >> 3;
  const int RG = gps_qa::kBlock / M8 < gps_qa::kRowsDh ? gps_qa::kBlock / M8 : gps_qa::kRowsDh;
  const size_t lds = (size_t)(G * M + RG * G * M + gps_qa::kRowsDh * gps_qa::kMaxG + gps_qa::kMaxG + 1) * sizeof(float);
  const dim3 grid((T + gps_qa::kRowsDh - 1) / gps_qa::kRowsDh, B);
  if (h_bf16)
    hipLaunchKernelGGL(gps_qa::attflat_bwd_h_kernel<true>, grid, dim3(gps_qa::kBlock), lds, (hipStream_t)stream, T, G, M, h,
                       w2, keep, att, datt, dh, dw2, db2, partial, ticket);
  else
    hipLaunchKernelGGL(gps_qa::attflat_bwd_h_kernel<false>, grid, dim3(gps_qa::kBlock), lds, (hipStream_t)stream, T, G, M, h,
                       w2, keep, att, datt, dh, dw2, db2, partial, ticket);
  return launch_status();
}

int gps_bce_logits_partial_floats(int rows, int cols) {
  if (rows < 1 || cols < 1) return 1;
  return (int)bce_blocks((long long)rows * ((cols + 7) / 8));
}

}  // extern "C"

template <bool BWD>
static int bce_launch(int rows, int cols, int x_bf16, const void *x, long long ld_x, int y_f32, const void *y,
                      const unsigned char *w, float scale, float *partial, float *loss, unsigned int *ticket,
                      const float *gout, void *dx, long long ld_dx, gps_stream_t stream) {
  const long long chunks = (long long)rows * ((cols + 7) / 8);
  const long long blocks = bce_blocks(chunks), per_block = (chunks + blocks - 1) / blocks;
  const int esz = x_bf16 ? 2 : 4;
  const bool vec = !(cols & 7) && !(ld_x & 7) && aligned16(x) && aligned16(y) && (!w || !(reinterpret_cast<uintptr_t>(w) & 7)) &&
                   (!BWD || (!(ld_dx & 7) && aligned16(dx)));
  if ((reinterpret_cast<uintptr_t>(x) % esz) || (reinterpret_cast<uintptr_t>(y) % (y_f32 ? 4 : 8))) return GPS_ERR_UNSUPPORTED;
#define GPS_QA_BCE(XB, YF, VEC)                                                                                        \
  hipLaunchKernelGGL((gps_qa::bce_kernel<XB, YF, VEC, BWD>), dim3((unsigned)blocks), dim3(gps_qa::kBlock), 0,          \
                     (hipStream_t)stream, rows, cols, x, ld_x, y, w, scale, per_block, partial, loss, ticket, gout, dx, \
                     ld_dx)
#define GPS_QA_BCE2(XB, YF) do { if (vec) GPS_QA_BCE(XB, YF, true); else GPS_QA_BCE(XB, YF, false); } while (0)
  if (x_bf16 && y_f32) GPS_QA_BCE2(true, true);
  else if (x_bf16) GPS_QA_BCE2(true, false);
  else if (y_f32) GPS_QA_BCE2(false, true);
  else GPS_QA_BCE2(false, false);
#undef GPS_QA_BCE2
#undef GPS_QA_BCE
  return launch_status();
}

extern "C" {

int gps_bce_logits_forward(int rows, int cols, int x_bf16, const void *x, long long ld_x, int y_f32, const void *y,
                           const unsigned char *w, float scale, float *partial, float *loss, unsigned int *ticket,
                           gps_stream_t stream) {
  if (rows < 0 || cols < 0) return GPS_ERR_INVALID_ARGUMENT;
  if (rows == 0 || cols == 0) return GPS_OK;                        // nothing launched: the caller's loss is 0
  if (!x || !y || !partial || !loss || !ticket || ld_x < cols) return GPS_ERR_INVALID_ARGUMENT;
  return bce_launch<false>(rows, cols, x_bf16, x, ld_x, y_f32, y, w, scale, partial, loss, ticket, nullptr, nullptr, 0, stream);
}

int gps_bce_logits_backward(int rows, int cols, int x_bf16, const void *x, long long ld_x, int y_f32, const void *y,
                            const unsigned char *w, float scale, const float *grad_out, void *dx, long long ld_dx,
                            gps_stream_t stream) {
  if (rows < 0 || cols < 0) return GPS_ERR_INVALID_ARGUMENT;
  if (rows == 0 || cols == 0) return GPS_OK;
  if (!x || !y || !grad_out || !dx || ld_x < cols || ld_dx < cols) return GPS_ERR_INVALID_ARGUMENT;
  return bce_launch<true>(rows, cols, x_bf16, x, ld_x, y_f32, y, w, scale, nullptr, nullptr, nullptr, grad_out, dx, ld_dx, stream);
}

}  // extern "C"
