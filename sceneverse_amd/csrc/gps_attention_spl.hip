// gps_attention_spl.hip -- the plane form of the language-conditioned pairwise-spatial self-attention core
// (reference modules/layers/transformers.py:193-239, fusion 'cond') for LONG rows: 145 .. 512 objects (BASELINE
// configs[4], 256 objects per scene).  Same mathematics and operand conventions as gps_attention_sp.hip (fp16 planes
// (B, 5, L, ld_pl), the conditioning vector read / its gradient written in place as bf16, the spatial term in base 2 with
// the log2(1e-6) clamp, fp32 softmax statistics, lse in natural log (B, H, L), transposed-orientation results); what
// changes is that the keys no longer fit in LDS (K + V of one (scene, head) are 147 KB at L = 512), so the structure is the
// block-streaming one of gps_attention_fa.hip:
//   * forward: a workgroup (4 waves) owns 64 queries of one (scene, head) and streams the keys through LDS in 64-row
//     blocks, double-buffered, with an online softmax.  A lane owns one query and the keys 16 j + 4 g + 0..3 of every
//     16-key tile (scores computed transposed, S^T = K Q^T): its planes are one 8-byte load per plane and tile, requested
//     one key block ahead (they are consumed before the score MFMAs of the block are needed);
//   * backward, launch 1 (64 queries per workgroup): the key blocks are walked TWICE -- the first walk accumulates
//     delta = rowsum(P dP) in fp32 (not rowsum(dO * O) from the bf16 output: see gps_attention_sp.hip bwd_strip), the
//     second forms dS, dQ^T = K^T dS^T and the gradient of the conditioning vector; delta goes to gps_attn_args.delta_ws;
//   * backward, launch 2 (64 keys per workgroup): the query blocks (Q, dO, lse, delta) are streamed; a wave computes the
//     transposed scores of its 16 keys against the 64 queries of the block (again one query per lane, four keys: the
//     same 8-byte plane loads), parks P and dS in its own LDS rows and reads them back hardware-transposed as the B
//     operands of dV^T = dO^T P and dK^T = Q^T dS (same wave: no barrier).
// Every output element is written by exactly one lane, every sum runs in a fixed order: the backward is run-to-run
// bit-identical (no atomics).  No dropout (the reference never applies it on this layer).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gps_hip.h"
#include "gps_attention_dev.h"
#include "gps_attention_run.h"

namespace gps_attn_spl {

using namespace gps_attn_dev;

constexpr int BLK = 64;                          // rows per streamed block, and queries / keys per workgroup
constexpr int kThreads = kStreamThreads;
constexpr int TPK = 16 + 8;                      // pitch of a wave's parked P / dS rows in the dK / dV launch (16 keys)

struct Params {
  int B, H, L, nblk;                             // nblk: 64-row blocks of the OWNED side per (scene, head)
  int ld_qkv, ld_o, ld_pl, ld_sw, ld_dqkv, ld_dsw;
  const uint16_t *q, *k, *v;                     // (B, L, ld_qkv), head h at column 64 h
  const _Float16 *pl;                            // (B, 5, L, ld_pl)
  const uint16_t *sw;                            // bf16: row (b, l) at sw + (b L + l) ld_sw, head h at + 6 h
  const uint8_t *mask;                           // (B, L), 1 = padded key, or null
  uint16_t *out;                                 // (B, L, ld_o)
  float *lse;                                    // (B, H, L), natural log
  const uint16_t *dout;                          // (B, L, ld_o)
  uint16_t *dq, *dk, *dv;                        // (B, L, ld_dqkv)
  uint16_t *dsw;                                 // bf16, addressed like sw with ld_dsw
  float *delta;                                  // (B, H, L): written by launch 1, read by launch 2
};

// which (scene, head, block) a workgroup owns: with B a multiple of 8 every workgroup of scene b runs on XCD b mod 8
// (block id mod 8), so the heads and blocks of a scene -- which all read its pairwise planes -- share that L2
struct Work {
  int b, h, blk;
  size_t row0;
};
__device__ __forceinline__ void locate(const Params &P, Work &W) {
  const int id = blockIdx.x, per = P.H * P.nblk;
  int b, rem;
  if ((P.B & 7) == 0) {
    const int xcd = id & 7, slot = id >> 3;
    b = (slot / per) * 8 + xcd;
    rem = slot % per;
  } else {
    b = id / per;
    rem = id % per;
  }
  W.b = b;
  W.h = rem / P.nblk;
  W.blk = rem % P.nblk;
  W.row0 = (size_t)b * P.L;
}

// additive key term (base 2): 0, or -inf for padded keys and keys past L
__device__ __forceinline__ float key_term(const Params &P, size_t row0, int t) {
  return (t < P.L && !(P.mask && P.mask[row0 + t])) ? 0.f : -INFINITY;
}

// what a (query, key tile) pair reads for the spatial term: the five fp16 planes of (query q, keys t0 .. t0 + 3), t0 a
// multiple of 4 -- one 8-byte load per plane; past the row: in-bounds columns (those keys are masked)
struct Planes4 {
  u32x2 d[5];
};
__device__ __forceinline__ void load_planes4(const Params &P, int b, int q, int t0, Planes4 &S) {
  // uniform (scalar) base + 32-bit lane offsets
  const unsigned int plane = (unsigned int)(P.L * P.ld_pl) * 2u;             // bytes
  const char *base = reinterpret_cast<const char *>(P.pl) + (size_t)b * 5 * plane;
  const unsigned int off = (unsigned int)(q * P.ld_pl + min(t0, P.ld_pl - 4)) * 2u;
#pragma unroll
  for (int d = 0; d < 5; ++d) S.d[d] = *reinterpret_cast<const u32x2 *>(base + d * plane + off);
}
// the conditioning vector (bias, w_1..w_5) of query q as loaded: six bf16
__device__ __forceinline__ void load_cond(const Params &P, size_t row0, int h, int q, unsigned int (&raw)[3]) {
  const unsigned int *p = reinterpret_cast<const unsigned int *>(P.sw + (row0 + q) * P.ld_sw + h * 6);
#pragma unroll
  for (int i = 0; i < 3; ++i) raw[i] = p[i];
}
// u = -log2(e) z of (query, key t0 + r);  e = 2^u,  log2(clamp(sigmoid z, 1e-6)) = max(-log2(1 + e), log2(1e-6))
__device__ __forceinline__ float spatial_u(const Planes4 &S, const float (&w)[6], int r) {
  float u = w[0];
#pragma unroll
  for (int d = 0; d < 5; ++d) u = fmaf((float)__builtin_bit_cast(f16x4, S.d[d])[r], w[1 + d], u);
  return u;
}

constexpr int kTile = BLK * KS;                                              // elements of one LDS tile
constexpr size_t kLdsQ = (size_t)4 * kTile * 2 + 2 * BLK * 4;                // K, V double-buffered + key terms
constexpr size_t kLdsKv = (size_t)4 * kTile * 2 + 2 * 2 * BLK * 4 + (size_t)4 * 2 * BLK * TPK * 2;   // + lse2, delta, parked P / dS

// ==========================================================================================
// forward: workgroup = 64 queries of one (scene, head); key blocks streamed, online softmax
// ==========================================================================================
__global__ __launch_bounds__(kThreads) void fwd_kernel(const Params P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint16_t *Kb = reinterpret_cast<uint16_t *>(smem);            // [2][64][KS]
  uint16_t *Vb = Kb + 2 * kTile;                                 // [2][64][KS]
  float *mbs = reinterpret_cast<float *>(Vb + 2 * kTile);        // [2][64] key term
  Work W;
  locate(P, W);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, g = lane >> 4;
  const int L = P.L, h = W.h;
  const uint16_t *qb = P.q + W.row0 * P.ld_qkv + h * DH;
  const uint16_t *kb = P.k + W.row0 * P.ld_qkv + h * DH;
  const uint16_t *vb = P.v + W.row0 * P.ld_qkv + h * DH;
  const int nkb = (L + BLK - 1) / BLK;
  const int qi = W.blk * BLK + 16 * wave + m;                    // this lane's query
  const bool active = W.blk * BLK + 16 * wave < L;               // wave-uniform: the strip has at least one query
  const int qc = min(qi, L - 1);                                 // rows past L: any valid row (never stored)

  BlockPair st;
  st.issue(kb, P.ld_qkv, vb, P.ld_qkv, 0, L);
  bf16x8 bq[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) bq[c] = as_frag(load_frag(qb, qc, P.ld_qkv, 32 * c + 8 * g));
  unsigned int wraw[3];
  load_cond(P, W.row0, h, qc, wraw);
  Planes4 S[4];                                                  // planes of the key block being processed
  if (active)
#pragma unroll
    for (int j = 0; j < 4; ++j) load_planes4(P, W.b, qc, 16 * j + 4 * g, S[j]);
  st.commit(Kb, Vb);
  if (threadIdx.x < BLK) mbs[threadIdx.x] = key_term(P, W.row0, threadIdx.x);
  float w[6];
  cond_vector(wraw, w);
  __syncthreads();

  float m_run = -INFINITY, l_run = 0.f;                          // running maximum (base-2 logits), lane's part of the normaliser
  f32x4 o[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) o[n] = zero_acc();

  for (int kbi = 0; kbi < nkb; ++kbi) {
    const int cur = kbi & 1, nxt = cur ^ 1;
    const bool more = kbi + 1 < nkb;
    if (more) st.issue(kb, P.ld_qkv, vb, P.ld_qkv, (kbi + 1) * BLK, L);
    const float mnext = (more && threadIdx.x < BLK) ? key_term(P, W.row0, (kbi + 1) * BLK + threadIdx.x) : 0.f;
    if (active) {
      const uint16_t *Kc = Kb + cur * kTile, *Vc = Vb + cur * kTile;
      const float *mc = mbs + cur * BLK;
      f32x4 x[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        x[j] = zero_acc();
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const u32x4 a = *reinterpret_cast<const u32x4 *>(Kc + (16 * j + m) * KS + 32 * c + 8 * g);
          x[j] = mfma32(as_frag(a), bq[c], x[j]);             // S^T[key 16 j + 4 g + r][query qi]
        }
      }
      float bmax = -INFINITY;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f32x4 kt = *reinterpret_cast<const f32x4 *>(mc + 16 * j + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float bias2 = spatial_bias2(__builtin_amdgcn_exp2f(spatial_u(S[j], w, r)));
          x[j][r] = fmaf(x[j][r], kC, bias2 + kt[r]);
        }
        bmax = fmaxf(fmaxf(bmax, fmaxf(x[j][0], x[j][1])), fmaxf(x[j][2], x[j][3]));
      }
      if (more)                                                  // the next block's planes: in flight behind P V and the barrier
#pragma unroll
        for (int j = 0; j < 4; ++j) load_planes4(P, W.b, qc, (kbi + 1) * BLK + 16 * j + 4 * g, S[j]);
      bmax = xor_max_g(bmax);
      const float m_new = fmaxf(m_run, bmax);
      const float m_use = m_new == -INFINITY ? 0.f : m_new;      // every key so far masked: keep the arithmetic finite
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);
      m_run = m_new;
      float psum = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          x[j][r] = __builtin_amdgcn_exp2f(x[j][r] - m_use);
          psum += x[j][r];
        }
      l_run = fmaf(l_run, alpha, psum);
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) o[n][r] *= alpha;
      // O^T strip += V^T P^T: o[n][r] = O[query qi][d = 16 n + 4 g + r]
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const bf16x8 pb = pack_tiles(x[2 * c], x[2 * c + 1]);
#pragma unroll
        for (int n = 0; n < 4; ++n) o[n] = mfma32(tr_frag_perm(Vc, KS, c, 16 * n, lane), pb, o[n]);
      }
    }
    if (more) {
      st.commit(Kb + nxt * kTile, Vb + nxt * kTile);
      if (threadIdx.x < BLK) mbs[nxt * BLK + threadIdx.x] = mnext;
    }
    __syncthreads();
  }
  if (!active) return;
  const float lsum = xor_sum_g(l_run);
  if (g == 0 && qi < L) P.lse[((size_t)W.b * P.H + h) * L + qi] = (m_run + __builtin_amdgcn_logf(lsum)) * kLn2;
  const float inv = __builtin_amdgcn_rcpf(lsum);
  if (qi < L) {
    uint16_t *op = P.out + (W.row0 + qi) * P.ld_o + h * DH + 4 * g;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const u32x2 v = {pack2(o[n][0] * inv, o[n][1] * inv), pack2(o[n][2] * inv, o[n][3] * inv)};
      *reinterpret_cast<u32x2 *>(op + 16 * n) = v;
    }
  }
}

// ==========================================================================================
// backward, launch 1: workgroup = 64 queries -> delta, dQ, d cond-vector; the key blocks walked twice
// ==========================================================================================
__global__ __launch_bounds__(kThreads) void bwd_dq_kernel(const Params P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint16_t *Kb = reinterpret_cast<uint16_t *>(smem);
  uint16_t *Vb = Kb + 2 * kTile;
  float *mbs = reinterpret_cast<float *>(Vb + 2 * kTile);
  Work W;
  locate(P, W);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, g = lane >> 4;
  const int L = P.L, h = W.h;
  const uint16_t *qb = P.q + W.row0 * P.ld_qkv + h * DH;
  const uint16_t *kb = P.k + W.row0 * P.ld_qkv + h * DH;
  const uint16_t *vb = P.v + W.row0 * P.ld_qkv + h * DH;
  const uint16_t *dob = P.dout + W.row0 * P.ld_o + h * DH;
  const int nkb = (L + BLK - 1) / BLK;
  const int qi = W.blk * BLK + 16 * wave + m;
  const bool active = W.blk * BLK + 16 * wave < L;
  const int qc = min(qi, L - 1);
  const size_t stat = ((size_t)W.b * P.H + h) * L;              // row of lse / delta

  BlockPair st;
  st.issue(kb, P.ld_qkv, vb, P.ld_qkv, 0, L);
  bf16x8 bq[2], bdo[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    bq[c] = as_frag(load_frag(qb, qc, P.ld_qkv, 32 * c + 8 * g));
    bdo[c] = as_frag(load_frag(dob, qc, P.ld_o, 32 * c + 8 * g));
  }
  const float lse2 = qi < L ? P.lse[stat + qc] * kLog2e : INFINITY;   // queries past L: p = 2^(x - inf) = 0
  unsigned int wraw[3];
  load_cond(P, W.row0, h, qc, wraw);
  Planes4 S[4];
  if (active)
#pragma unroll
    for (int j = 0; j < 4; ++j) load_planes4(P, W.b, qc, 16 * j + 4 * g, S[j]);
  st.commit(Kb, Vb);
  if (threadIdx.x < BLK) mbs[threadIdx.x] = key_term(P, W.row0, threadIdx.x);
  float w[6];
  cond_vector(wraw, w);
  __syncthreads();

  float delta = 0.f, dw[6];
#pragma unroll
  for (int d = 0; d < 6; ++d) dw[d] = 0.f;
  f32x4 o[4];                                                    // dQ^T strip = K^T dS^T
#pragma unroll
  for (int n = 0; n < 4; ++n) o[n] = zero_acc();

  // walk `it` < nkb: delta = rowsum(P dP);  walk `it` >= nkb: dS, dQ, d cond-vector.  The staging runs on across the
  // seam (the block after the last one of the first walk is block 0 again).
  for (int it = 0; it < 2 * nkb; ++it) {
    const int kbi = it < nkb ? it : it - nkb;
    const int nb = kbi + 1 < nkb ? kbi + 1 : 0;                  // block staged during this iteration
    const int cur = it & 1, nxt = cur ^ 1;
    const bool more = it + 1 < 2 * nkb;
    if (more) st.issue(kb, P.ld_qkv, vb, P.ld_qkv, nb * BLK, L);
    const float mnext = (more && threadIdx.x < BLK) ? key_term(P, W.row0, nb * BLK + threadIdx.x) : 0.f;
    if (active) {
      const uint16_t *Kc = Kb + cur * kTile, *Vc = Vb + cur * kTile;
      const float *mc = mbs + cur * BLK;
      if (it == nkb) delta = xor_sum_g(delta);                   // wave-uniform
      f32x4 s[4], dp[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        s[j] = zero_acc();
        dp[j] = zero_acc();
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const u32x4 a = *reinterpret_cast<const u32x4 *>(Kc + (16 * j + m) * KS + 32 * c + 8 * g);
          const u32x4 av = *reinterpret_cast<const u32x4 *>(Vc + (16 * j + m) * KS + 32 * c + 8 * g);
          s[j] = mfma32(as_frag(a), bq[c], s[j]);               // S^T
          dp[j] = mfma32(as_frag(av), bdo[c], dp[j]);           // (dO V^T)^T
        }
      }
      if (it < nkb) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const f32x4 kt = *reinterpret_cast<const f32x4 *>(mc + 16 * j + 4 * g);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float bias2 = spatial_bias2(__builtin_amdgcn_exp2f(spatial_u(S[j], w, r)));
            const float p = __builtin_amdgcn_exp2f(fmaf(s[j][r], kC, bias2 + kt[r]) - lse2);
            delta = fmaf(p, dp[j][r], delta);
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) load_planes4(P, W.b, qc, nb * BLK + 16 * j + 4 * g, S[j]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const f32x4 kt = *reinterpret_cast<const f32x4 *>(mc + 16 * j + 4 * g);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float e = __builtin_amdgcn_exp2f(spatial_u(S[j], w, r));
            const float ope = 1.f + e;
            const float bias2 = fmaxf(-__builtin_amdgcn_logf(ope), kClamp2);
            const float p = __builtin_amdgcn_exp2f(fmaf(s[j][r], kC, bias2 + kt[r]) - lse2);
            // d/dz log(clamp(sigmoid z, 1e-6)) = 1 - sigmoid z = e / (1 + e) where sigmoid z > 1e-6, else 0
            const float gate = ope < 1e6f ? e * __builtin_amdgcn_rcpf(ope) : 0.f;
            const float dl = p * (dp[j][r] - delta);             // d loss / d logit; the 1/8 goes onto dQ below
            const float dz = dl * gate;
            dw[0] += dz;
#pragma unroll
            for (int d = 0; d < 5; ++d) dw[1 + d] = fmaf((float)__builtin_bit_cast(f16x4, S[j].d[d])[r], dz, dw[1 + d]);
            s[j][r] = dl;
          }
        }
        if (more)
#pragma unroll
          for (int j = 0; j < 4; ++j) load_planes4(P, W.b, qc, nb * BLK + 16 * j + 4 * g, S[j]);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const bf16x8 db = pack_tiles(s[2 * c], s[2 * c + 1]);
#pragma unroll
          for (int n = 0; n < 4; ++n) o[n] = mfma32(tr_frag_perm(Kc, KS, c, 16 * n, lane), db, o[n]);
        }
      }
    }
    if (more) {
      st.commit(Kb + nxt * kTile, Vb + nxt * kTile);
      if (threadIdx.x < BLK) mbs[nxt * BLK + threadIdx.x] = mnext;
    }
    __syncthreads();
  }
  if (!active) return;
#pragma unroll
  for (int d = 0; d < 6; ++d) dw[d] = xor_sum_g(dw[d]);
  if (g == 0 && qi < L) {
    P.delta[stat + qi] = delta;
    unsigned int *wp = reinterpret_cast<unsigned int *>(P.dsw + (W.row0 + qi) * P.ld_dsw + h * 6);
    wp[0] = pack2(dw[0], dw[1]);
    wp[1] = pack2(dw[2], dw[3]);
    wp[2] = pack2(dw[4], dw[5]);
  }
  if (qi < L) {
    uint16_t *op = P.dq + (W.row0 + qi) * P.ld_dqkv + h * DH + 4 * g;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const u32x2 v = {pack2(o[n][0] * 0.125f, o[n][1] * 0.125f), pack2(o[n][2] * 0.125f, o[n][3] * 0.125f)};
      *reinterpret_cast<u32x2 *>(op + 16 * n) = v;
    }
  }
}

// ==========================================================================================
// backward, launch 2: workgroup = 64 keys -> dK, dV; query blocks (Q, dO, lse, delta) streamed
// ==========================================================================================
__global__ __launch_bounds__(kThreads) void bwd_dkv_kernel(const Params P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint16_t *Qb = reinterpret_cast<uint16_t *>(smem);            // [2][64][KS]
  uint16_t *Ob = Qb + 2 * kTile;                                 // [2][64][KS]  dO rows
  float *ls = reinterpret_cast<float *>(Ob + 2 * kTile);         // [2][64] log2(e) * lse (+inf past L)
  float *dl = ls + 2 * BLK;                                      // [2][64] delta
  uint16_t *park = reinterpret_cast<uint16_t *>(dl + 2 * BLK);   // per wave: P [64][TPK], dS [64][TPK]
  Work W;
  locate(P, W);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, g = lane >> 4;
  const int L = P.L, h = W.h;
  const uint16_t *qb = P.q + W.row0 * P.ld_qkv + h * DH;
  const uint16_t *kb = P.k + W.row0 * P.ld_qkv + h * DH;
  const uint16_t *vb = P.v + W.row0 * P.ld_qkv + h * DH;
  const uint16_t *dob = P.dout + W.row0 * P.ld_o + h * DH;
  const size_t stat = ((size_t)W.b * P.H + h) * L;
  const int nqb = (L + BLK - 1) / BLK;
  const int k0 = W.blk * BLK + 16 * wave;                        // first key of the wave's strip
  const bool active = k0 < L;                                    // wave-uniform
  const int t = k0 + m, tc = min(t, L - 1);                      // this lane's key of dK / dV (and of the K / V fragments)

  BlockPair st;
  st.issue(qb, P.ld_qkv, dob, P.ld_o, 0, L);
  bf16x8 bk[2], bv[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    bk[c] = as_frag(load_frag(kb, tc, P.ld_qkv, 32 * c + 8 * g));
    bv[c] = as_frag(load_frag(vb, tc, P.ld_qkv, 32 * c + 8 * g));
  }
  float kt[4];                                                   // key term of the score keys k0 + 4 g + r
#pragma unroll
  for (int r = 0; r < 4; ++r) kt[r] = key_term(P, W.row0, k0 + 4 * g + r);
  float l_next = INFINITY, d_next = 0.f;
  if (threadIdx.x < BLK && threadIdx.x < L) {
    l_next = P.lse[stat + threadIdx.x] * kLog2e;
    d_next = P.delta[stat + threadIdx.x];
  }
  // spatial operands of the query block being processed: query tile i -> query 16 i + m of the block
  Planes4 S[4];
  unsigned int wraw[4][3];
  if (active)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int qq = min(16 * i + m, L - 1);
      load_planes4(P, W.b, qq, k0 + 4 * g, S[i]);
      load_cond(P, W.row0, h, qq, wraw[i]);
    }
  st.commit(Qb, Ob);
  if (threadIdx.x < BLK) {
    ls[threadIdx.x] = l_next;
    dl[threadIdx.x] = d_next;
  }
  __syncthreads();

  uint16_t *PSw = park + wave * 2 * BLK * TPK, *DSw = PSw + BLK * TPK;
  f32x4 dk[4], dv[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    dk[n] = zero_acc();
    dv[n] = zero_acc();
  }
  for (int qbi = 0; qbi < nqb; ++qbi) {
    const int cur = qbi & 1, nxt = cur ^ 1;
    const bool more = qbi + 1 < nqb;
    if (more) {
      st.issue(qb, P.ld_qkv, dob, P.ld_o, (qbi + 1) * BLK, L);
      const int qn = (qbi + 1) * BLK + threadIdx.x;
      l_next = INFINITY;
      d_next = 0.f;
      if (threadIdx.x < BLK && qn < L) {
        l_next = P.lse[stat + qn] * kLog2e;
        d_next = P.delta[stat + qn];
      }
    }
    if (active) {
      const uint16_t *Qc = Qb + cur * kTile, *Oc = Ob + cur * kTile;
      const float *lc = ls + cur * BLK, *dc = dl + cur * BLK;
      // S^T[key k0 + 4 g + r][query 16 i + m] and (dO V^T)^T: the wave's K / V rows are the A operands
      f32x4 s[4], dp[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        s[i] = zero_acc();
        dp[i] = zero_acc();
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const u32x4 vq = *reinterpret_cast<const u32x4 *>(Qc + (16 * i + m) * KS + 32 * c + 8 * g);
          const u32x4 vo = *reinterpret_cast<const u32x4 *>(Oc + (16 * i + m) * KS + 32 * c + 8 * g);
          s[i] = mfma32(bk[c], as_frag(vq), s[i]);
          dp[i] = mfma32(bv[c], as_frag(vo), dp[i]);
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float w[6];
        cond_vector(wraw[i], w);
        const float lq = lc[16 * i + m], dq = dc[16 * i + m];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float bias2 = spatial_bias2(__builtin_amdgcn_exp2f(spatial_u(S[i], w, r)));
          const float p = __builtin_amdgcn_exp2f(fmaf(s[i][r], kC, bias2 + kt[r]) - lq);
          dp[i][r] = p * (dp[i][r] - dq);                        // dS; 1/8 goes onto dK below
          s[i][r] = p;
        }
        // P[query][key] and dS[query][key] rows of this wave: one 8-byte write each
        *reinterpret_cast<u32x2 *>(PSw + (16 * i + m) * TPK + 4 * g) = pack_tile(s[i]);
        *reinterpret_cast<u32x2 *>(DSw + (16 * i + m) * TPK + 4 * g) = pack_tile(dp[i]);
      }
      if (more)                                                  // the next query block's spatial operands
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int qq = min((qbi + 1) * BLK + 16 * i + m, L - 1);
          load_planes4(P, W.b, qq, k0 + 4 * g, S[i]);
          load_cond(P, W.row0, h, qq, wraw[i]);
        }
      // dV^T += dO^T P, dK^T += Q^T dS over the block's 64 queries: the parked rows read back transposed (written by this
      // wave: LDS operations of a wave complete in order)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const bf16x8 bp = tr_frag_nat(PSw, TPK, c, 0, lane);    // P[queries 32 c + 8 g + 0..7][key k0 + m]
        const bf16x8 bs = tr_frag_nat(DSw, TPK, c, 0, lane);
#pragma unroll
        for (int n = 0; n < 4; ++n) {
          dv[n] = mfma32(tr_frag_nat(Oc, KS, c, 16 * n, lane), bp, dv[n]);
          dk[n] = mfma32(tr_frag_nat(Qc, KS, c, 16 * n, lane), bs, dk[n]);
        }
      }
    }
    if (more) {
      st.commit(Qb + nxt * kTile, Ob + nxt * kTile);
      if (threadIdx.x < BLK) {
        ls[nxt * BLK + threadIdx.x] = l_next;
        dl[nxt * BLK + threadIdx.x] = d_next;
      }
    }
    __syncthreads();
  }
  if (active && t < L) {                         // dk[n][r] = dK[key t][d = 16 n + 4 g + r]
    uint16_t *pk = P.dk + (W.row0 + t) * P.ld_dqkv + h * DH + 4 * g;
    uint16_t *pv = P.dv + (W.row0 + t) * P.ld_dqkv + h * DH + 4 * g;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const u32x2 vk = {pack2(dk[n][0] * 0.125f, dk[n][1] * 0.125f), pack2(dk[n][2] * 0.125f, dk[n][3] * 0.125f)};
      const u32x2 vv = {pack2(dv[n][0], dv[n][1]), pack2(dv[n][2], dv[n][3])};
      *reinterpret_cast<u32x2 *>(pk + 16 * n) = vk;
      *reinterpret_cast<u32x2 *>(pv + 16 * n) = vv;
    }
  }
}

}  // namespace gps_attn_spl

namespace gps_attn {

// the plane form above 144 rows (gps_attention_sp.hip run_spatial_planes has checked the arguments): Lq == Lk in
// 145 .. 512; the backward call needs gps_attn_args.delta_ws (B, H, L) fp32
int run_spatial_planes_long(const gps_attn_args *a, bool backward, hipStream_t s) {
  using namespace gps_attn_spl;
  if (a->Lk > 512 || a->Lk < 1) return GPS_ERR_UNSUPPORTED;
  if (backward && !a->delta_ws) return GPS_ERR_INVALID_ARGUMENT;
  Params P = {};
  P.B = a->B; P.H = a->H; P.L = a->Lk; P.nblk = (a->Lk + BLK - 1) / BLK;
  P.ld_qkv = a->ld_kv; P.ld_o = a->ld_o; P.ld_pl = a->ld_pl; P.ld_sw = a->ld_sw;
  P.q = (const uint16_t *)a->q; P.k = (const uint16_t *)a->k; P.v = (const uint16_t *)a->v;
  P.pl = (const _Float16 *)a->pl_planes; P.sw = (const uint16_t *)a->sw16; P.mask = a->mask;
  P.out = (uint16_t *)a->out; P.lse = a->lse;
  const dim3 grid(P.B * P.H * P.nblk), block(kThreads);
  if (!backward) {
    hipLaunchKernelGGL(fwd_kernel, grid, block, kLdsQ, s, P);
    return hipGetLastError() == hipSuccess ? GPS_OK : GPS_ERR_LAUNCH;
  }
  P.dout = (const uint16_t *)a->dout; P.dq = (uint16_t *)a->dq; P.dk = (uint16_t *)a->dk; P.dv = (uint16_t *)a->dv;
  P.ld_dqkv = a->ld_dq; P.dsw = (uint16_t *)a->dsw16; P.ld_dsw = a->ld_dsw; P.delta = a->delta_ws;
  hipLaunchKernelGGL(bwd_dq_kernel, grid, block, kLdsQ, s, P);
  if (hipGetLastError() != hipSuccess) return GPS_ERR_LAUNCH;
  hipLaunchKernelGGL(bwd_dkv_kernel, grid, block, kLdsKv, s, P);
  return hipGetLastError() == hipSuccess ? GPS_OK : GPS_ERR_LAUNCH;
}

}  // namespace gps_attn
