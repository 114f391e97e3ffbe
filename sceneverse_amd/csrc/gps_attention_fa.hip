// gps_attention_fa.hip -- the PLAIN attention core (no pairwise term) in block-streaming form, round 5: every text layer
// of BERT (variable-length sentences and captions packed back to back), the joint text + object layers of the unified
// encoder (130 tokens, key-padding mask), cross-attention.  Reference behaviour: nn.MultiheadAttention with
// key_padding_mask and dropout on the probabilities (modules/layers/transformers.py:141; HF BertSelfAttention for the
// text encoder, modules/language/bert.py:21-26).
//
// Why a second streaming family (gps_attention.hip has one): that one gives a workgroup a whole (sequence, head) and
// keeps the sequence's K and V resident in LDS -- 92 KB at 300 tokens, sized for the LONGEST sequence of the launch, one
// workgroup per CU.  A 30-token sentence then occupies a CU like a 300-token caption does, nothing overlaps a workgroup's
// staging round trip, and the two-pass softmax evaluates every score twice.  Here:
//   * a workgroup (4 waves) owns 64 queries (forward, dQ) or 64 keys (dK / dV) of one (sequence, head) and streams the
//     other side through LDS in 64-row blocks, double-buffered: 37 KB whatever the sequence length -> 4 workgroups per CU,
//     work proportional to the sequence's own length (blocks past its end exit at once);
//   * online softmax (running maximum and normaliser per query, lane-local: scores are computed transposed, S^T = K Q^T,
//     so a lane owns one query): every score is evaluated once in the forward pass;
//   * the backward pass is two launches -- dQ per query block (also writes delta = rowsum(dO * O) per query), dK / dV per
//     key block (reads it) -- each with the 64-row blocks of the other side streamed the same way;
//   * results leave in the transposed orientation (O^T = V^T P^T, dQ^T = K^T dS^T, dV^T = dO^T P, dK^T = Q^T dS): 8-byte
//     stores, lane-local normalisation; "column" operands are hardware-transposed LDS reads (ds_read_b64_tr_b16).
// Same dropout stream (one hash per (query, key pair), 16-bit thresholds), same lse, same argument conventions as the
// streaming kernels of gps_attention.hip: forward and backward of the two families can be mixed (tests do).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "gps_hip.h"
#include "gps_attention_dev.h"
#include "gps_attention_run.h"
#include "gps_device_flags.h"
#include "gps_dropout.h"

namespace gps_attn_fa {

using namespace gps_attn_dev;
using namespace gps_dropout;

constexpr int BLK = 64;               // rows per streamed block, and queries / keys per workgroup
constexpr int kThreads = kStreamThreads;

struct Params {
  int B, H, L, Lq;                    // L / Lq: capacities of keys / queries (pitch of lse, delta and of the dropout counter)
  int ld_q, ld_kv, ld_o, ld_dq, ld_dkv;
  int nblk;                           // blocks of the OWNED side per sequence: ceil(capacity / 64)
  const uint16_t *q, *k, *v;
  const uint8_t *mask;
  uint16_t *out;
  float *lse;
  const uint16_t *dout;
  uint16_t *dq, *dk, *dv;
  float *delta;                       // (B, H, Lq) workspace: written by the dQ launch, read by the dK / dV launch
  float p_drop;
  unsigned int drop_thr;
  unsigned long long seed;
  const unsigned long long *seed_dev;
  const int *seq_order, *q_limit, *cu_rows;
};

// which (sequence, head, block) a workgroup owns: the blocks of one (sequence, head) -- which re-read the same K / V (or
// Q / dO) rows -- sit on ONE XCD (block id mod 8) and share its L2
struct Work {
  int b, h, blk;
  int L, Lq;                  // this sequence's keys / computed queries
  size_t row0, row0q;
};
__device__ __forceinline__ bool locate(const Params &P, Work &W) {
  const int id = blockIdx.x, units = P.B * P.H;
  int u, blk;
  if ((units & 7) == 0) {
    const int xcd = id & 7, slot = id >> 3;
    u = (slot / P.nblk) * 8 + xcd;
    blk = slot % P.nblk;
  } else {
    u = id / P.nblk;
    blk = id % P.nblk;
  }
  int b = u / P.H;
  W.h = u % P.H;
  if (P.seq_order) b = P.seq_order[b];
  W.b = b;
  W.blk = blk;
  W.L = P.L;
  W.Lq = P.Lq;
  W.row0 = (size_t)b * P.L;
  W.row0q = (size_t)b * P.Lq;
  if (P.cu_rows) {                                            // packed variable-length sequences
    W.row0 = W.row0q = (size_t)P.cu_rows[b];
    W.L = W.Lq = P.cu_rows[b + 1] - P.cu_rows[b];
    if (W.L <= 0) return false;
    if (P.q_limit) W.Lq = min(W.Lq, max(P.q_limit[b], 0));    // only the leading queries are wanted
  }
  return true;
}

constexpr int kTile = BLK * KS;           // elements of one LDS tile
constexpr size_t kLdsFwd = (size_t)4 * kTile * 2 + 2 * BLK * 4;              // K, V double-buffered + key terms
constexpr size_t kLdsDkv = (size_t)4 * kTile * 2 + 2 * 2 * BLK * 4;          // Q, dO double-buffered + lse2, delta

// ==========================================================================================
// forward: workgroup = 64 queries of one (sequence, head); key blocks streamed
// ==========================================================================================
__global__ __launch_bounds__(kThreads) void fwd_kernel(const Params P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint16_t *Kb = reinterpret_cast<uint16_t *>(smem);            // [2][64][KS]
  uint16_t *Vb = Kb + 2 * kTile;                                 // [2][64][KS]
  float *mbs = reinterpret_cast<float *>(Vb + 2 * kTile);        // [2][64] additive key term (base 2): 0 or -inf
  Work W;
  if (!locate(P, W)) return;
  if (W.blk * BLK >= W.Lq) return;                               // workgroup-uniform: no query of this block exists
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, g = lane >> 4;
  const int L = W.L, Lq = W.Lq, h = W.h;
  const uint16_t *qb = P.q + W.row0q * P.ld_q + h * DH;
  const uint16_t *kb = P.k + W.row0 * P.ld_kv + h * DH;
  const uint16_t *vb = P.v + W.row0 * P.ld_kv + h * DH;
  const int nkb = (L + BLK - 1) / BLK;
  const int qi = W.blk * BLK + 16 * wave + m;                    // this lane's query
  const bool active = W.blk * BLK + 16 * wave < Lq;              // wave-uniform: the strip has at least one query
  const int qc = min(qi, Lq - 1);

  BlockPair st;
  st.issue(kb, P.ld_kv, vb, P.ld_kv, 0, L);
  bf16x8 bq[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) bq[c] = as_frag(load_frag(qb, qc, P.ld_q, 32 * c + 8 * g));
  st.commit(Kb, Vb);
  if (threadIdx.x < BLK) mbs[threadIdx.x] = (threadIdx.x < L && !(P.mask && P.mask[W.row0 + threadIdx.x])) ? 0.f : -INFINITY;
  __syncthreads();

  const bool dropout = P.drop_thr != 0u;
  const float keep_scale = dropout ? 1.f / (1.f - P.p_drop) : 1.f;
  const unsigned int seedmix = dropout ? seed_fold(effective_seed(P.seed, P.seed_dev)) : 0u;
  const unsigned int thr16 = P.drop_thr >> 16;
  const unsigned int rp = (((unsigned int)W.b * P.H + h) * P.Lq + qi) * (unsigned int)((P.L + 1) >> 1);

  float m_run = -INFINITY, l_run = 0.f;                          // running maximum (base-2 logits) and this lane's part of the normaliser
  f32x4 o[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) o[n] = zero_acc();

  for (int kbi = 0; kbi < nkb; ++kbi) {
    const int cur = kbi & 1, nxt = cur ^ 1;
    const bool more = kbi + 1 < nkb;
    if (more) st.issue(kb, P.ld_kv, vb, P.ld_kv, (kbi + 1) * BLK, L);
    float mnext = 0.f;
    if (more && threadIdx.x < BLK) {
      const int t = (kbi + 1) * BLK + threadIdx.x;
      mnext = (t < L && !(P.mask && P.mask[W.row0 + t])) ? 0.f : -INFINITY;
    }
    if (active) {
      const uint16_t *Kc = Kb + cur * kTile, *Vc = Vb + cur * kTile;
      const float *mc = mbs + cur * BLK;
      f32x4 x[4];
      float bmax = -INFINITY;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f32x4 acc = zero_acc();
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const u32x4 a = *reinterpret_cast<const u32x4 *>(Kc + (16 * j + m) * KS + 32 * c + 8 * g);
          acc = mfma32(as_frag(a), bq[c], acc);
        }
        const f32x4 kt = *reinterpret_cast<const f32x4 *>(mc + 16 * j + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) x[j][r] = fmaf(acc[r], kC, kt[r]);
        bmax = fmaxf(fmaxf(bmax, fmaxf(x[j][0], x[j][1])), fmaxf(x[j][2], x[j][3]));
      }
      bmax = xor_max_g(bmax);
      const float m_new = fmaxf(m_run, bmax);
      const float m_use = m_new == -INFINITY ? 0.f : m_new;      // every key so far masked: keep the arithmetic finite
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);
      m_run = m_new;
      float psum = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          x[j][r] = __builtin_amdgcn_exp2f(x[j][r] - m_use);
          psum += x[j][r];
        }
        if (dropout) {            // keys 16 j + 4 g + {0,1} and {2,3} of the block: two hashes for the four elements
          const int t0 = kbi * BLK + 16 * j + 4 * g;
          const unsigned int r01 = pair_rng(seedmix, rp, t0), r23 = pair_rng(seedmix, rp, t0 + 2);
          x[j][0] = (r01 & 0xFFFFu) >= thr16 ? x[j][0] : 0.f;
          x[j][1] = (r01 >> 16) >= thr16 ? x[j][1] : 0.f;
          x[j][2] = (r23 & 0xFFFFu) >= thr16 ? x[j][2] : 0.f;
          x[j][3] = (r23 >> 16) >= thr16 ? x[j][3] : 0.f;
        }
      }
      l_run = fmaf(l_run, alpha, psum);
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) o[n][r] *= alpha;
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
  const float lsum = xor_sum_g(l_run);                           // all keys masked -> 0 -> NaN row, like torch
  if (g == 0 && qi < Lq) P.lse[((size_t)W.b * P.H + h) * P.Lq + qi] = (m_run + __builtin_amdgcn_logf(lsum)) * kLn2;
  const float sc = keep_scale / lsum;
  if (qi < Lq) {
    uint16_t *op = P.out + (W.row0q + qi) * P.ld_o + h * DH + 4 * g;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const u32x2 v = {pack2(o[n][0] * sc, o[n][1] * sc), pack2(o[n][2] * sc, o[n][3] * sc)};
      *reinterpret_cast<u32x2 *>(op + 16 * n) = v;
    }
  }
}

// ==========================================================================================
// backward, launch 1: workgroup = 64 queries -> dQ (and delta per query); key blocks streamed
// ==========================================================================================
__global__ __launch_bounds__(kThreads) void bwd_dq_kernel(const Params P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint16_t *Kb = reinterpret_cast<uint16_t *>(smem);
  uint16_t *Vb = Kb + 2 * kTile;
  float *mbs = reinterpret_cast<float *>(Vb + 2 * kTile);
  Work W;
  if (!locate(P, W)) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, g = lane >> 4;
  const int L = W.L, Lq = W.Lq, h = W.h;
  if (W.blk * BLK >= Lq) {
    // queries of the sequence that were not computed (q_limit): their dQ rows are zero
    if (P.q_limit && P.cu_rows && W.blk * BLK < L) {
      for (int e = threadIdx.x; e < BLK * 8; e += kThreads) {
        const int qr = W.blk * BLK + (e >> 3);
        if (qr < L) *reinterpret_cast<u32x4 *>(P.dq + (W.row0q + qr) * P.ld_dq + h * DH + 8 * (e & 7)) = zero4();
      }
    }
    return;
  }
  const uint16_t *qb = P.q + W.row0q * P.ld_q + h * DH;
  const uint16_t *kb = P.k + W.row0 * P.ld_kv + h * DH;
  const uint16_t *vb = P.v + W.row0 * P.ld_kv + h * DH;
  const uint16_t *dob = P.dout + W.row0q * P.ld_o + h * DH;
  const uint16_t *ob = P.out + W.row0q * P.ld_o + h * DH;
  const int nkb = (L + BLK - 1) / BLK;
  const int qi = W.blk * BLK + 16 * wave + m;
  const bool active = W.blk * BLK + 16 * wave < Lq;
  const int qc = min(qi, Lq - 1);

  BlockPair st;
  st.issue(kb, P.ld_kv, vb, P.ld_kv, 0, L);
  bf16x8 bq[2], bdo[2];
  u32x4 ov[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    bq[c] = as_frag(load_frag(qb, qc, P.ld_q, 32 * c + 8 * g));
    bdo[c] = as_frag(qi < Lq ? load_frag(dob, qc, P.ld_o, 32 * c + 8 * g) : zero4());
    ov[c] = load_frag(ob, qc, P.ld_o, 32 * c + 8 * g);
  }
  const size_t stat = ((size_t)W.b * P.H + h) * P.Lq;            // row of lse / delta
  float lse2 = qi < Lq ? P.lse[stat + qc] : INFINITY;            // queries past Lq: p = 2^(x - inf) = 0
  st.commit(Kb, Vb);
  if (threadIdx.x < BLK) mbs[threadIdx.x] = (threadIdx.x < L && !(P.mask && P.mask[W.row0 + threadIdx.x])) ? 0.f : -INFINITY;
  // delta = sum_d dO[q][d] O[q][d] = rowsum(P' dP') for the dropped, rescaled probabilities of the forward pass
  float delta = 0.f;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const u32x4 dv = __builtin_bit_cast(u32x4, bdo[c]);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      delta = fmaf(bf2f(dv[e] & 0xFFFFu), bf2f(ov[c][e] & 0xFFFFu), delta);
      delta = fmaf(__uint_as_float(dv[e] & 0xFFFF0000u), __uint_as_float(ov[c][e] & 0xFFFF0000u), delta);
    }
  }
  delta = xor_sum_g(delta);
  lse2 *= kLog2e;
  if (g == 0 && qi < Lq && P.delta) P.delta[stat + qi] = delta;
  __syncthreads();

  const bool dropout = P.drop_thr != 0u;
  const float keep_scale = dropout ? 1.f / (1.f - P.p_drop) : 1.f;
  const unsigned int seedmix = dropout ? seed_fold(effective_seed(P.seed, P.seed_dev)) : 0u;
  const unsigned int thr16 = P.drop_thr >> 16;
  const unsigned int rp = (((unsigned int)W.b * P.H + h) * P.Lq + qi) * (unsigned int)((P.L + 1) >> 1);

  f32x4 o[4];                                                    // dQ^T strip = K^T dS^T
#pragma unroll
  for (int n = 0; n < 4; ++n) o[n] = zero_acc();
  for (int kbi = 0; kbi < nkb; ++kbi) {
    const int cur = kbi & 1, nxt = cur ^ 1;
    const bool more = kbi + 1 < nkb;
    if (more) st.issue(kb, P.ld_kv, vb, P.ld_kv, (kbi + 1) * BLK, L);
    float mnext = 0.f;
    if (more && threadIdx.x < BLK) {
      const int t = (kbi + 1) * BLK + threadIdx.x;
      mnext = (t < L && !(P.mask && P.mask[W.row0 + t])) ? 0.f : -INFINITY;
    }
    if (active) {
      const uint16_t *Kc = Kb + cur * kTile, *Vc = Vb + cur * kTile;
      const float *mc = mbs + cur * BLK;
      f32x4 ds[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f32x4 acc = zero_acc(), dacc = zero_acc();
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const u32x4 a = *reinterpret_cast<const u32x4 *>(Kc + (16 * j + m) * KS + 32 * c + 8 * g);
          const u32x4 av = *reinterpret_cast<const u32x4 *>(Vc + (16 * j + m) * KS + 32 * c + 8 * g);
          acc = mfma32(as_frag(a), bq[c], acc);            // S^T
          dacc = mfma32(as_frag(av), bdo[c], dacc);        // (dO V^T)^T
        }
        const f32x4 kt = *reinterpret_cast<const f32x4 *>(mc + 16 * j + 4 * g);
        if (dropout) {
          const int t0 = kbi * BLK + 16 * j + 4 * g;
          const unsigned int r01 = pair_rng(seedmix, rp, t0), r23 = pair_rng(seedmix, rp, t0 + 2);
          dacc[0] = (r01 & 0xFFFFu) >= thr16 ? dacc[0] : 0.f;    // dropped gradient, before its 1 / (1 - p) scale
          dacc[1] = (r01 >> 16) >= thr16 ? dacc[1] : 0.f;
          dacc[2] = (r23 & 0xFFFFu) >= thr16 ? dacc[2] : 0.f;
          dacc[3] = (r23 >> 16) >= thr16 ? dacc[3] : 0.f;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = __builtin_amdgcn_exp2f(fmaf(acc[r], kC, kt[r]) - lse2);
          ds[j][r] = p * fmaf(dacc[r], keep_scale, -delta);      // the 1/8 of the logits goes onto dQ below
        }
      }
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const bf16x8 db = pack_tiles(ds[2 * c], ds[2 * c + 1]);
#pragma unroll
        for (int n = 0; n < 4; ++n) o[n] = mfma32(tr_frag_perm(Kc, KS, c, 16 * n, lane), db, o[n]);
      }
    }
    if (more) {
      st.commit(Kb + nxt * kTile, Vb + nxt * kTile);
      if (threadIdx.x < BLK) mbs[nxt * BLK + threadIdx.x] = mnext;
    }
    __syncthreads();
  }
  if (active && qi < Lq) {
    uint16_t *op = P.dq + (W.row0q + qi) * P.ld_dq + h * DH + 4 * g;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const u32x2 v = {pack2(o[n][0] * 0.125f, o[n][1] * 0.125f), pack2(o[n][2] * 0.125f, o[n][3] * 0.125f)};
      *reinterpret_cast<u32x2 *>(op + 16 * n) = v;
    }
  }
  if (P.q_limit && P.cu_rows && Lq < L) {     // the uncomputed queries that share this block with computed ones
    for (int e = threadIdx.x; e < BLK * 8; e += kThreads) {
      const int qr = W.blk * BLK + (e >> 3);
      if (qr >= Lq && qr < L) *reinterpret_cast<u32x4 *>(P.dq + (W.row0q + qr) * P.ld_dq + h * DH + 8 * (e & 7)) = zero4();
    }
  }
}

// ==========================================================================================
// backward, launch 2: workgroup = 64 keys -> dK, dV; query blocks (Q, dO, lse, delta) streamed
// ==========================================================================================
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(3, 3))) void bwd_dkv_kernel(const Params P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint16_t *Qb = reinterpret_cast<uint16_t *>(smem);            // [2][64][KS]
  uint16_t *Ob = Qb + 2 * kTile;                                 // [2][64][KS]  dO rows
  float *ls = reinterpret_cast<float *>(Ob + 2 * kTile);         // [2][64] log2(e) * lse (+inf past Lq)
  float *dl = ls + 2 * BLK;                                      // [2][64] delta
  Work W;
  if (!locate(P, W)) return;
  const int L = W.L, Lq = W.Lq, h = W.h;
  if (W.blk * BLK >= L) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, g = lane >> 4;
  const uint16_t *qb = P.q + W.row0q * P.ld_q + h * DH;
  const uint16_t *kb = P.k + W.row0 * P.ld_kv + h * DH;
  const uint16_t *vb = P.v + W.row0 * P.ld_kv + h * DH;
  const uint16_t *dob = P.dout + W.row0q * P.ld_o + h * DH;
  const size_t stat = ((size_t)W.b * P.H + h) * P.Lq;
  const int nqb = (Lq + BLK - 1) / BLK;
  const int t = W.blk * BLK + 16 * wave + m;                     // this lane's key
  const bool active = W.blk * BLK + 16 * wave < L;
  const int tc = min(t, L - 1);

  BlockPair st;
  st.issue(qb, P.ld_q, dob, P.ld_o, 0, Lq);
  bf16x8 bk[2], bv[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    bk[c] = as_frag(load_frag(kb, tc, P.ld_kv, 32 * c + 8 * g));
    bv[c] = as_frag(load_frag(vb, tc, P.ld_kv, 32 * c + 8 * g));
  }
  const float kt = (t < L && !(P.mask && P.mask[W.row0 + tc])) ? 0.f : -INFINITY;
  float l_next = INFINITY, d_next = 0.f;
  if (threadIdx.x < BLK && threadIdx.x < Lq) {
    l_next = P.lse[stat + threadIdx.x] * kLog2e;
    d_next = P.delta[stat + threadIdx.x];
  }
  st.commit(Qb, Ob);
  if (threadIdx.x < BLK) {
    ls[threadIdx.x] = l_next;
    dl[threadIdx.x] = d_next;
  }
  __syncthreads();

  const bool dropout = P.drop_thr != 0u;
  const float keep_scale = dropout ? 1.f / (1.f - P.p_drop) : 1.f;
  const unsigned int seedmix = dropout ? seed_fold(effective_seed(P.seed, P.seed_dev)) : 0u;
  const unsigned int thr16 = P.drop_thr >> 16;
  const unsigned int pitch2 = (unsigned int)((P.L + 1) >> 1);
  const unsigned int bh_base = ((unsigned int)W.b * P.H + h) * P.Lq;

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
      st.issue(qb, P.ld_q, dob, P.ld_o, (qbi + 1) * BLK, Lq);
      const int qn = (qbi + 1) * BLK + threadIdx.x;
      l_next = INFINITY;
      d_next = 0.f;
      if (threadIdx.x < BLK && qn < Lq) {
        l_next = P.lse[stat + qn] * kLog2e;
        d_next = P.delta[stat + qn];
      }
    }
    if (active) {
      const uint16_t *Qc = Qb + cur * kTile, *Oc = Ob + cur * kTile;
      const float *lc = ls + cur * BLK, *dc = dl + cur * BLK;
      // 32 queries at a time: scores, dP, probabilities and dS of two query tiles, then their share of dV^T += dO^T P and
      // dK^T += Q^T dS (reduction over those 32 queries, in the order pack_tiles lays them out) -- two tiles of P / dS
      // live at once, not four (registers: three waves per SIMD)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        f32x4 pt[2], ds[2];
#pragma unroll
        for (int ii = 0; ii < 2; ++ii) {
          const int i = 2 * c + ii;            // query tile of the block
          f32x4 sacc = zero_acc(), dacc = zero_acc();
#pragma unroll
          for (int cc = 0; cc < 2; ++cc) {
            const u32x4 vq = *reinterpret_cast<const u32x4 *>(Qc + (16 * i + m) * KS + 32 * cc + 8 * g);
            const u32x4 vo = *reinterpret_cast<const u32x4 *>(Oc + (16 * i + m) * KS + 32 * cc + 8 * g);
            sacc = mfma32(as_frag(vq), bk[cc], sacc);       // S[query 16 i + 4 g + r][key t]
            dacc = mfma32(as_frag(vo), bv[cc], dacc);       // dO V^T
          }
          const f32x4 lq = *reinterpret_cast<const f32x4 *>(lc + 16 * i + 4 * g);
          const f32x4 dq4 = *reinterpret_cast<const f32x4 *>(dc + 16 * i + 4 * g);
          bool keep[4] = {true, true, true, true};
          if (dropout) {
            // hashes of (query q0 + r, key pair t >> 1): this lane computes two of the four, the lane of the other key of
            // the pair (m ^ 1) the other two
            const int q0 = qbi * BLK + 16 * i + 4 * g, par = m & 1;
            const unsigned int qa = (unsigned int)(q0 + 2 * par);
            const unsigned int ha = pair_rng(seedmix, (bh_base + qa) * pitch2, t);
            const unsigned int hb = pair_rng(seedmix, (bh_base + qa + 1u) * pitch2, t);
            const unsigned int oa = (unsigned int)__shfl_xor((int)ha, 1, 64), ob2 = (unsigned int)__shfl_xor((int)hb, 1, 64);
            const unsigned int hr0 = par ? oa : ha, hr1 = par ? ob2 : hb, hr2 = par ? ha : oa, hr3 = par ? hb : ob2;
            const unsigned int sh = par ? 16u : 0u;
            keep[0] = ((hr0 >> sh) & 0xFFFFu) >= thr16;
            keep[1] = ((hr1 >> sh) & 0xFFFFu) >= thr16;
            keep[2] = ((hr2 >> sh) & 0xFFFFu) >= thr16;
            keep[3] = ((hr3 >> sh) & 0xFFFFu) >= thr16;
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float p = __builtin_amdgcn_exp2f(fmaf(sacc[r], kC, kt) - lq[r]);
            const float dp = keep[r] ? dacc[r] : 0.f;
            pt[ii][r] = keep[r] ? p : 0.f;                                  // 1 / (1 - p) goes onto dV below
            ds[ii][r] = p * fmaf(dp, keep_scale, -dq4[r]);                  // 1/8 goes onto dK below
          }
        }
        const bf16x8 pb = pack_tiles(pt[0], pt[1]);
        const bf16x8 db = pack_tiles(ds[0], ds[1]);
#pragma unroll
        for (int n = 0; n < 4; ++n) {
          dv[n] = mfma32(tr_frag_perm(Oc, KS, c, 16 * n, lane), pb, dv[n]);
          dk[n] = mfma32(tr_frag_perm(Qc, KS, c, 16 * n, lane), db, dk[n]);
        }
        __builtin_amdgcn_sched_barrier(0);
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
  if (active && t < L) {
    uint16_t *pk = P.dk + (W.row0 + t) * P.ld_dkv + h * DH + 4 * g;
    uint16_t *pv = P.dv + (W.row0 + t) * P.ld_dkv + h * DH + 4 * g;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const u32x2 vk = {pack2(dk[n][0] * 0.125f, dk[n][1] * 0.125f), pack2(dk[n][2] * 0.125f, dk[n][3] * 0.125f)};
      const u32x2 vv = {pack2(dv[n][0] * keep_scale, dv[n][1] * keep_scale), pack2(dv[n][2] * keep_scale, dv[n][3] * keep_scale)};
      *reinterpret_cast<u32x2 *>(pk + 16 * n) = vk;
      *reinterpret_cast<u32x2 *>(pv + 16 * n) = vv;
    }
  }
}

// ==========================================================================================
// backward in ONE launch (self-attention, capacity <= 320): workgroup = one whole (sequence, head); key blocks j outer,
// query blocks i inner; every (query, key) element -- S, dO V^T, P, dS, its dropout hash -- is formed ONCE, five products.
//   role A (key strip, the body of bwd_dkv_kernel): wave w owns keys 16 w .. 16 w + 15 of block j, K / V fragments in
//     registers; S and dO V^T of the 64 queries of block i, P, dS; dV^T += dO^T P, dK^T += Q^T dS in registers;
//   hand-over: dS parked in bf16 in an LDS tile [key][query] (8-byte stores), K_j row-major in LDS; one barrier;
//   role B (query strip): wave w owns queries 16 w .. 16 w + 15 of EVERY query block and adds K_j^T dS^T to the dQ^T
//     accumulators of block i -- both operands hardware-transposed reads in the key order of pack_tiles.  The dQ^T
//     accumulators of all NQB query blocks stay in registers: the loop over i is a run-time loop (unrolled, the compiler
//     peels and hoists across the copies and spills at NQB = 5) and only the dQ^T MFMAs are selected by uniform branches.
// delta = rowsum(dO * O) is formed in the prologue (expression and element order of attn_bwd_stream_kernel) and kept in
// LDS beside log2(e) lse: no workspace, no atomics, no word that outlives the launch; fixed summation order.
// ==========================================================================================
constexpr int kFusedMaxCap = 320;
constexpr size_t lds_fused(int nqb) { return (size_t)7 * kTile * 2 + (size_t)2 * nqb * BLK * 4; }   // Q, dO x2 | K | dS x2 | lse2, delta

template <int NQB, bool DROPOUT>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2))) void bwd_fused_kernel(const Params P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint16_t *Qb = reinterpret_cast<uint16_t *>(smem);            // [2][64][KS]
  uint16_t *Ob = Qb + 2 * kTile;                                 // [2][64][KS]  dO rows
  uint16_t *Kt = Ob + 2 * kTile;                                 // [64][KS]     K rows of block j
  uint16_t *Ds = Kt + kTile;                                     // [2][64 keys][KS] parked dS, [key][query]
  float *ls = reinterpret_cast<float *>(Ds + 2 * kTile);         // [NQB * 64] log2(e) * lse (+inf past Lq)
  float *dl = ls + NQB * BLK;                                    // [NQB * 64] delta
  Work W;
  if (!locate(P, W)) return;
  const int L = W.L, Lq = W.Lq, h = W.h;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, g = lane >> 4;
  const uint16_t *qb = P.q + W.row0q * P.ld_q + h * DH;
  const uint16_t *kb = P.k + W.row0 * P.ld_kv + h * DH;
  const uint16_t *vb = P.v + W.row0 * P.ld_kv + h * DH;
  const uint16_t *dob = P.dout + W.row0q * P.ld_o + h * DH;
  const uint16_t *ob = P.out + W.row0q * P.ld_o + h * DH;
  const size_t stat = ((size_t)W.b * P.H + h) * P.Lq;
  const int nkb = (L + BLK - 1) / BLK;
  const int nqb = min((Lq + BLK - 1) / BLK, NQB);

  BlockPair st;
  if (nqb > 0) st.issue(qb, P.ld_q, dob, P.ld_o, 0, Lq);
  // delta[q] = sum_d dO[q][d] O[q][d]: one lane per query, the 64 terms in order
  for (int t = threadIdx.x; t < NQB * BLK; t += kThreads) {
    float d = 0.f;
    if (t < Lq) {
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const u32x4 a = *reinterpret_cast<const u32x4 *>(dob + (size_t)t * P.ld_o + 8 * c);
        const u32x4 o = *reinterpret_cast<const u32x4 *>(ob + (size_t)t * P.ld_o + 8 * c);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          d = fmaf(__uint_as_float(a[e] << 16), __uint_as_float(o[e] << 16), d);
          d = fmaf(__uint_as_float(a[e] & 0xFFFF0000u), __uint_as_float(o[e] & 0xFFFF0000u), d);
        }
      }
    }
    dl[t] = d;
    ls[t] = t < Lq ? P.lse[stat + t] * kLog2e : INFINITY;
  }
  if (nqb > 0) st.commit(Qb, Ob);

  constexpr bool dropout = DROPOUT;            // compile-time: no branch inside the tile loop, its two tiles schedule as one block
  const float keep_scale = dropout ? 1.f / (1.f - P.p_drop) : 1.f;
  const unsigned int seedmix = dropout ? seed_fold(effective_seed(P.seed, P.seed_dev)) : 0u;
  const unsigned int thr16 = P.drop_thr >> 16;
  const unsigned int pitch2 = (unsigned int)((P.L + 1) >> 1);
  const unsigned int bh_base = ((unsigned int)W.b * P.H + h) * P.Lq;

  f32x4 dq[NQB][4];                                              // dQ^T strips of every query block = K^T dS^T
#pragma unroll
  for (int i = 0; i < NQB; ++i)
#pragma unroll
    for (int n = 0; n < 4; ++n) dq[i][n] = zero_acc();
  int cur = 0;                                                   // Q / dO buffer of the current query block; parked dS alternates with it

  for (int j = 0; j < nkb; ++j) {
    const int t = j * BLK + 16 * wave + m;                       // this lane's key
    const bool active = j * BLK + 16 * wave < L;                 // wave-uniform: the strip has at least one key
    const int tc = min(t, L - 1);
    u32x4 kr[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int e = threadIdx.x + i * kThreads, r = j * BLK + (e >> 3), ch = e & 7;
      kr[i] = r < L ? *reinterpret_cast<const u32x4 *>(reinterpret_cast<const char *>(kb) + (unsigned int)(r * P.ld_kv + ch * 8) * 2u) : zero4();
    }
    bf16x8 bk[2], bv[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      bk[c] = as_frag(load_frag(kb, tc, P.ld_kv, 32 * c + 8 * g));
      bv[c] = as_frag(load_frag(vb, tc, P.ld_kv, 32 * c + 8 * g));
    }
    const float kt = (t < L && !(P.mask && P.mask[W.row0 + tc])) ? 0.f : -INFINITY;
    __syncthreads();       // the dQ products of block j - 1 have read its K tile (j = 0: the prologue's lse2 / delta / Q / dO)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int e = threadIdx.x + i * kThreads, r = e >> 3, ch = e & 7;
      *reinterpret_cast<u32x4 *>(Kt + r * KS + ch * 8) = kr[i];
    }
    f32x4 dk[4], dv[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      dk[n] = zero_acc();
      dv[n] = zero_acc();
    }
#pragma nounroll
    for (int i = 0; i < nqb; ++i) {
      {
        const int nxt = cur ^ 1;
        const bool more = i + 1 < nqb || j + 1 < nkb;
        if (more) st.issue(qb, P.ld_q, dob, P.ld_o, (i + 1 < nqb ? i + 1 : 0) * BLK, Lq);
        const uint16_t *Qc = Qb + cur * kTile, *Oc = Ob + cur * kTile;
        uint16_t *Dc = Ds + cur * kTile;
        uint16_t *drow = Dc + (16 * wave + m) * KS + 4 * g;      // this lane's key row of the parked dS
        if (active) {
          const float *lc = ls + i * BLK, *dc = dl + i * BLK;
          // role A, 32 queries at a time as in bwd_dkv_kernel
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            f32x4 pt[2], ds[2];
#pragma unroll
            for (int ii = 0; ii < 2; ++ii) {
              const int it = 2 * c + ii;         // query tile of the block
              f32x4 sacc = zero_acc(), dacc = zero_acc();
#pragma unroll
              for (int cc = 0; cc < 2; ++cc) {
                const u32x4 vq = *reinterpret_cast<const u32x4 *>(Qc + (16 * it + m) * KS + 32 * cc + 8 * g);
                const u32x4 vo = *reinterpret_cast<const u32x4 *>(Oc + (16 * it + m) * KS + 32 * cc + 8 * g);
                sacc = mfma32(as_frag(vq), bk[cc], sacc);       // S[query 16 it + 4 g + r][key t]
                dacc = mfma32(as_frag(vo), bv[cc], dacc);       // dO V^T
              }
              const f32x4 lq = *reinterpret_cast<const f32x4 *>(lc + 16 * it + 4 * g);
              const f32x4 dq4 = *reinterpret_cast<const f32x4 *>(dc + 16 * it + 4 * g);
              bool keep[4] = {true, true, true, true};
              if (dropout) {
                // hashes of (query q0 + r, key pair t >> 1): this lane computes two of the four, the lane of the other key
                // of the pair (m ^ 1) the other two
                const int q0 = i * BLK + 16 * it + 4 * g, par = m & 1;
                const unsigned int qa = (unsigned int)(q0 + 2 * par);
                const unsigned int ha = pair_rng(seedmix, (bh_base + qa) * pitch2, t);
                const unsigned int hb = pair_rng(seedmix, (bh_base + qa + 1u) * pitch2, t);
                const unsigned int oa = (unsigned int)__shfl_xor((int)ha, 1, 64), ob2 = (unsigned int)__shfl_xor((int)hb, 1, 64);
                const unsigned int hr0 = par ? oa : ha, hr1 = par ? ob2 : hb, hr2 = par ? ha : oa, hr3 = par ? hb : ob2;
                const unsigned int sh = par ? 16u : 0u;
                keep[0] = ((hr0 >> sh) & 0xFFFFu) >= thr16;
                keep[1] = ((hr1 >> sh) & 0xFFFFu) >= thr16;
                keep[2] = ((hr2 >> sh) & 0xFFFFu) >= thr16;
                keep[3] = ((hr3 >> sh) & 0xFFFFu) >= thr16;
              }
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const float p = __builtin_amdgcn_exp2f(fmaf(sacc[r], kC, kt) - lq[r]);
                const float dp = keep[r] ? dacc[r] : 0.f;
                pt[ii][r] = keep[r] ? p : 0.f;                                  // 1 / (1 - p) goes onto dV below
                ds[ii][r] = p * fmaf(dp, keep_scale, -dq4[r]);                  // 1/8 goes onto dK and dQ below
              }
            }
            const bf16x8 pb = pack_tiles(pt[0], pt[1]);
            const bf16x8 db = pack_tiles(ds[0], ds[1]);
            const u32x4 dw = __builtin_bit_cast(u32x4, db);
            const u32x2 d0 = {dw[0], dw[1]}, d1 = {dw[2], dw[3]};
            *reinterpret_cast<u32x2 *>(drow + 32 * c) = d0;                     // queries 32 c + 4 g + 0..3 of key 16 wave + m
            *reinterpret_cast<u32x2 *>(drow + 32 * c + 16) = d1;
#pragma unroll
            for (int n = 0; n < 4; ++n) {
              dv[n] = mfma32(tr_frag_perm(Oc, KS, c, 16 * n, lane), pb, dv[n]);
              dk[n] = mfma32(tr_frag_perm(Qc, KS, c, 16 * n, lane), db, dk[n]);
            }
            __builtin_amdgcn_sched_barrier(0);
          }
        } else {                                                 // no key in this strip: its dS rows are zero
          const u32x2 z = {0u, 0u};
#pragma unroll
          for (int c = 0; c < 4; ++c) *reinterpret_cast<u32x2 *>(drow + 16 * c) = z;
        }
        if (more) st.commit(Qb + nxt * kTile, Ob + nxt * kTile);
        __syncthreads();
        // role B: dQ^T of block i += K_j^T dS^T, the strip of queries 16 wave .. + 15 (wave-uniform: it has a query)
        if (i * BLK + 16 * wave < Lq) {
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            const bf16x8 db = tr_frag_perm(Dc, KS, c, 16 * wave, lane);         // dS[query 16 wave + m][keys in pack_tiles order]
            bf16x8 ka[4];
#pragma unroll
            for (int n = 0; n < 4; ++n) ka[n] = tr_frag_perm(Kt, KS, c, 16 * n, lane);
            // the accumulators are registers: the block index is resolved by workgroup-uniform branches, not by address
#pragma unroll
            for (int ii = 0; ii < NQB; ++ii) {
              if (ii == i) {
#pragma unroll
                for (int n = 0; n < 4; ++n) dq[ii][n] = mfma32(ka[n], db, dq[ii][n]);
              }
            }
          }
        }
        cur = nxt;
      }
    }
    if (active && t < L) {
      uint16_t *pk = P.dk + (W.row0 + t) * P.ld_dkv + h * DH + 4 * g;
      uint16_t *pv = P.dv + (W.row0 + t) * P.ld_dkv + h * DH + 4 * g;
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const u32x2 vk = {pack2(dk[n][0] * 0.125f, dk[n][1] * 0.125f), pack2(dk[n][2] * 0.125f, dk[n][3] * 0.125f)};
        const u32x2 vv = {pack2(dv[n][0] * keep_scale, dv[n][1] * keep_scale), pack2(dv[n][2] * keep_scale, dv[n][3] * keep_scale)};
        *reinterpret_cast<u32x2 *>(pk + 16 * n) = vk;
        *reinterpret_cast<u32x2 *>(pv + 16 * n) = vv;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NQB; ++i) {
    const int qi = i * BLK + 16 * wave + m;
    if (i < nqb && qi < Lq) {
      uint16_t *op = P.dq + (W.row0q + qi) * P.ld_dq + h * DH + 4 * g;
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const u32x2 v = {pack2(dq[i][n][0] * 0.125f, dq[i][n][1] * 0.125f), pack2(dq[i][n][2] * 0.125f, dq[i][n][3] * 0.125f)};
        *reinterpret_cast<u32x2 *>(op + 16 * n) = v;
      }
    }
  }
  if (P.q_limit && P.cu_rows && Lq < L) {       // queries that were not computed: their dQ rows are zero
    for (int e = threadIdx.x; e < (L - Lq) * 8; e += kThreads) {
      const int qr = Lq + (e >> 3);
      *reinterpret_cast<u32x4 *>(P.dq + (W.row0q + qr) * P.ld_dq + h * DH + 8 * (e & 7)) = zero4();
    }
  }
}

}  // namespace gps_attn_fa

namespace gps_attn {

// block-streaming plain form (no pairwise term); argument checks done by run_ex.  Backward needs `out` and the
// (B, H, Lq) fp32 workspace `delta_ws`.
int run_plain_blocks(const gps_attn_args *a, bool backward, hipStream_t s) {
  using namespace gps_attn_fa;
  if (a->sw || a->pl || a->pl_planes || a->dtype != GPS_ATTN_BF16) return GPS_ERR_UNSUPPORTED;
  if (backward && (!a->out || !a->delta_ws)) return GPS_ERR_UNSUPPORTED;
  Params P = {};
  P.B = a->B; P.H = a->H; P.L = a->Lk; P.Lq = a->Lq;
  P.ld_q = a->ld_q; P.ld_kv = a->ld_kv; P.ld_o = a->ld_o;
  P.q = (const uint16_t *)a->q; P.k = (const uint16_t *)a->k; P.v = (const uint16_t *)a->v;
  P.mask = a->mask; P.out = (uint16_t *)a->out; P.lse = a->lse;
  P.p_drop = a->p_drop; P.seed = a->seed; P.seed_dev = (const unsigned long long *)a->seed_dev;
  P.drop_thr = gps_dropout::drop_threshold(a->p_drop);
  P.cu_rows = a->cu_rows;
  P.seq_order = a->cu_rows ? a->seq_order : nullptr;
  P.q_limit = a->cu_rows ? a->q_limit : nullptr;
  const int nqb = (a->Lq + BLK - 1) / BLK, nkb = (a->Lk + BLK - 1) / BLK;
  if (!backward) {
    P.nblk = nqb;
    hipLaunchKernelGGL(fwd_kernel, dim3(P.B * P.H * nqb), dim3(kThreads), kLdsFwd, s, P);
    return hipGetLastError() == hipSuccess ? GPS_OK : GPS_ERR_LAUNCH;
  }
  P.dout = (const uint16_t *)a->dout; P.dq = (uint16_t *)a->dq; P.dk = (uint16_t *)a->dk; P.dv = (uint16_t *)a->dv;
  P.ld_dq = a->ld_dq; P.ld_dkv = a->ld_dkv; P.delta = a->delta_ws;
  P.nblk = nqb;
  hipLaunchKernelGGL(bwd_dq_kernel, dim3(P.B * P.H * nqb), dim3(kThreads), kLdsFwd, s, P);
  if (hipGetLastError() != hipSuccess) return GPS_ERR_LAUNCH;
  P.nblk = nkb;
  hipLaunchKernelGGL(bwd_dkv_kernel, dim3(P.B * P.H * nkb), dim3(kThreads), kLdsDkv, s, P);
  return hipGetLastError() == hipSuccess ? GPS_OK : GPS_ERR_LAUNCH;
}

template <int NQB, bool DROPOUT>
static int launch_fused_as(const gps_attn_fa::Params &P, size_t &granted, hipStream_t s) {
  using namespace gps_attn_fa;
  constexpr size_t lds = lds_fused(NQB);
  if (gps_dev::grant_lds((const void *)&bwd_fused_kernel<NQB, DROPOUT>, lds, lds, granted) != GPS_OK) return GPS_ERR_LAUNCH;
  hipLaunchKernelGGL((bwd_fused_kernel<NQB, DROPOUT>), dim3(P.B * P.H), dim3(kThreads), lds, s, P);
  return hipGetLastError() == hipSuccess ? GPS_OK : GPS_ERR_LAUNCH;
}
template <int NQB>
static int launch_fused(const gps_attn_fa::Params &P, size_t *granted, hipStream_t s) {
  return P.drop_thr != 0u ? launch_fused_as<NQB, true>(P, granted[1], s) : launch_fused_as<NQB, false>(P, granted[0], s);
}

// one-launch backward of plain self-attention up to kFusedMaxCap tokens (fixed-length with a key-padding mask, or packed
// variable-length sequences); argument checks done by run_ex.  Needs `out`; delta_ws is not used.
int run_plain_fused_bwd(const gps_attn_args *a, hipStream_t s) {
  using namespace gps_attn_fa;
  if (a->sw || a->pl || a->pl_planes || a->dtype != GPS_ATTN_BF16 || !a->out || a->Lq != a->Lk || a->Lk > kFusedMaxCap)
    return GPS_ERR_UNSUPPORTED;
  Params P = {};
  P.B = a->B; P.H = a->H; P.L = a->Lk; P.Lq = a->Lq;
  P.ld_q = a->ld_q; P.ld_kv = a->ld_kv; P.ld_o = a->ld_o;
  P.q = (const uint16_t *)a->q; P.k = (const uint16_t *)a->k; P.v = (const uint16_t *)a->v;
  P.mask = a->mask; P.out = (uint16_t *)a->out; P.lse = a->lse;
  P.p_drop = a->p_drop; P.seed = a->seed; P.seed_dev = (const unsigned long long *)a->seed_dev;
  P.drop_thr = gps_dropout::drop_threshold(a->p_drop);
  P.cu_rows = a->cu_rows;
  P.seq_order = a->cu_rows ? a->seq_order : nullptr;
  P.q_limit = a->cu_rows ? a->q_limit : nullptr;
  P.dout = (const uint16_t *)a->dout; P.dq = (uint16_t *)a->dq; P.dk = (uint16_t *)a->dk; P.dv = (uint16_t *)a->dv;
  P.ld_dq = a->ld_dq; P.ld_dkv = a->ld_dkv;
  P.nblk = 1;                                   // one workgroup per (sequence, head)
  static gps_dev::PerDevice<size_t, 8> granted_dev;      // [register blocks][dropout]
  size_t *granted = granted_dev.row();
  const int nqb = (a->Lq + BLK - 1) / BLK;      // dQ^T register blocks: 1, 2, 3 or 5
  if (nqb <= 1) return launch_fused<1>(P, granted + 0, s);
  if (nqb == 2) return launch_fused<2>(P, granted + 2, s);
  if (nqb == 3) return launch_fused<3>(P, granted + 4, s);
  return launch_fused<5>(P, granted + 6, s);
}

}  // namespace gps_attn
