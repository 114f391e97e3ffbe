// gps_sa_mlp.hip -- fused set-abstraction level for a FROZEN PointNet++ encoder on MI355X (gfx950).
//
// One launch replaces, for one SA level of the reference
//   modules/third_party/pointnet2/pointnet2_utils.py:345-356   group xyz, subtract centre, group feats, cat
//   modules/third_party/pointnet2/pytorch_utils.py:11-36       SharedMLP = 3 x (conv1x1 no-bias, BN, ReLU)
//   modules/third_party/pointnet2/pointnet2_modules.py:65-71   max_pool2d over nsample
// i.e. 2 group_points launches, `-=`, `cat`, 3 x (GEMM, batch-norm, ReLU) and a max-pool -- about
// half of the GPS training step in the first rocprof trace (profiles/r1/bench_b_kernel_stats.csv).
// In 35 of the reference's 37 configs the encoder is frozen: BN runs on its running statistics and
// nothing needs a gradient, so conv+BN folds into W' = diag(gamma/sqrt(var+eps)) W and a shift.
//
// Design (CDNA4):
//   * one 256-thread workgroup per object; the object's points/features/indices are staged once in
//     LDS (coalesced 16-byte loads), so the grouped (3+C, npoint, nsample) tensor -- 268 KB per
//     object at SA2, the largest HBM stream of the point path -- never exists in HBM;
//   * a wave owns one group = one 32-column tile (nsample == 32) through ALL three layers (dense kernels; the distinct-sample
//     form of the split-bf16 variant, below, owns 32 columns of a compacted list instead -- default at SA2).  Layers
//     run on v_mfma_f32_32x32x2_f32 (fp32 in, fp32 accumulate: bitwise an fmaf chain, so results
//     stay within fp32 summation-order noise of the reference's fp32 conv).  The D fragment of one
//     layer (lane = column, registers = rows) IS the B fragment of the next layer's MFMAs once the
//     K index is permuted to the D row order -- the permutation is applied to the packed weights
//     instead, so activations never leave the VGPRs between layers;
//   * weights stream through LDS one 32-row output tile at a time (double buffered, one barrier per
//     tile); folded BN shift initialises the accumulator, ReLU is one v_max per register;
//   * max over the 32 samples = DPP row reduction + row_bcast15; pooled rows are collected in LDS
//     and written with coalesced stores.
//
//   * split-bf16 form (namespace x3, the default precision): the streamed-weight level (SA2) runs the MLP on each
//     group's DISTINCT samples only -- the ball query's filler slots repeat slot 0 and cannot change the max -- with a
//     compact column list in LDS, several objects per workgroup and a segmented max-pool (sa_mlp_x3_distinct_kernel;
//     gps_sa_mlp_set_distinct).  The dense kernels below stay as the reference and as the resident-weight level (SA1).
//
// What the three kernels share is stated once: Geometry (steps, tile sizes and counts of a (CF, C1, C2, C3) MLP), Layout
// (the LDS carve-up, read by the kernel for its pointers and by the host for its byte count), stage_objects, WeightStream
// and copy_out_dense; the two split-bf16 kernels also share gather_layer1, split_tile, group_max and mlp_tile (the
// three-layer walk over one 32-column tile, pooling passed in).
//
// K-slot order.  For v_mfma_f32_32x32x2_f32 lane l holds A[i = l&31][k = l>>5], B[k = l>>5][j = l&31]
// and D[row = (r&3) + 8*(r>>2) + 4*(l>>5)][col = l&31] in register r.  Input channels are therefore
// consumed in "slots" (it, r): the step for slot (it, r) multiplies channel it*32 + (r&3) + 8*(r>>2)
// (lanes 0-31) and that + 4 (lanes 32-63).  gps_sa_mlp_pack_layer() writes the weights in that
// order, zero where the channel is >= c_in.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gps_hip.h"
#include "gps_device_flags.h"

namespace gps { const int *object_extent(); }   // gps_point_ops.hip: device int or null (gps_point_set_object_extent)

#ifndef GPS_SA1_WAVES
#define GPS_SA1_WAVES 8   // weights resident in LDS: waves only share the object
#endif
#ifndef GPS_SA2_WAVES
#define GPS_SA2_WAVES 8   // streamed weights: 8 groups per weight tile
#endif

namespace gps_sa {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kBlock = 256;
constexpr int kWaves = 4;
constexpr int kNS = 32;  // samples per group == MFMA N

__host__ __device__ constexpr int slot_channel(int it, int r, int h) {
  return it * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
}
// number of K steps of a layer with c_in input channels (slots whose lower channel exists)
__host__ __device__ constexpr int layer_steps(int c_in) {
  int s = 0;
  for (int it = 0; it < (c_in + 31) / 32; ++it)
    for (int r = 0; r < 16; ++r)
      if (slot_channel(it, r, 0) < c_in) ++s;
  return s;
}
// floats of one packed 32-row output tile: steps x 64 weights + 32 shifts, padded to whole
// 1 KiB pieces (one global_load_lds_dwordx4 wave-instruction each)
__host__ __device__ constexpr int tile_floats(int c_in) {
  return (layer_steps(c_in) * 64 + 32 + 255) / 256 * 256;
}

// ------------------------------------------------------------------------------------------
// weight packing: w (c_out, c_in) row-major (already BN-folded), shift (c_out) ->
//   dst[mt][step][h*32 + i] = w[mt*32 + i][channel(step, h)]   (0 beyond c_in)
//   dst[mt][steps*64 + i]   = shift[mt*32 + i]
// ------------------------------------------------------------------------------------------
__global__ void pack_layer_kernel(int c_in, int c_out, const float *__restrict__ w,
                                  const float *__restrict__ shift, float *__restrict__ dst) {
  const int steps = layer_steps(c_in);
  const int tf = tile_floats(c_in);
  const int total = (c_out / 32) * tf;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    const int mt = e / tf, o = e - mt * tf;
    if (o >= steps * 64) {
      dst[e] = o < steps * 64 + 32 ? shift[mt * 32 + (o - steps * 64)] : 0.f;
      continue;
    }
    const int s = o >> 6, h = (o >> 5) & 1, i = o & 31;
    // s-th valid slot
    int it = 0, r = 0, cnt = 0;
    for (int a = 0; a < (c_in + 31) / 32; ++a)
      for (int q = 0; q < 16; ++q)
        if (slot_channel(a, q, 0) < c_in) {
          if (cnt == s) { it = a; r = q; }
          ++cnt;
        }
    const int k = slot_channel(it, r, h);
    dst[e] = k < c_in ? w[(size_t)(mt * 32 + i) * c_in + k] : 0.f;
  }
}

// ------------------------------------------------------------------------------------------
// helpers
// ------------------------------------------------------------------------------------------
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_max_f32(float v) {
  const int o = __builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, ROW_MASK,
                                            0xf, false);
  return fmaxf(v, __int_as_float(o));
}
// max over lanes 0-31 -> lane 31, over lanes 32-63 -> lane 63
__device__ __forceinline__ float half_wave_max(float v) {
  v = dpp_max_f32<0x111, 0xf>(v);  // row_shr:1
  v = dpp_max_f32<0x112, 0xf>(v);  // row_shr:2
  v = dpp_max_f32<0x114, 0xf>(v);  // row_shr:4
  v = dpp_max_f32<0x118, 0xf>(v);  // row_shr:8  -> lane 15 of each 16-lane row = row max
  v = dpp_max_f32<0x142, 0xa>(v);  // row_bcast:15 into rows 1 and 3 -> lanes 31 / 63
  return v;
}

// One 32-row output tile: acc = shift; acc += sum_s A[s] (LDS) x B[s] (registers).
template <int STEPS>
__device__ __forceinline__ f32x16 mfma_tile(const float *__restrict__ tile, const float (&B)[STEPS],
                                            int lane) {
  f32x16 acc;
  const float *sh = tile + STEPS * 64 + 4 * (lane >> 5);
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = sh[(r & 3) + 8 * (r >> 2)];
#pragma unroll
  for (int s = 0; s < STEPS; ++s)
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(tile[s * 64 + lane], B[s], acc, 0, 0, 0);
  return acc;
}

// Cooperative asynchronous copy of one packed tile (len floats, a multiple of 256) from global
// memory straight into LDS: each wave-instruction moves 1 KiB (64 lanes x 16 B) to
// wave-uniform base + lane * 16, no VGPRs held while the MFMAs run.  Completion = the issuing
// wave's vmcnt(0), then the workgroup barrier.
template <int NWAVES = kWaves>
__device__ __forceinline__ void tile_copy_async(const float *__restrict__ src, float *dst, int len,
                                                int wave, int lane) {
  for (int c = wave; c * 256 < len; c += NWAVES)
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void *)(src + c * 256 + lane * 4),
        (__attribute__((address_space(3))) void *)(dst + c * 256), 16, 0, 0);
}
__device__ __forceinline__ void tile_copy_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// ------------------------------------------------------------------------------------------
// What the fp32 kernel and the two split-bf16 kernels have in common.
// ------------------------------------------------------------------------------------------
// Layer geometry of a (CF -> C1 -> C2 -> C3) MLP in one packed form: STEPS(c_in) = K steps of a layer, TILE(c_in) = floats
// of one packed 32-row output tile of it (layer_steps / tile_floats here, x3::steps16 / x3::tile_floats16 below).
template <int CF_, int C1_, int C2_, int C3_, int (*STEPS)(int), int (*TILE)(int)>
struct Geometry {
  static_assert(C1_ % 32 == 0 && C2_ % 32 == 0 && C3_ % 32 == 0, "whole 32-row output tiles");
  static constexpr int CF = CF_, C1 = C1_, C2 = C2_, C3 = C3_, CIN = 3 + CF_;
  static constexpr int S1 = STEPS(CIN), S2 = STEPS(C1), S3 = STEPS(C2);
  static constexpr int T1 = TILE(CIN), T2 = TILE(C1), T3 = TILE(C2);
  static constexpr int M1 = C1 / 32, M2 = C2 / 32, M3 = C3 / 32;
  static constexpr int TMAX = T1 > T2 ? (T1 > T3 ? T1 : T3) : (T2 > T3 ? T2 : T3);
  static constexpr int TOTAL = M1 * T1 + M2 * T2 + M3 * T3;   // floats of wpack = [layer 1 tiles | layer 2 tiles | layer 3 tiles]
  static constexpr int G = M1 + M2 + M3;                      // weight tiles (stages) per round
  // offset (floats) in wpack of weight tile g (mod G), and its length
  static __device__ __forceinline__ int tile_off(int g, int &len) {
    if (g >= G) g -= G;
    if (g < M1) { len = T1; return g * T1; }
    if (g < M1 + M2) { len = T2; return M1 * T1 + (g - M1) * T2; }
    len = T3;
    return M1 * T1 + M2 * T2 + (g - M1 - M2) * T3;
  }
};

// The carve-up of dynamic LDS, offsets in floats.  The kernel takes its pointers from Layout<..., int>, the host its byte
// count from Layout<..., size_t>::bytes(): no size is written down apart from this list.  OBJS objects per workgroup;
//   DISTINCT = false (fp32 and dense split-bf16 kernels, OBJS = 1): pooled features [C3][npoint], as they go to HBM;
//   DISTINCT = true: pooled rows [group][channel] of bit patterns with a pitch of C3 + 1 words (why: the distinct kernel's
//   header), the list of kept columns and the groups' offsets into it.
template <class GEO, bool RESIDENT, int OBJS, bool DISTINCT, typename I>
struct Layout {
  static constexpr int WBUF = RESIDENT ? GEO::TOTAL : 2 * GEO::TMAX;   // the whole wpack, or buffers w0 (at 0) and w1 (at TMAX)
  static constexpr int OLD = GEO::C3 + 1;                              // pitch of a pooled row (DISTINCT)
  I out, feat, xyz, ctr, idx, list, off, end;
  __host__ __device__ Layout(I n, I npoint) {
    const I groups = OBJS * npoint;
    out = WBUF;                                                        // [C3][npoint] | [groups][OLD]
    feat = out + (DISTINCT ? (groups * OLD + 3) & ~(I)3 : GEO::C3 * npoint);   // [OBJS][CF][n]  (channel-major, 16-byte aligned)
    xyz = feat + OBJS * GEO::CF * n;                                   // [OBJS][n][3]
    ctr = xyz + OBJS * n * 3;                                          // [groups][3]
    idx = ctr + groups * 3;                                            // [groups][32] int32
    list = idx + groups * kNS;                                         // [groups * 32] kept columns: group << 16 | point
    off = list + (DISTINCT ? groups * kNS : 0);                        // [groups + 1] first list entry of a group
    end = off + (DISTINCT ? groups + 1 : 0);
  }
  size_t bytes() const { return sizeof(float) * (size_t)end; }
};

// Stage `nobj` consecutive objects, the first obj0, into LDS: features ([o][CF][n], channel-major as in HBM; PM: they arrive
// point-major, feats[(obj * n + p) * ld_feat + c], and are transposed on the way), xyz, centres, idx.  OBJS = 1 where nobj is.
template <int CF, bool PM, int OBJS, int BLOCK>
__device__ __forceinline__ void stage_objects(int obj0, int nobj, int n, int npoint, const float *__restrict__ xyz,
                                              const float *__restrict__ new_xyz, const float *__restrict__ feats,
                                              const int32_t *__restrict__ idx, int ld_feat, float *s_feat, float *s_xyz,
                                              float *s_ctr, int32_t *s_idx, int tid) {
  const float *gx = xyz + (size_t)obj0 * n * 3;
  const float *gc = new_xyz + (size_t)obj0 * npoint * 3;
  const int32_t *gi = idx + (size_t)obj0 * npoint * kNS;
  if (PM) {
    const float *gf = feats + (size_t)obj0 * n * ld_feat;
    for (int e = tid; e < nobj * CF * n; e += BLOCK) {
      const int pp = e / CF, c = e - pp * CF;                   // pp = o * n + p
      const int o = OBJS > 1 ? pp / n : 0;
      s_feat[o * CF * n + c * n + (pp - o * n)] = gf[(size_t)pp * ld_feat + c];
    }
  } else {
    const float *gf = feats + (size_t)obj0 * CF * n;
    if (((CF * n) & 3) == 0) {
      const float4 *g4 = reinterpret_cast<const float4 *>(gf);
      float4 *l4 = reinterpret_cast<float4 *>(s_feat);
      for (int e = tid; e < (nobj * CF * n) >> 2; e += BLOCK) l4[e] = g4[e];
    } else {
      for (int e = tid; e < nobj * CF * n; e += BLOCK) s_feat[e] = gf[e];
    }
  }
  for (int e = tid; e < nobj * n * 3; e += BLOCK) s_xyz[e] = gx[e];
  for (int e = tid; e < nobj * npoint * 3; e += BLOCK) s_ctr[e] = gc[e];
  for (int e = tid; e < nobj * npoint * kNS; e += BLOCK) s_idx[e] = gi[e];
}

// The weight tiles of wpack, one per stage g of a round rd.  RESIDENT: the whole wpack sits in LDS after first(), a stage
// is an offset.  Otherwise the 32-row tiles stream through the double buffer w0 / w1: g counts the stages of a round, gg
// all stages so far; tile gg sits in buffer gg & 1 and begin() starts the copy of the next tile into the other one (G may
// be odd, so the parity carries over rounds), end() is that copy's wait and the workgroup's one barrier per tile.
template <class GEO, int WAVES, bool RESIDENT>
struct WeightStream {
  const float *wpack;
  float *s_w0;
  int wave, lane;
  __device__ __forceinline__ void first() const {               // completion: tile_copy_wait() + barrier, by the caller
    tile_copy_async<WAVES>(wpack, s_w0, RESIDENT ? GEO::TOTAL : GEO::T1, wave, lane);
  }
  __device__ __forceinline__ const float *begin(int rd, int g) const {   // -> the LDS tile to compute on
    int len;
    if (RESIDENT) return s_w0 + GEO::tile_off(g, len);
    const int gg = rd * GEO::G + g;
    const int off = GEO::tile_off(g + 1, len);
    float *s_w1 = s_w0 + GEO::TMAX;
    tile_copy_async<WAVES>(wpack + off, (gg & 1) ? s_w0 : s_w1, len, wave, lane);
    return (gg & 1) ? s_w1 : s_w0;
  }
  __device__ __forceinline__ void end() const {
    if (!RESIDENT) {
      tile_copy_wait();
      __syncthreads();
    }
  }
};

// pooled features [C3][npoint] of one object out, coalesced
template <int BLOCK>
__device__ __forceinline__ void copy_out_dense(const float *s_out, float *go, int total, int tid) {
  if ((total & 3) == 0) {
    const float4 *l4 = reinterpret_cast<const float4 *>(s_out);
    float4 *g4 = reinterpret_cast<float4 *>(go);
    for (int e = tid; e < total >> 2; e += BLOCK) g4[e] = l4[e];
  } else {
    for (int e = tid; e < total; e += BLOCK) go[e] = s_out[e];
  }
}

// ------------------------------------------------------------------------------------------
// fused SA level: ball-query indices in, pooled features out.
//   xyz (b,n,3), new_xyz (b,npoint,3), feats (b,CF,n), idx (b,npoint,32) -> out (b,C3,npoint)
//   wpack = [layer 1 tiles | layer 2 tiles | layer 3 tiles]
// ------------------------------------------------------------------------------------------
template <int CF, int C1, int C2, int C3>
using GeometryF32 = Geometry<CF, C1, C2, C3, layer_steps, tile_floats>;

template <int CF, int C1, int C2, int C3>
__global__ __launch_bounds__(kBlock, 2) void sa_mlp_kernel(
    int b, int n, int npoint, const float *__restrict__ xyz, const float *__restrict__ new_xyz,
    const float *__restrict__ feats, const int32_t *__restrict__ idx,
    const float *__restrict__ wpack, float *__restrict__ out, const int *__restrict__ n_obj_dev) {
  if (n_obj_dev && (int)blockIdx.x >= *n_obj_dev) return;      // object extent: nothing read or written
  using GEO = GeometryF32<CF, C1, C2, C3>;
  constexpr int CIN = GEO::CIN, S1 = GEO::S1, S2 = GEO::S2, S3 = GEO::S3, M1 = GEO::M1, M2 = GEO::M2, M3 = GEO::M3;

  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Layout<GEO, false, 1, false, int> L(n, npoint);
  float *s_out = lds + L.out, *s_feat = lds + L.feat, *s_xyz = lds + L.xyz, *s_ctr = lds + L.ctr;
  int32_t *s_idx = reinterpret_cast<int32_t *>(lds + L.idx);

  const int obj = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 31, h = lane >> 5;

  stage_objects<CF, false, 1, kBlock>(obj, 1, n, npoint, xyz, new_xyz, feats, idx, 0, s_feat, s_xyz, s_ctr, s_idx, tid);
  const WeightStream<GEO, kWaves, false> ws{wpack, lds, wave, lane};
  ws.first();
  tile_copy_wait();
  __syncthreads();

  const int rounds = (npoint + kWaves - 1) / kWaves;
  for (int rd = 0; rd < rounds; ++rd) {
    const int tile = rd * kWaves + wave;
    const bool live = tile < npoint;
    const int j = live ? tile : npoint - 1;

    // ---- layer-1 B operand: X0[channel][sample] gathered from LDS ------------------------
    float a0[S1];
    {
      const int p = s_idx[j * kNS + col];
      int s = 0;
#pragma unroll
      for (int it = 0; it < (CIN + 31) / 32; ++it)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (slot_channel(it, r, 0) < CIN) {
            const int k = slot_channel(it, r, h);          // this lane's channel of the slot
            float v = 0.f;
            if (slot_channel(it, r, 1) < 3) {              // both halves are xyz rows
              v = s_xyz[p * 3 + k] - s_ctr[j * 3 + k];
            } else if (slot_channel(it, r, 0) >= 3 && slot_channel(it, r, 1) < CIN) {
              v = s_feat[(k - 3) * n + p];                 // both halves are feature rows
            } else {                                       // mixed slot: decide per lane
              if (k < 3) v = s_xyz[p * 3 + k] - s_ctr[j * 3 + k];
              else if (k < CIN) v = s_feat[(k - 3) * n + p];
            }
            a0[s++] = v;
          }
    }

    float a1[M1 * 16], a2[M2 * 16];
    int g = 0;                                             // stage within the round
    // ---- layer 1 ----------------------------------------------------------------------------
#pragma unroll
    for (int mt = 0; mt < M1; ++mt, ++g) {
      const f32x16 acc = mfma_tile<S1>(ws.begin(rd, g), a0, lane);
#pragma unroll
      for (int r = 0; r < 16; ++r) a1[mt * 16 + r] = fmaxf(acc[r], 0.f);
      ws.end();
    }
    // ---- layer 2 ----------------------------------------------------------------------------
#pragma unroll
    for (int mt = 0; mt < M2; ++mt, ++g) {
      const f32x16 acc = mfma_tile<S2>(ws.begin(rd, g), a1, lane);
#pragma unroll
      for (int r = 0; r < 16; ++r) a2[mt * 16 + r] = fmaxf(acc[r], 0.f);
      ws.end();
    }
    // ---- layer 3 + max over the 32 samples ---------------------------------------------------
    for (int mt = 0; mt < M3; ++mt, ++g) {
      const f32x16 acc = mfma_tile<S3>(ws.begin(rd, g), a2, lane);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float m = half_wave_max(acc[r]);
        if (col == 31 && live)
          s_out[(mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * npoint + tile] = fmaxf(m, 0.f);
      }
      ws.end();
    }
  }
  copy_out_dense<kBlock>(s_out, out + (size_t)obj * C3 * npoint, C3 * npoint, tid);
}

template <int CF, int C1, int C2, int C3>
int launch_sa(int b, int n, int npoint, const float *xyz, const float *new_xyz, const float *feats,
              const int32_t *idx, const float *wpack, float *out, hipStream_t s) {
  const size_t lds = Layout<GeometryF32<CF, C1, C2, C3>, false, 1, false, size_t>(n, npoint).bytes();
  if (lds > 80 * 1024) return GPS_ERR_UNSUPPORTED;   // keep two workgroups per CU
  static gps_dev::PerDevice<size_t, 1> granted;
  const int st = gps_dev::grant_lds(reinterpret_cast<const void *>(&sa_mlp_kernel<CF, C1, C2, C3>), lds, 80 * 1024,
                                    granted.row()[0]);
  if (st != GPS_OK) return st;
  hipLaunchKernelGGL((sa_mlp_kernel<CF, C1, C2, C3>), dim3(b), dim3(kBlock), lds, s, b, n, npoint, xyz,
                     new_xyz, feats, idx, wpack, out, gps::object_extent());
  return GPS_OK;
}


// ==========================================================================================
// split-bf16 variant: every fp32 operand x is carried as (hi, lo) = (bf16(x), bf16(x - hi)) and each
// product as  W_hi X_hi + W_hi X_lo + W_lo X_hi  on v_mfma_f32_32x32x16_bf16 with fp32 accumulation:
// 3 MFMAs at the bf16 rate (16x the fp32 MFMA rate) instead of 8, i.e. ~5.3x fewer matrix-pipe
// cycles, for a relative error ~2^-16 per product (the dropped W_lo X_lo term and the 2^-17
// representation residuals) -- inside the 1e-4 tolerance of the parity tests.
//
// Same chaining trick: D regs [8u, 8u+8) of a 32-row tile are the B fragment (K = 16) of step
// (tile, u) of the next layer; K-slot (half h, element e) <-> channel 32 it + 16 u + 8 (e>>2) + 4 h + (e&3).
// Packed tile (bytes): step s: [hi: 64 lanes x 16 B][lo: 64 lanes x 16 B]; then 32 fp32 shifts;
// padded to 1 KiB.
// ==========================================================================================
namespace x3 {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x8 __attribute__((ext_vector_type(8)));

__host__ __device__ constexpr int steps16(int c_in) { return (c_in + 15) / 16; }
__host__ __device__ constexpr int slot_channel16(int it_u, int e, int h) {   // it_u = 2 * it + u
  return 16 * it_u + 8 * (e >> 2) + 4 * h + (e & 3);
}
// floats (4-byte units) of one packed 32-row tile
__host__ __device__ constexpr int tile_floats16(int c_in) {
  return (steps16(c_in) * 512 + 32 + 255) / 256 * 256;
}
template <int CF, int C1, int C2, int C3>
using Geometry16 = Geometry<CF, C1, C2, C3, steps16, tile_floats16>;

__device__ __forceinline__ uint16_t f2bf(float f) {
  unsigned int u = __float_as_uint(f);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

__global__ void pack_layer16_kernel(int c_in, int c_out, const float *__restrict__ w,
                                    const float *__restrict__ shift, float *__restrict__ dst) {
  const int steps = steps16(c_in);
  const int tf = tile_floats16(c_in);
  const int total = (c_out / 32) * tf;
  for (int e4 = blockIdx.x * blockDim.x + threadIdx.x; e4 < total; e4 += gridDim.x * blockDim.x) {
    const int mt = e4 / tf, o = e4 - mt * tf;   // o: 4-byte unit inside the tile
    if (o >= steps * 512) {
      dst[e4] = o < steps * 512 + 32 ? shift[mt * 32 + (o - steps * 512)] : 0.f;
      continue;
    }
    const int s = o >> 9, part = (o >> 8) & 1, lane = (o >> 2) & 63, pair = o & 3;   // 2 bf16 per unit
    const int i = lane & 31, h = lane >> 5;
    unsigned int packed = 0;
    for (int q = 0; q < 2; ++q) {
      const int e = 2 * pair + q;
      const int k = slot_channel16(s, e, h);
      const float x = k < c_in ? w[(size_t)(mt * 32 + i) * c_in + k] : 0.f;
      const uint16_t hi = f2bf(x);
      const float back = __uint_as_float((unsigned int)hi << 16);
      const uint16_t v = part == 0 ? hi : f2bf(x - back);
      packed |= (unsigned int)v << (16 * q);
    }
    dst[e4] = __uint_as_float(packed);
  }
}

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
// two fp32 -> one dword of two bf16 (round to nearest even); hipcc's vector convert emits one
// single-element v_cvt_pk per value plus shifts/ors, so the instruction is named explicitly
__device__ __forceinline__ unsigned int cvt_pk_bf16(float a, float b) {
  unsigned int r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// max(x, 0) as ONE compiler-visible instruction: on the raw bits, signed-integer max with 0 maps
// every negative float (and -0) to +0 and keeps every non-negative one (v_max_i32).  fmaxf() would
// cost a canonicalising v_max first; an inline-asm v_max_f32 must NOT be used here: hipcc's hazard
// recogniser does not see inline-asm readers of MFMA results and would not pad the XDL-write ->
// VALU-read wait states (observed: stale accumulators).
__device__ __forceinline__ float relu1(float x) {
  const int i = __float_as_int(x);
  return __int_as_float(i > 0 ? i : 0);
}
// v -> (hi, lo) bf16 fragments with v ~= hi + lo:  3 VALU per element
__device__ __forceinline__ void split8(const f32x8 &v, bf16x8 &hi, bf16x8 &lo) {
  u32x4 h, l;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    h[i] = cvt_pk_bf16(v[2 * i], v[2 * i + 1]);
    const float b0 = __uint_as_float(h[i] << 16), b1 = __uint_as_float(h[i] & 0xFFFF0000u);
    l[i] = cvt_pk_bf16(v[2 * i] - b0, v[2 * i + 1] - b1);
  }
  hi = __builtin_bit_cast(bf16x8, h);
  lo = __builtin_bit_cast(bf16x8, l);
}
// NPROD = 3: the three products above (fp32-accurate); NPROD = 1: W_hi X_hi only -- plain bf16 operands with fp32
// accumulation, what torch's bf16 autocast computes for the reference's Conv2d stacks (opt-in: gps_sa_mlp_set_products)
template <int STEPS, bool TRANSPOSED = false, int NPROD = 3>
__device__ __forceinline__ f32x16 mfma_tile16(const float *__restrict__ tile, const bf16x8 (&Bhi)[STEPS],
                                              const bf16x8 (&Blo)[STEPS], int lane) {
  f32x16 acc;
  if (TRANSPOSED) {
    const float shc = tile[STEPS * 512 + (lane & 31)];        // shift of this lane's output channel
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = shc;
  } else {
    const float *sh = tile + STEPS * 512 + 4 * (lane >> 5);
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = sh[(r & 3) + 8 * (r >> 2)];
  }
  const bf16x8 *frag = reinterpret_cast<const bf16x8 *>(tile) + lane;
#pragma unroll
  for (int s = 0; s < STEPS; ++s) {
    const bf16x8 ahi = frag[s * 128];
    if (NPROD == 1) {
      acc = TRANSPOSED ? __builtin_amdgcn_mfma_f32_32x32x16_bf16(Bhi[s], ahi, acc, 0, 0, 0)
                       : __builtin_amdgcn_mfma_f32_32x32x16_bf16(ahi, Bhi[s], acc, 0, 0, 0);
      continue;
    }
    const bf16x8 alo = frag[s * 128 + 64];
    if (TRANSPOSED) {
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Bhi[s], alo, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Blo[s], ahi, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Bhi[s], ahi, acc, 0, 0, 0);
    } else {
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(alo, Bhi[s], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ahi, Blo[s], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ahi, Bhi[s], acc, 0, 0, 0);
    }
  }
  return acc;
}

// Layer-1 B operand of one column (= this lane's, both halves of the wave), split: channel k < 3 is xo[k] - co[k] (the
// point's xyz row minus its group's centre row), channel k >= 3 is fo[(k - 3) * n] (fo = the object's channel-major
// features at the point), zero from CIN on.  Slots whose 8 channels are all features skip the per-lane decision.
template <class GEO>
__device__ __forceinline__ void gather_layer1(const float *fo, int n, const float *xo, const float *co, int h,
                                              bf16x8 (&a0h)[GEO::S1], bf16x8 (&a0l)[GEO::S1]) {
#pragma unroll
  for (int s = 0; s < GEO::S1; ++s) {
    f32x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = slot_channel16(s, e, h);
      float x;
      if (slot_channel16(s, e, 0) >= 3 && slot_channel16(s, e, 1) < GEO::CIN) {
        x = fo[(k - 3) * n];
      } else {
        x = 0.f;
        if (k < 3) x = xo[k] - co[k];
        else if (k < GEO::CIN) x = fo[(k - 3) * n];
      }
      v[e] = x;
    }
    split8(v, a0h[s], a0l[s]);
  }
}

// ReLU + hi/lo split of one 32-row output tile = two K steps of the next layer
__device__ __forceinline__ void split_tile(const f32x16 &acc, bf16x8 &h0, bf16x8 &l0, bf16x8 &h1, bf16x8 &l1) {
  f32x8 v0, v1;
#pragma unroll
  for (int e = 0; e < 8; ++e) { v0[e] = relu1(acc[e]); v1[e] = relu1(acc[8 + e]); }
  split8(v0, h0, l0);
  split8(v1, h1, l1);
}

// A last-layer tile whose 32 columns are ONE group: lane = output channel, registers (+ the other half of the wave) = the
// 32 samples -> max-pool = 15 in-lane max + one cross-half exchange
__device__ __forceinline__ float group_max(const f32x16 &acc) {
  float m0 = fmaxf(fmaxf(acc[0], acc[1]), fmaxf(acc[2], acc[3]));
  float m1 = fmaxf(fmaxf(acc[4], acc[5]), fmaxf(acc[6], acc[7]));
  float m2 = fmaxf(fmaxf(acc[8], acc[9]), fmaxf(acc[10], acc[11]));
  float m3 = fmaxf(fmaxf(acc[12], acc[13]), fmaxf(acc[14], acc[15]));
  const float m = fmaxf(fmaxf(m0, m1), fmaxf(m2, m3));
  return fmaxf(m, __shfl_xor(m, 32, 64));
}

// The three layers over one 32-column tile, stages 0 .. G-1 of round rd of the weight stream; the last layer runs in the
// transposed form (lane = output channel) and hands each of its M3 tiles to pool(acc, mt).
// Software pipeline: the post-processing (ReLU + hi/lo split, or the pooling) of output tile mt-1 is issued after the
// MFMAs of tile mt, in the same scheduling region, so that its VALU work runs in the shadow of the matrix pipe
// (independent registers).  Only the last tile of a layer is post-processed in the open (the next layer needs all of it).
// pool is taken by value and must capture by value: through references the compiler re-reads what it captured after
// every LDS atomic of the distinct form and works out the run masks again for each of the M3 tiles (measured at SA2 on
// the workload's clouds: 237 us against 228, profiles/r9/sa_mlp_refactor.txt).
template <class GEO, int NPROD, class STREAM, class POOL>
__device__ __forceinline__ void mlp_tile(const STREAM &ws, int rd, const bf16x8 (&a0h)[GEO::S1], const bf16x8 (&a0l)[GEO::S1],
                                         int lane, POOL pool) {
  constexpr int S1 = GEO::S1, S2 = GEO::S2, S3 = GEO::S3, M1 = GEO::M1, M2 = GEO::M2, M3 = GEO::M3;
  bf16x8 a1h[S2], a1l[S2], a2h[S3], a2l[S3];
  int g = 0;
  f32x16 prev;
#pragma unroll
  for (int mt = 0; mt < M1; ++mt, ++g) {
    const float *wt = ws.begin(rd, g);
    const f32x16 acc = mfma_tile16<S1, false, NPROD>(wt, a0h, a0l, lane);
    if (mt > 0) split_tile(prev, a1h[2 * mt - 2], a1l[2 * mt - 2], a1h[2 * mt - 1], a1l[2 * mt - 1]);
    prev = acc;
    ws.end();
  }
  split_tile(prev, a1h[2 * M1 - 2], a1l[2 * M1 - 2], a1h[2 * M1 - 1], a1l[2 * M1 - 1]);
#pragma unroll
  for (int mt = 0; mt < M2; ++mt, ++g) {
    const float *wt = ws.begin(rd, g);
    const f32x16 acc = mfma_tile16<S2, false, NPROD>(wt, a1h, a1l, lane);
    if (mt > 0) split_tile(prev, a2h[2 * mt - 2], a2l[2 * mt - 2], a2h[2 * mt - 1], a2l[2 * mt - 1]);
    prev = acc;
    ws.end();
  }
  split_tile(prev, a2h[2 * M2 - 2], a2l[2 * M2 - 2], a2h[2 * M2 - 1], a2l[2 * M2 - 1]);
  // unrolled for both kernels: rolled, the distinct form measured 770 us against 742 with every group full at SA2, and
  // the dense rows are within their spread either way (profiles/r9/sa_mlp_refactor.txt)
#pragma unroll
  for (int mt = 0; mt < M3; ++mt, ++g) {
    const float *wt = ws.begin(rd, g);
    const f32x16 acc = mfma_tile16<S3, true, NPROD>(wt, a2h, a2l, lane);
    if (mt > 0) pool(prev, mt - 1);
    prev = acc;
    ws.end();
  }
  pool(prev, M3 - 1);
}

// WAVES waves per workgroup (each owns one 32-sample group per round).  RESIDENT: the whole packed
// MLP fits in LDS next to the object -> loaded once per workgroup, no per-tile barriers; otherwise
// the 32-row weight tiles stream through a double buffer (one barrier per tile).  More waves per
// workgroup = more columns per streamed weight byte (the LDS-DMA weight stream, not the matrix pipe,
// bounds the streaming form: profiles/r1).
// PM: the features arrive point-major -- feats[(obj * n + p) * ld_feat + c], e.g. the rgb columns of an interleaved
// (B, N, 3 + C) cloud (pointer at column 3, ld_feat = 6) -- and are transposed into the channel-major LDS image while
// they are staged, instead of by a separate full-cloud transpose copy in HBM (63 us per step at SA1).
template <int CF, int C1, int C2, int C3, int WAVES, bool RESIDENT, bool PM = false, int NPROD = 3>
__global__ __launch_bounds__(WAVES * 64) void sa_mlp_x3_kernel(
    int b, int n, int npoint, const float *__restrict__ xyz, const float *__restrict__ new_xyz,
    const float *__restrict__ feats, const int32_t *__restrict__ idx,
    const float *__restrict__ wpack, float *__restrict__ out, int ld_feat, const int *__restrict__ n_obj_dev) {
  if (n_obj_dev && (int)blockIdx.x >= *n_obj_dev) return;      // object extent: nothing read or written
  using GEO = Geometry16<CF, C1, C2, C3>;
  constexpr int BLOCK = WAVES * 64;

  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Layout<GEO, RESIDENT, 1, false, int> L(n, npoint);
  float *s_out = lds + L.out, *s_feat = lds + L.feat, *s_xyz = lds + L.xyz, *s_ctr = lds + L.ctr;
  int32_t *s_idx = reinterpret_cast<int32_t *>(lds + L.idx);

  const int obj = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 31, h = lane >> 5;
  stage_objects<CF, PM, 1, BLOCK>(obj, 1, n, npoint, xyz, new_xyz, feats, idx, ld_feat, s_feat, s_xyz, s_ctr, s_idx, tid);
  const WeightStream<GEO, WAVES, RESIDENT> ws{wpack, lds, wave, lane};
  ws.first();
  tile_copy_wait();
  __syncthreads();

  const int rounds = (npoint + WAVES - 1) / WAVES;
  for (int rd = 0; rd < rounds; ++rd) {
    const int tile = rd * WAVES + wave;
    const bool live = tile < npoint;
    const int j = live ? tile : npoint - 1;

    bf16x8 a0h[GEO::S1], a0l[GEO::S1];
    const int p = s_idx[j * kNS + col];
    gather_layer1<GEO>(s_feat + p, n, s_xyz + p * 3, s_ctr + j * 3, h, a0h, a0l);
    mlp_tile<GEO, NPROD>(ws, rd, a0h, a0l, lane, [=](const f32x16 &acc, int mt) {
      const float m = group_max(acc);
      if (lane < 32 && live) s_out[(mt * 32 + lane) * npoint + tile] = fmaxf(m, 0.f);   // ReLU after the max
    });
  }
  if (RESIDENT) __syncthreads();
  copy_out_dense<BLOCK>(s_out, out + (size_t)obj * C3 * npoint, C3 * npoint, tid);
}

// ------------------------------------------------------------------------------------------
// Distinct-sample form (default; gps_sa_mlp_set_distinct).  gps_ball_query fills the slots of a group past the points
// it found with the group's first hit, so slot c > 0 with idx[c] == idx[0] is the same point, the same centre and the
// same MLP column as slot 0: the max-pool cannot see it.  The rule is applied to whatever idx holds (it does not assume
// that the kept slots form a prefix), so the pooled features are those of the dense kernel above for any idx.
// The kernel is the dense one -- the same Geometry, stage_objects, WeightStream, gather_layer1 and mlp_tile -- with another
// choice of columns and another pooling; what is its own:
//   * after staging, the workgroup builds in LDS the list of kept (group, point) columns, group after group (scan_groups:
//     ballot + prefix count per group; one prefix sum over the groups); one tile = 32 consecutive list entries, and
//     gather_layer1 is given the entry's own point and its own group's centre; tiles past the end of the list are not
//     computed (a wave without a tile only keeps the weight stream's copies and barriers going), lanes past the end of
//     the last tile repeat the last entry and are not pooled;
//   * a group's columns may straddle tiles and waves: a tile of 32 columns of ONE group is pooled like a dense tile
//     (group_max); otherwise each lane keeps a running max over its registers' runs of equal group (rkey, cut).  Either
//     way a maximum is folded into the group's pooled row with an LDS integer max on the bit pattern (rows start at +0,
//     which is also the ReLU after the max; max is order-independent, so the result is deterministic; on the bit pattern
//     a positive NaN is the largest value and is kept, where the dense form's fmaxf drops it).  The pooled
//     rows are kept [group][channel] with a pitch of C3 + 1 words: conflict-free for the lanes (= channels) of a fold
//     and for the transposing copy-out;
//   * OBJS > 1 (streamed weights, SA2): a workgroup takes OBJS consecutive objects and ONE list over them, so that a
//     streamed weight tile feeds up to WAVES tiles of columns although one object has about three; objects past the
//     device-side extent are neither read nor written.
// ------------------------------------------------------------------------------------------
#ifndef GPS_SA2_OBJS
#define GPS_SA2_OBJS 3   // objects per workgroup of the streamed form (LDS admits 1..3 at n = 32, npoint = 16)
#endif

template <int CF, int C1, int C2, int C3, int WAVES, bool RESIDENT, bool PM, int NPROD, int OBJS>
__global__ __launch_bounds__(WAVES * 64) void sa_mlp_x3_distinct_kernel(
    int b, int n, int npoint, const float *__restrict__ xyz, const float *__restrict__ new_xyz,
    const float *__restrict__ feats, const int32_t *__restrict__ idx,
    const float *__restrict__ wpack, float *__restrict__ out, int ld_feat, const int *__restrict__ n_obj_dev) {
  int n_obj = b;
  if (n_obj_dev) { const int ext = *n_obj_dev; n_obj = ext < b ? ext : b; }
  const int obj0 = blockIdx.x * OBJS;
  if (obj0 >= n_obj) return;                                   // object extent: nothing read or written
  const int nobj = n_obj - obj0 < OBJS ? n_obj - obj0 : OBJS;  // objects of this workgroup
  using GEO = Geometry16<CF, C1, C2, C3>;
  using LAYOUT = Layout<GEO, RESIDENT, OBJS, true, int>;
  constexpr int BLOCK = WAVES * 64;
  constexpr int OLD = LAYOUT::OLD;           // pitch of a pooled row

  extern __shared__ __attribute__((aligned(16))) float lds[];
  const LAYOUT L(n, npoint);
  int *s_out = reinterpret_cast<int *>(lds + L.out);            // bit patterns
  float *s_feat = lds + L.feat, *s_xyz = lds + L.xyz, *s_ctr = lds + L.ctr;
  int32_t *s_idx = reinterpret_cast<int32_t *>(lds + L.idx);
  int32_t *s_list = reinterpret_cast<int32_t *>(lds + L.list);
  int32_t *s_off = reinterpret_cast<int32_t *>(lds + L.off);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 31, h = lane >> 5;
  const int NG = nobj * npoint;              // groups of this workgroup

  const WeightStream<GEO, WAVES, RESIDENT> ws{wpack, lds, wave, lane};
  ws.first();
  stage_objects<CF, PM, OBJS, BLOCK>(obj0, nobj, n, npoint, xyz, new_xyz, feats, idx, ld_feat, s_feat, s_xyz, s_ctr, s_idx, tid);
  for (int e = tid; e < NG * OLD; e += BLOCK) s_out[e] = 0;
  __syncthreads();

  // ---- the kept columns: slot c > 0 of a group is dropped iff idx[c] == idx[0] -----------------------------------
  // a half wave per group; pass 0 counts, pass 1 writes the list at the group's offset
  auto scan_groups = [&](bool write) {
    for (int g0 = wave * 2; g0 < NG; g0 += WAVES * 2) {
      const int g = g0 + h;
      const bool valid = g < NG;
      const int p = valid ? s_idx[g * kNS + col] : 0;
      const int p0 = __shfl(p, h * 32, 64);
      const bool keep = valid && (col == 0 || p != p0);
      const unsigned int hm = (unsigned int)(__ballot(keep) >> (32 * h));
      if (!write) {
        if (col == 0 && valid) s_off[g] = __popc(hm);
      } else if (keep) {
        s_list[s_off[g] + __popc(hm & ((1u << col) - 1u))] = (g << 16) | (p & 0xFFFF);
      }
    }
  };
  scan_groups(false);
  __syncthreads();
  if (wave == 0) {                           // exclusive prefix sum of the counts, total in s_off[NG]
    int run = 0;
    for (int base = 0; base < NG; base += 64) {
      const bool in = base + lane < NG;
      const int c = in ? s_off[base + lane] : 0;
      int inc = c;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
      }
      if (in) s_off[base + lane] = run + inc - c;
      run += __shfl(inc, 63, 64);
    }
    if (lane == 0) s_off[NG] = run;
  }
  __syncthreads();
  scan_groups(true);
  tile_copy_wait();
  __syncthreads();

  const int total = __builtin_amdgcn_readfirstlane(s_off[NG]);   // >= NG: slot 0 of a group is always kept
  const int ntiles = (total + 31) >> 5;
  const int rounds = (ntiles + WAVES - 1) / WAVES;
  for (int rd = 0; rd < rounds; ++rd) {
    const int tile = rd * WAVES + wave;
    if (tile >= ntiles) {                    // wave-uniform: a wave without a tile only keeps the weight stream going
      if (RESIDENT) break;
      for (int g = 0; g < GEO::G; ++g) {     // the same copies and barriers as the waves that compute
        ws.begin(rd, g);
        ws.end();
      }
      continue;
    }

    bf16x8 a0h[GEO::S1], a0l[GEO::S1];
    // pooled layer: accumulator register r of this lane holds column cbase + (r & 3) + 8 * (r >> 2) of the list
    unsigned int cut = 0;                    // bit r: that column may be of another group than register r - 1's (or is past the end)
    int rkey[16];                            // group of register r's column, -1 past the end of the list
    int g_first;                             // group of the tile's first column
    bool uni;                                // the tile is 32 columns of ONE group: pooled like a dense tile
    {
      const int ei = tile * kNS + col < total ? tile * kNS + col : total - 1;
      const int ent = s_list[ei];
      const int j = ent >> 16, p = ent & 0xFFFF;                 // j = o * npoint + group of the object
      const int o = OBJS > 1 ? j / npoint : 0;
      gather_layer1<GEO>(s_feat + o * CF * n + p, n, s_xyz + (o * n + p) * 3, s_ctr + j * 3, h, a0h, a0l);
      // where the group changes along the tile: one ballot over the columns (= lanes), no LDS traffic
      const int key = tile * kNS + col < total ? j : -1;
      const int left = __shfl_up(key, 1, 64);
      const unsigned int edges = (unsigned int)__ballot(col > 0 && key != left);     // bit c: column c starts a run
      g_first = __builtin_amdgcn_readfirstlane(j);
      uni = edges == 0 && tile * kNS + kNS - 1 < total;
#pragma unroll
      for (int r = 0; r < 16; ++r) {         // every lane active here: the key of column c + 4 h sits in that lane
        const int c = (r & 3) + 8 * (r >> 2);
        const int k0 = __builtin_amdgcn_readlane(key, c), k1 = __builtin_amdgcn_readlane(key, c + 4);
        rkey[r] = h ? k1 : k0;
      }
      const unsigned int eh = edges >> (4 * h);
#pragma unroll
      for (int r = 1; r < 16; ++r) {
        // register r - 1 holds the column before this one, or (r & 3 == 0) the one five before it
        const unsigned int m = (r & 3) ? (eh >> ((r & 3) + 8 * (r >> 2))) & 1u : (eh >> (8 * (r >> 2) - 4)) & 0x1Fu;
        if (m) cut |= 1u << r;
      }
    }
    mlp_tile<GEO, NPROD>(ws, rd, a0h, a0l, lane, [=](const f32x16 &acc, int mt) {
      int *row = s_out + mt * 32 + col;
      if (uni) {
        const float m = group_max(acc);
        if (lane < 32) atomicMax(row + g_first * OLD, __float_as_int(m));
        return;
      }
      auto fold = [&](int r, float m) {      // the run that ends with register r -> its group's pooled row
        if (rkey[r] >= 0) atomicMax(row + rkey[r] * OLD, __float_as_int(m));
      };
      float m = acc[0];
#pragma unroll
      for (int r = 1; r < 16; ++r) {
        if ((cut >> r) & 1u) {
          fold(r - 1, m);
          m = acc[r];
        } else {
          m = fmaxf(m, acc[r]);
        }
      }
      fold(15, m);
    });
  }
  __syncthreads();
  // ---- pooled rows out: (object, channel, group) in HBM, [group][channel] here ----------------------------------
  float *go = out + (size_t)obj0 * C3 * npoint;
  const int words = nobj * C3 * npoint;
  if ((npoint & 3) == 0) {
    float4 *g4 = reinterpret_cast<float4 *>(go);
    for (int e4 = tid; e4 < words >> 2; e4 += BLOCK) {
      const int e = e4 << 2, oc = e / npoint, j = e - oc * npoint;     // oc = o * C3 + c
      const int o = OBJS > 1 ? oc / C3 : 0, c = oc - o * C3;
      const int *src = s_out + (o * npoint + j) * OLD + c;
      g4[e4] = make_float4(__int_as_float(src[0]), __int_as_float(src[OLD]), __int_as_float(src[2 * OLD]),
                           __int_as_float(src[3 * OLD]));
    }
  } else {
    for (int e = tid; e < words; e += BLOCK) {
      const int oc = e / npoint, j = e - oc * npoint;
      const int o = OBJS > 1 ? oc / C3 : 0, c = oc - o * C3;
      go[e] = __int_as_float(s_out[(o * npoint + j) * OLD + c]);
    }
  }
}

static int g_products = 3;      // 3 = split-bf16 triple product (fp32-accurate, default); 1 = single bf16 product (opt-in)
// 0 = every launch runs the MLP on all 32 slots; 1 (default) = the streamed-weight form (SA2) runs it on each group's distinct
// samples only; 2 = so does the resident-weight form (SA1), where it measured slower than the dense kernel
// (profiles/r8/sa_distinct_bench.txt)
static int g_distinct = 1;

template <int CF, int C1, int C2, int C3, int WAVES, bool RESIDENT, bool PM, int NPROD>
int launch_sa_x3_n(int b, int n, int npoint, const float *xyz, const float *new_xyz, const float *feats,
                   const int32_t *idx, const float *wpack, float *out, hipStream_t s, int ld_feat) {
  const size_t lds = Layout<Geometry16<CF, C1, C2, C3>, RESIDENT, 1, false, size_t>(n, npoint).bytes();
  if (lds > 160 * 1024) return GPS_ERR_UNSUPPORTED;
  static gps_dev::PerDevice<size_t, 1> granted;
  const int st = gps_dev::grant_lds(reinterpret_cast<const void *>(&sa_mlp_x3_kernel<CF, C1, C2, C3, WAVES, RESIDENT, PM, NPROD>),
                                    lds, lds, granted.row()[0]);
  if (st != GPS_OK) return st;
  hipLaunchKernelGGL((sa_mlp_x3_kernel<CF, C1, C2, C3, WAVES, RESIDENT, PM, NPROD>), dim3(b), dim3(WAVES * 64), lds, s, b, n,
                     npoint, xyz, new_xyz, feats, idx, wpack, out, ld_feat, gps::object_extent());
  return GPS_OK;
}

// OBJS objects per workgroup when LDS admits them, else fewer; shapes the distinct form cannot hold (its column list and
// pooled-row pitch need more LDS than the dense form; point / group ids are packed in 16 + 15 bits) run the dense kernel
template <int CF, int C1, int C2, int C3, int WAVES, bool RESIDENT, bool PM, int NPROD, int OBJS>
int launch_sa_x3_distinct(int b, int n, int npoint, const float *xyz, const float *new_xyz, const float *feats,
                          const int32_t *idx, const float *wpack, float *out, hipStream_t s, int ld_feat) {
  const size_t lds = Layout<Geometry16<CF, C1, C2, C3>, RESIDENT, OBJS, true, size_t>(n, npoint).bytes();
  if (lds > 160 * 1024 || n > 0xFFFF || (long long)OBJS * npoint > 0x7FFF) {
    if constexpr (OBJS > 1)
      return launch_sa_x3_distinct<CF, C1, C2, C3, WAVES, RESIDENT, PM, NPROD, OBJS - 1>(b, n, npoint, xyz, new_xyz, feats, idx,
                                                                                         wpack, out, s, ld_feat);
    else
      return launch_sa_x3_n<CF, C1, C2, C3, WAVES, RESIDENT, PM, NPROD>(b, n, npoint, xyz, new_xyz, feats, idx, wpack, out, s, ld_feat);
  }
  static gps_dev::PerDevice<size_t, 1> granted;
  const int st = gps_dev::grant_lds(reinterpret_cast<const void *>(&sa_mlp_x3_distinct_kernel<CF, C1, C2, C3, WAVES, RESIDENT, PM, NPROD, OBJS>),
                                    lds, lds, granted.row()[0]);
  if (st != GPS_OK) return st;
  hipLaunchKernelGGL((sa_mlp_x3_distinct_kernel<CF, C1, C2, C3, WAVES, RESIDENT, PM, NPROD, OBJS>), dim3((b + OBJS - 1) / OBJS),
                     dim3(WAVES * 64), lds, s, b, n, npoint, xyz, new_xyz, feats, idx, wpack, out, ld_feat, gps::object_extent());
  return GPS_OK;
}

template <int CF, int C1, int C2, int C3, int WAVES, bool RESIDENT, bool PM = false>
int launch_sa_x3(int b, int n, int npoint, const float *xyz, const float *new_xyz, const float *feats,
                 const int32_t *idx, const float *wpack, float *out, hipStream_t s, int ld_feat = 0) {
  if (g_distinct >= (RESIDENT ? 2 : 1)) {
    constexpr int OBJS = RESIDENT ? 1 : GPS_SA2_OBJS;
    return g_products == 1
               ? launch_sa_x3_distinct<CF, C1, C2, C3, WAVES, RESIDENT, PM, 1, OBJS>(b, n, npoint, xyz, new_xyz, feats, idx, wpack, out, s, ld_feat)
               : launch_sa_x3_distinct<CF, C1, C2, C3, WAVES, RESIDENT, PM, 3, OBJS>(b, n, npoint, xyz, new_xyz, feats, idx, wpack, out, s, ld_feat);
  }
  return g_products == 1
             ? launch_sa_x3_n<CF, C1, C2, C3, WAVES, RESIDENT, PM, 1>(b, n, npoint, xyz, new_xyz, feats, idx, wpack, out, s, ld_feat)
             : launch_sa_x3_n<CF, C1, C2, C3, WAVES, RESIDENT, PM, 3>(b, n, npoint, xyz, new_xyz, feats, idx, wpack, out, s, ld_feat);
}

}  // namespace x3

}  // namespace gps_sa

extern "C" {

long long gps_sa_mlp_layer_floats(int c_in, int c_out) {
  if (c_in < 1 || c_out < 32 || (c_out & 31)) return -1;
  return (long long)(c_out / 32) * gps_sa::tile_floats(c_in);
}

long long gps_sa_mlp_wpack_floats(int c_in, int c1, int c2, int c3) {
  if (c_in < 1 || c1 < 32 || c2 < 32 || c3 < 32 || (c1 & 31) || (c2 & 31) || (c3 & 31)) return -1;
  return gps_sa_mlp_layer_floats(c_in, c1) + gps_sa_mlp_layer_floats(c1, c2) + gps_sa_mlp_layer_floats(c2, c3);
}

int gps_sa_mlp_pack_layer(int c_in, int c_out, const float *w, const float *shift, float *dst,
                          gps_stream_t stream) {
  if (c_in < 1 || c_out < 32 || (c_out & 31) || !w || !shift || !dst) return GPS_ERR_INVALID_ARGUMENT;
  const int total = (int)gps_sa_mlp_layer_floats(c_in, c_out);
  hipLaunchKernelGGL(gps_sa::pack_layer_kernel, dim3((total + 255) / 256), dim3(256), 0,
                     (hipStream_t)stream, c_in, c_out, w, shift, dst);
  return hipGetLastError() == hipSuccess ? GPS_OK : GPS_ERR_LAUNCH;
}

int gps_sa_mlp_set_products(int n) {
  const int was = gps_sa::x3::g_products;
  if (n == 1 || n == 3) gps_sa::x3::g_products = n;
  return was;
}

int gps_sa_mlp_set_distinct(int on) {
  const int was = gps_sa::x3::g_distinct;
  if (on >= 0 && on <= 2) gps_sa::x3::g_distinct = on;
  return was;
}

long long gps_sa_mlp_layer_floats_bf16x3(int c_in, int c_out) {
  if (c_in < 1 || c_out < 32 || (c_out & 31)) return -1;
  return (long long)(c_out / 32) * gps_sa::x3::tile_floats16(c_in);
}

int gps_sa_mlp_pack_layer_bf16x3(int c_in, int c_out, const float *w, const float *shift, float *dst,
                                 gps_stream_t stream) {
  if (c_in < 1 || c_out < 32 || (c_out & 31) || !w || !shift || !dst) return GPS_ERR_INVALID_ARGUMENT;
  const int total = (int)gps_sa_mlp_layer_floats_bf16x3(c_in, c_out);
  hipLaunchKernelGGL(gps_sa::x3::pack_layer16_kernel, dim3((total + 255) / 256), dim3(256), 0,
                     (hipStream_t)stream, c_in, c_out, w, shift, dst);
  return hipGetLastError() == hipSuccess ? GPS_OK : GPS_ERR_LAUNCH;
}

int gps_sa_mlp_forward_bf16x3(int b, int n, int npoint, int nsample, int c_feat, int c1, int c2, int c3,
                              const float *xyz, const float *new_xyz, const float *features,
                              const int32_t *idx, const float *wpack, float *out, gps_stream_t stream) {
  if (b < 0 || n < 1 || npoint < 1 || nsample < 1 || c_feat < 0) return GPS_ERR_INVALID_ARGUMENT;
  if (b == 0) return GPS_OK;
  if (!xyz || !new_xyz || !idx || !wpack || !out || (c_feat > 0 && !features))
    return GPS_ERR_INVALID_ARGUMENT;
  if (nsample != gps_sa::kNS) return GPS_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  int st = GPS_ERR_UNSUPPORTED;
  if (c_feat == 3 && c1 == 64 && c2 == 64 && c3 == 128)
    st = gps_sa::x3::launch_sa_x3<3, 64, 64, 128, GPS_SA1_WAVES, true>(b, n, npoint, xyz, new_xyz, features, idx,
                                                                      wpack, out, s);
  else if (c_feat == 128 && c1 == 128 && c2 == 128 && c3 == 256)
    st = gps_sa::x3::launch_sa_x3<128, 128, 128, 256, GPS_SA2_WAVES, false>(b, n, npoint, xyz, new_xyz, features,
                                                                            idx, wpack, out, s);
  if (st != GPS_OK) return st;
  return hipGetLastError() == hipSuccess ? GPS_OK : GPS_ERR_LAUNCH;
}

int gps_sa_mlp_forward_bf16x3_pm(int b, int n, int npoint, int nsample, int c_feat, int c1, int c2, int c3,
                                 const float *xyz, const float *new_xyz, const float *features_pm, long long ld_feat,
                                 const int32_t *idx, const float *wpack, float *out, gps_stream_t stream) {
  if (b < 0 || n < 1 || npoint < 1 || nsample < 1 || c_feat < 1 || ld_feat < c_feat || ld_feat > 0x7FFFFFFF)
    return GPS_ERR_INVALID_ARGUMENT;
  if (b == 0) return GPS_OK;
  if (!xyz || !new_xyz || !idx || !wpack || !out || !features_pm) return GPS_ERR_INVALID_ARGUMENT;
  if (nsample != gps_sa::kNS) return GPS_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  int st = GPS_ERR_UNSUPPORTED;
  if (c_feat == 3 && c1 == 64 && c2 == 64 && c3 == 128)
    st = gps_sa::x3::launch_sa_x3<3, 64, 64, 128, GPS_SA1_WAVES, true, true>(b, n, npoint, xyz, new_xyz, features_pm, idx,
                                                                            wpack, out, s, (int)ld_feat);
  if (st != GPS_OK) return st;
  return hipGetLastError() == hipSuccess ? GPS_OK : GPS_ERR_LAUNCH;
}

int gps_sa_mlp_forward(int b, int n, int npoint, int nsample, int c_feat, int c1, int c2, int c3,
                       const float *xyz, const float *new_xyz, const float *features,
                       const int32_t *idx, const float *wpack, float *out, gps_stream_t stream) {
  if (b < 0 || n < 1 || npoint < 1 || nsample < 1 || c_feat < 0) return GPS_ERR_INVALID_ARGUMENT;
  if (b == 0) return GPS_OK;
  if (!xyz || !new_xyz || !idx || !wpack || !out || (c_feat > 0 && !features))
    return GPS_ERR_INVALID_ARGUMENT;
  if (nsample != gps_sa::kNS) return GPS_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  int st = GPS_ERR_UNSUPPORTED;
  if (c_feat == 3 && c1 == 64 && c2 == 64 && c3 == 128)
    st = gps_sa::launch_sa<3, 64, 64, 128>(b, n, npoint, xyz, new_xyz, features, idx, wpack, out, s);
  else if (c_feat == 128 && c1 == 128 && c2 == 128 && c3 == 256)
    st = gps_sa::launch_sa<128, 128, 128, 256>(b, n, npoint, xyz, new_xyz, features, idx, wpack, out, s);
  if (st != GPS_OK) return st;
  return hipGetLastError() == hipSuccess ? GPS_OK : GPS_ERR_LAUNCH;
}

}  // extern "C"
