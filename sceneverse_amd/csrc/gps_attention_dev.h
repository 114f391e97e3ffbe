// Internal (not installed): device helpers shared by the bf16 attention kernels (gps_attention.hip, _fa, _sp, _spl; the
// fp32 / fp8 kernels of _ex take the workgroup mapping and the lane-group reductions).  MFMA fragment conventions of
// v_mfma_f32_16x16x32_bf16 with lane = (m = lane & 15, g = lane >> 4): an A / B operand holds 8 bf16 of row / column m,
// a D fragment holds rows 4 g + 0..3 of column m.  Every helper is __forceinline__: a kernel compiles to the same
// instructions as with a private copy (tools/asm_audit.py --digest shows it).  pack2 / bf2f are the library's one pair
// (gps_dev.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gps_dev.h"

namespace gps_attn_dev {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;

constexpr int DH = 64;                           // head width (the only one the GPS configs use)
constexpr int KS = DH + 8;                       // LDS row pitch of row-major Q / K / V / dO tiles, bf16 elements (144 B: conflict-free b128)
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;
constexpr float kC = 0.125f * kLog2e;            // base-2 logit per unit of q . k
constexpr float kClamp2 = -19.931568569324174f;  // log2(1e-6)

using gps_dev::bf2f;
using gps_dev::pack2;       // v_cvt_pk_bf16_f32: round to nearest even
__device__ __forceinline__ bf16x8 as_frag(u32x4 v) { return __builtin_bit_cast(bf16x8, v); }
__device__ __forceinline__ u32x4 zero4() { u32x4 z = {0u, 0u, 0u, 0u}; return z; }
__device__ __forceinline__ f32x4 zero_acc() { f32x4 z = {0.f, 0.f, 0.f, 0.f}; return z; }
__device__ __forceinline__ f32x4 mfma32(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
// pack the D fragments of two adjacent 16-row tiles into one A fragment: K order 32 c + 4 g + 0..3, 32 c + 16 + 4 g + 0..3
__device__ __forceinline__ bf16x8 pack_tiles(const f32x4 &a, const f32x4 &b) {
  const u32x4 v = {pack2(a[0], a[1]), pack2(a[2], a[3]), pack2(b[0], b[1]), pack2(b[2], b[3])};
  return as_frag(v);
}
__device__ __forceinline__ u32x2 pack_tile(const f32x4 &a) {
  const u32x2 v = {pack2(a[0], a[1]), pack2(a[2], a[3])};
  return v;
}
__device__ __forceinline__ float xor_max_g(float v) {   // across the 4 lane groups (same lane & 15)
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float xor_sum_g(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

// hardware-transposed read (ds_read_b64_tr_b16): the 16-lane group of `lane` gets rows row0 .. row0 + 3 of columns
// col0 .. col0 + 15 of a row-major bf16 tile, lane i (= lane & 15) receiving column col0 + i (4 values = 2 dwords)
__device__ __forceinline__ u32x2 tr4(const uint16_t *tile, int pitch, int row0, int col0, int lane) {
  const int i = lane & 15;
  const uint16_t *p = tile + (row0 + (i >> 2)) * pitch + col0 + 4 * (i & 3);
  const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)p);
  return __builtin_bit_cast(u32x2, v);
}
// MFMA operand (A: row = lane & 15 of M^T; B: column = lane & 15 of M) holding M[rows][col0 + (lane & 15)] for the eight rows
//   permuted:  32 c + 4 g + 0..3, 32 c + 16 + 4 g + 0..3   (the K order of pack_tiles)
//   natural:   32 c + 8 g + 0..7
__device__ __forceinline__ bf16x8 tr_frag_perm(const uint16_t *tile, int pitch, int c, int col0, int lane) {
  const int g = lane >> 4;
  const u32x2 lo = tr4(tile, pitch, 32 * c + 4 * g, col0, lane), hi = tr4(tile, pitch, 32 * c + 16 + 4 * g, col0, lane);
  const u32x4 v = {lo[0], lo[1], hi[0], hi[1]};
  return as_frag(v);
}
__device__ __forceinline__ bf16x8 tr_frag_nat(const uint16_t *tile, int pitch, int c, int col0, int lane) {
  const int g = lane >> 4;
  const u32x2 lo = tr4(tile, pitch, 32 * c + 8 * g, col0, lane), hi = tr4(tile, pitch, 32 * c + 8 * g + 4, col0, lane);
  const u32x4 v = {lo[0], lo[1], hi[0], hi[1]};
  return as_frag(v);
}
// one 16-byte fragment load: row `row` (pitch ld elements) of a bf16 matrix whose head block starts at `base` (uniform)
__device__ __forceinline__ u32x4 load_frag(const uint16_t *base, int row, int ld, int col) {
  return *reinterpret_cast<const u32x4 *>(reinterpret_cast<const char *>(base) + (unsigned int)(row * ld + col) * 2u);
}

// one workgroup per (scene, head): with B a multiple of 8 the heads of a scene run on one XCD (block id mod 8) and
// share what they all read (the pairwise tensor / planes) in that XCD's L2, scenes spread over the XCDs
__device__ __forceinline__ void block_to_bh(int B, int H, int &b, int &h) {
  const int id = blockIdx.x;
  if ((B & 7) == 0) {
    const int xcd = id & 7, slot = id >> 3;
    b = (slot / H) * 8 + xcd;
    h = slot % H;
  } else {
    b = id / H;
    h = id % H;
  }
}

// one 64-row block of two bf16 matrices (head h's 64 columns; rows >= rows_valid zero) -> two LDS tiles [64][KS], by a
// workgroup of kStreamThreads (the block-streaming families): issue() requests the four 16-byte pieces of a thread,
// commit() writes them
constexpr int kStreamThreads = 256;
struct BlockPair {
  u32x4 va[2], vb[2];
  __device__ __forceinline__ void issue(const uint16_t *src_a, int ld_a, const uint16_t *src_b, int ld_b, int row_first, int rows_valid) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int e = threadIdx.x + i * kStreamThreads, r = row_first + (e >> 3), ch = e & 7;
      va[i] = zero4();
      vb[i] = zero4();
      if (r < rows_valid) {
        va[i] = *reinterpret_cast<const u32x4 *>(reinterpret_cast<const char *>(src_a) + (unsigned int)(r * ld_a + ch * 8) * 2u);
        vb[i] = *reinterpret_cast<const u32x4 *>(reinterpret_cast<const char *>(src_b) + (unsigned int)(r * ld_b + ch * 8) * 2u);
      }
    }
  }
  __device__ __forceinline__ void commit(uint16_t *dst_a, uint16_t *dst_b) const {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int e = threadIdx.x + i * kStreamThreads, r = e >> 3, ch = e & 7;
      *reinterpret_cast<u32x4 *>(dst_a + r * KS + ch * 8) = va[i];
      *reinterpret_cast<u32x4 *>(dst_b + r * KS + ch * 8) = vb[i];
    }
  }
};

// plane form of the spatial term, base 2.  -log2(e) * (bias, w_1..w_5) from the conditioning vector as loaded (six
// bf16 in three words): u = -log2(e) z is then five fmas, e = 2^u, and
//   log2(clamp(sigmoid z, 1e-6)) = max(-log2(1 + e), log2(1e-6))
__device__ __forceinline__ void cond_vector(const unsigned int (&raw)[3], float (&w)[6]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    w[2 * i] = -kLog2e * bf2f(raw[i] & 0xFFFFu);
    w[2 * i + 1] = -kLog2e * __uint_as_float(raw[i] & 0xFFFF0000u);
  }
}
__device__ __forceinline__ float spatial_bias2(float e) { return fmaxf(-__builtin_amdgcn_logf(1.f + e), kClamp2); }

}  // namespace gps_attn_dev
