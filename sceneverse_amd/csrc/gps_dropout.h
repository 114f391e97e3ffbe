// Internal (not installed): the counter-based dropout stream of the library, defined once.
//
// The contract: the same (seed, index) gives the same 32 bits in forward and backward, in every kernel of every file
// -- masks are never stored, the backward pass recomputes them, and it may run on another kernel family than the
// forward did (the plain attention core: gps_attention.hip, _ex, _fa and _sp are mixed by the default dispatch).  An
// element is kept iff its bits are >= the threshold p * 2^32 (drop_threshold), so the keep rate is 1 - p.
//   * the hash is a 32-bit avalanche function (two multiplies, three xor-shifts; "lowbias32" constants) of the index
//     folded with the seed; the seed part (seed_fold) is wave-uniform and runs on the scalar unit;
//   * the seed is `seed` plus an optional device word (effective_seed): HIP-graph replays get fresh masks by advancing
//     that word on the device;
//   * element stream (rng_u32): one hash per element, index = the element's linear index (LayerNorm, GEMM epilogues,
//     the BERT embedding, the whole-sequence attention kernels);
//   * pair stream (pair_rng / pair_keep): one hash per pair of adjacent keys (t even, t odd) of a query, its low / high
//     16 bits decide the two elements against the threshold's upper 16 bits (the drop probability is quantised to
//     1 / 65536); index of the pair = (row base + key) / 2 with an even row pitch, so that the lane holding keys
//     4 g + 0..3 of a query needs two hashes (the streaming, block-streaming and K / V-resident attention kernels).
//   * consumers of the element stream carry (threshold, scale, seed) as a Drop and apply it through drop_factor /
//     drop_factor4 / keep_mask4 / drop4 (the LayerNorm, the grounding head tail, the BERT embedding).
// tests/test_dropout_hash.py emulates mix32 / rng_u32 in numpy.
#pragma once
#include <hip/hip_runtime.h>

namespace gps_dropout {

__device__ __forceinline__ unsigned int mix32(unsigned int x) {
  x ^= x >> 16;
  x *= 0x21F0AAADu;
  x ^= x >> 15;
  x *= 0x735A2D97u;
  x ^= x >> 15;
  return x;
}
__device__ __forceinline__ unsigned int seed_fold(unsigned long long seed) {      // wave-uniform
  return mix32((unsigned int)seed ^ mix32((unsigned int)(seed >> 32) + 0x9E3779B9u));
}
// the two fields of a kernel's parameter struct, by reference: the kernels were written against a helper that took the
// struct, and by-value arguments change the register allocation of some of them (attn_bwd_stream_kernel, attn_f32_bwd_kernel)
__device__ __forceinline__ unsigned long long effective_seed(const unsigned long long &seed, const unsigned long long *const &seed_dev) {
  return seed + (seed_dev ? *seed_dev : 0ull);
}
__device__ __forceinline__ unsigned int rng_u32(unsigned long long seed, unsigned long long idx) {
  return mix32(((unsigned int)idx + (unsigned int)(idx >> 32) * 0x85EBCA6Bu) ^ seed_fold(seed));
}
__device__ __forceinline__ unsigned int pair_rng(unsigned int seedmix, unsigned int row_pair_base, int t) {
  return mix32((row_pair_base + (unsigned int)(t >> 1)) ^ seedmix);
}
__device__ __forceinline__ bool pair_keep(unsigned int r, int t, unsigned int thr16) {
  return ((t & 1) ? (r >> 16) : (r & 0xFFFFu)) >= thr16;
}

// element-stream dropout of a kernel, as its consumers carry it.  A kernel keeps its arithmetic form: drop4 is
// `keep ? h * scale : 0`, not `h * factor` (the two differ for non-finite h).
struct Drop {
  unsigned int thr;          // keep iff rng >= thr; 0 = no dropout
  float scale;               // 1 / (1 - p)
  unsigned long long seed;
};
// factor of element e: 0 (dropped) or 1 / (1 - p); 1 without dropout
__device__ __forceinline__ float drop_factor(const Drop &dr, unsigned long long e) {
  if (dr.thr == 0u) return 1.f;
  return rng_u32(dr.seed, e) >= dr.thr ? dr.scale : 0.f;
}
// the factors of the 4 elements starting at e0
__device__ __forceinline__ float4 drop_factor4(const Drop &d, unsigned long long e0) {
  if (d.thr == 0u) return make_float4(1.f, 1.f, 1.f, 1.f);
  return make_float4(rng_u32(d.seed, e0 + 0) >= d.thr ? d.scale : 0.f, rng_u32(d.seed, e0 + 1) >= d.thr ? d.scale : 0.f,
                     rng_u32(d.seed, e0 + 2) >= d.thr ? d.scale : 0.f, rng_u32(d.seed, e0 + 3) >= d.thr ? d.scale : 0.f);
}
// bit j set = element e0 + j is kept (all four when there is no dropout)
__device__ __forceinline__ unsigned int keep_mask4(const Drop &d, unsigned long long e0) {
  if (d.thr == 0u) return 15u;
  return (rng_u32(d.seed, e0 + 0) >= d.thr ? 1u : 0u) | (rng_u32(d.seed, e0 + 1) >= d.thr ? 2u : 0u) |
         (rng_u32(d.seed, e0 + 2) >= d.thr ? 4u : 0u) | (rng_u32(d.seed, e0 + 3) >= d.thr ? 8u : 0u);
}
// dropout applied to 4 values
__device__ __forceinline__ float4 drop4(float4 h, const Drop &d, unsigned long long e0) {
  if (d.thr == 0u) return h;
  h.x = rng_u32(d.seed, e0 + 0) >= d.thr ? h.x * d.scale : 0.f;
  h.y = rng_u32(d.seed, e0 + 1) >= d.thr ? h.y * d.scale : 0.f;
  h.z = rng_u32(d.seed, e0 + 2) >= d.thr ? h.z * d.scale : 0.f;
  h.w = rng_u32(d.seed, e0 + 3) >= d.thr ? h.w * d.scale : 0.f;
  return h;
}

// host: keep iff rng >= drop_threshold(p); 0 = no dropout
inline unsigned int drop_threshold(float p) { return p > 0.f ? (unsigned int)((double)p * 4294967296.0) : 0u; }

}  // namespace gps_dropout
