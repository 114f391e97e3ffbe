// Internal (not installed): the device helpers every row-wise kernel file of the library needs, defined once -- wave
// reductions, bf16 / fp32 row access, the last-arrival hand-off between workgroups -- and the two host expressions every
// C entry point ends with.  A new kernel file includes this header instead of copying from a neighbour.  Every device
// helper is __forceinline__: a kernel compiles to the same instructions as with a private copy
// (tools/asm_audit.py --digest shows it, profiles/refactor_dev_helpers/).
// Type-specific folds stay with their kernels: Best (gps_refer.hip, gps_metrics.hip), the (max, sum) log-sum-exp merge
// (gps_losses.hip), the encoded min / max of gps_refer.hip, the double-precision sums of gps_objects.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gps_hip.h"

namespace gps_dev {

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;

// ---- wave reductions: the same value in all 64 lanes ------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// ---- fp32 -> bf16, two forms that are NOT interchangeable (different instructions, different NaN payloads): a kernel
// keeps the one it was written with
__device__ __forceinline__ uint32_t f2bf(float f) {                 // integer round to nearest even; NaN stays NaN
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
  u += 0x7fffu + ((u >> 16) & 1u);
  return u >> 16;
}
__device__ __forceinline__ uint16_t cvt_bf16(float f) {             // the (__bf16) cast: v_cvt_pk_bf16_f32
  return __builtin_bit_cast(uint16_t, (__bf16)f);
}
__device__ __forceinline__ unsigned int pack2(float lo, float hi) { // two casts in one word
  const bf16x2_t h = {(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(unsigned int, h);
}
__device__ __forceinline__ float bf2f(unsigned int bits16) { return __uint_as_float(bits16 << 16); }

// ---- 8 consecutive elements starting at element index `idx` (a multiple of 8 from a 16-byte aligned base) ------------
__device__ __forceinline__ void unpack8(const u32x4 q, float (&x)[8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    x[2 * i] = __uint_as_float(q[i] << 16);
    x[2 * i + 1] = __uint_as_float(q[i] & 0xFFFF0000u);
  }
}
// as they lie in memory: load() now, get() later (the loads of a row are issued together, converted at their first use)
template <bool BF16> struct Raw8;
template <> struct Raw8<true> {
  uint4 u;
  __device__ __forceinline__ void load(const void *base, size_t idx) {
    u = *reinterpret_cast<const uint4 *>(reinterpret_cast<const uint16_t *>(base) + idx);
  }
  __device__ __forceinline__ void get(float v[8]) const {
    v[0] = __uint_as_float(u.x << 16); v[1] = __uint_as_float(u.x & 0xffff0000u);
    v[2] = __uint_as_float(u.y << 16); v[3] = __uint_as_float(u.y & 0xffff0000u);
    v[4] = __uint_as_float(u.z << 16); v[5] = __uint_as_float(u.z & 0xffff0000u);
    v[6] = __uint_as_float(u.w << 16); v[7] = __uint_as_float(u.w & 0xffff0000u);
  }
};
template <> struct Raw8<false> {
  float4 a, b;
  __device__ __forceinline__ void load(const void *base, size_t idx) {
    const float4 *p = reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(base) + idx);
    a = p[0];
    b = p[1];
  }
  __device__ __forceinline__ void get(float v[8]) const {
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  }
};
template <bool BF16>
__device__ __forceinline__ void load8(const void *base, size_t idx, float v[8]) {
  Raw8<BF16> r;
  r.load(base, idx);
  r.get(v);
}
template <bool BF16>
__device__ __forceinline__ void store8(void *base, size_t idx, const float v[8]) {      // bf16: f2bf
  if constexpr (BF16) {
    uint4 u;
    u.x = f2bf(v[0]) | (f2bf(v[1]) << 16); u.y = f2bf(v[2]) | (f2bf(v[3]) << 16);
    u.z = f2bf(v[4]) | (f2bf(v[5]) << 16); u.w = f2bf(v[6]) | (f2bf(v[7]) << 16);
    *reinterpret_cast<uint4 *>(reinterpret_cast<uint16_t *>(base) + idx) = u;
  } else {
    float4 *p = reinterpret_cast<float4 *>(reinterpret_cast<float *>(base) + idx);
    p[0] = make_float4(v[0], v[1], v[2], v[3]);
    p[1] = make_float4(v[4], v[5], v[6], v[7]);
  }
}
template <bool BF16>
__device__ __forceinline__ float load1(const void *base, size_t idx) {
  if constexpr (BF16) return __uint_as_float((uint32_t) reinterpret_cast<const uint16_t *>(base)[idx] << 16);
  else return reinterpret_cast<const float *>(base)[idx];
}
template <bool BF16>
__device__ __forceinline__ void store1(void *base, size_t idx, float v) {
  if constexpr (BF16) reinterpret_cast<uint16_t *>(base)[idx] = (uint16_t)f2bf(v);
  else reinterpret_cast<float *>(base)[idx] = v;
}

// ---- 4 consecutive elements at p + e0 (float or bf16 rows by overload); bf16 stores use the cast form ----------------
template <typename T> struct Raw4 { using type = float4; };
template <> struct Raw4<uint16_t> { using type = uint2; };
__device__ __forceinline__ float4 load_raw(const float *p, size_t e0) { return *reinterpret_cast<const float4 *>(p + e0); }
__device__ __forceinline__ uint2 load_raw(const uint16_t *p, size_t e0) { return *reinterpret_cast<const uint2 *>(p + e0); }
__device__ __forceinline__ float4 to_f4(float4 v) { return v; }
__device__ __forceinline__ float4 to_f4(uint2 v) {
  return make_float4(__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xFFFF0000u),
                     __uint_as_float(v.y << 16), __uint_as_float(v.y & 0xFFFF0000u));
}
template <typename T> __device__ __forceinline__ float4 load4(const T *p, size_t e0) { return to_f4(load_raw(p, e0)); }
__device__ __forceinline__ void store4(float *p, size_t e0, float4 v) { *reinterpret_cast<float4 *>(p + e0) = v; }
__device__ __forceinline__ void store4(uint16_t *p, size_t e0, float4 v) {
  uint2 o;
  o.x = (unsigned int)cvt_bf16(v.x) | ((unsigned int)cvt_bf16(v.y) << 16);
  o.y = (unsigned int)cvt_bf16(v.z) | ((unsigned int)cvt_bf16(v.w) << 16);
  *reinterpret_cast<uint2 *>(p + e0) = o;
}

// loads above this line are issued before anything below it (the compiler otherwise sinks them next to their first use,
// i.e. behind the wave-uniform branches of the optional operands: one memory round trip per branch instead of one per row)
#define GPS_LOADS_ISSUED() asm volatile("" ::: "memory")

// ---- the last-arrival hand-off ----------------------------------------------------------------------------------------
// `count` producers (threads or workgroups) each write partial results, the LAST of them to arrive reads everybody's and
// finishes the sum in index order: no float atomics, and the result does not depend on the arrival order.
//   producer   publish() its values, then take_ticket() / arrive_and_last();
//   last one   (the call returned true) peek() at all of them.
// Why this is correct without L2 write-back / invalidate episodes (the kernel before leaves > 100 MB dirty, a release
// fence would flush it): publish() is an agent-scope relaxed atomic store, i.e. a write-through store (sc1) that does not
// linger in a cache of the writer; `s_waitcnt vmcnt(0)` returns once those stores are acknowledged, and only then is the
// ticket, an agent-scope read-modify-write, taken.  Whoever draws ticket count - 1 therefore drew it after every other
// producer's values had been written through; peek() is an agent-scope load (sc1), which is never served from a stale
// line of the reader's own caches.  The last arriver stores zero to the ticket word, so that the next launch finds it as
// the first one did.
// The caller guarantees: the ticket word is zero before the first launch, and at most one launch is in flight per ticket
// word (launches that share a word are ordered on one stream).
__device__ __forceinline__ void publish(float *p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float peek(const float *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void drain_stores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// the ticket itself, for a thread whose wave's publish()ed values have been drained: true for the last of `count`
__device__ __forceinline__ bool drained_ticket(unsigned int *ticket, unsigned int count) {
  const unsigned int t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const bool last = t == count - 1u;
  if (last) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return last;
}
// one thread: the values its own WAVE publish()ed are in memory (the wait is per wave), then the ticket
__device__ __forceinline__ bool take_ticket(unsigned int *ticket, unsigned int count) {
  drain_stores();
  return drained_ticket(ticket, count);
}
// one workgroup: every thread's publish()ed values are in memory (each wave drains its own before the barrier), then
// thread 0 takes the ticket: true in EVERY thread of the last of `count` workgroups to arrive (`flag` = one int of LDS)
__device__ __forceinline__ bool arrive_and_last(unsigned int *ticket, unsigned int count, int *flag) {
  drain_stores();
  __syncthreads();
  if (threadIdx.x == 0) *flag = drained_ticket(ticket, count) ? 1 : 0;
  __syncthreads();
  return *flag != 0;
}

// ---- host ---------------------------------------------------------------------------------------------------------------
inline int launch_status() { return hipGetLastError() == hipSuccess ? GPS_OK : GPS_ERR_LAUNCH; }
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace gps_dev
