// Internal (not installed): the run functions of the five attention files.  gps_attention.hip's run_ex checks the
// arguments of the C entry points and dispatches to the others; each takes checked arguments and launches its family.
#pragma once
#include <hip/hip_runtime.h>

#include "gps_hip.h"

namespace gps_attn {
int run_ex(const gps_attn_args *a, bool backward, hipStream_t s);       // gps_attention.hip
int run_f32(const gps_attn_args *a, bool backward, hipStream_t s);      // gps_attention_ex.hip
int run_fp8_forward(const gps_attn_args *a, hipStream_t s);             // gps_attention_ex.hip
int run_spatial_planes(const gps_attn_args *a, bool backward, hipStream_t s);   // gps_attention_sp.hip
int run_spatial_planes_long(const gps_attn_args *a, bool backward, hipStream_t s);   // gps_attention_spl.hip (L > 144)
int run_plain_blocks(const gps_attn_args *a, bool backward, hipStream_t s);     // gps_attention_fa.hip
int run_plain_fused_bwd(const gps_attn_args *a, hipStream_t s);                 // gps_attention_fa.hip (one launch)
int run_plain_resident(const gps_attn_args *a, bool backward, hipStream_t s);   // gps_attention_sp.hip
}  // namespace gps_attn
