// norm_apply.h -- one element of a norm's output, y = (s - mean) rstd gamma + beta, written once.
//
// add_layernorm_forward_kernel (layernorm.hip) stores it; tall_tn_partial (lora_side.hip) forms it in
// registers from the norm's input when a table gradient reads a norm output that was not kept
// (layers/tuning/recompute.py).  The two must give the same bits, so both call this: one subtraction,
// one product, one fused multiply-add.  LLaMA's RMS norm is the same expression with mu = 0, b = 0.
#pragma once
#include <hip/hip_runtime.h>

namespace spt {

__device__ __forceinline__ float ln_apply(float s, float mu, float rs, float g, float b) {
    return fmaf((s - mu) * rs, g, b);
}

}  // namespace spt
