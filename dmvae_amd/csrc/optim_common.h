// What the flat optimiser tail (optim.hip) and the multi-tensor one (optim_mt.hip) share: the per-element update, compiled from ONE definition so that both kernels
// give the same bits, and the final reduction of the grad-norm partial sums.
#pragma once
#include "common.h"

namespace dmvae_optim {

// ema' = ema * decay + p * (1 - decay): ONE rounding of the sum (fma), the product ema * decay rounded first.  decay = 0 gives p for every finite ema.
__device__ __forceinline__ float ema_one(const float ema, const float p, const float decay) {
#pragma clang fp contract(off)
  return __builtin_fmaf(1.f - decay, p, ema * decay);
}

// One element's update: torch.optim.AdamW's arithmetic (decoupled decay, bias corrections, IEEE sqrt and division) + the EMA; shared by every vector body, scalar
// path and tail of both files.  Every fused multiply-add is written out and contraction is off, so the roundings are these and no others wherever the function is
// inlined: left to the compiler, the 16-byte body of adamw_ema_kernel fused the EMA line as below while the scalar tail of the same kernel did not fuse it at all.
// The form is the one that body was compiled to:
//   m = fma(b1, m, (1 - b1) g'),  v = fma(b2, v, ((1 - b2) g') g'),  p = fma(1 - lr wd, p, -(step m / (sqrt(v) / bc2_sqrt + eps))),  1 - lr wd = fma(-lr, wd, 1).
__device__ __forceinline__ void adamw_one(float& pi, const float g, float& mi, float& vi, float* ema_i, const float coef, const float lr, const float b1, const float b2,
                                          const float eps, const float wd, const float step, const float bc2_sqrt, const float decay) {
#pragma clang fp contract(off)
  const float gi = g * coef;
  mi = __builtin_fmaf(b1, mi, (1.f - b1) * gi);
  vi = __builtin_fmaf(b2, vi, (1.f - b2) * gi * gi);
  const float denom = sqrtf(vi) / bc2_sqrt + eps;
  pi = __builtin_fmaf(__builtin_fmaf(-lr, wd, 1.f), pi, -(step * mi / denom));
  if (ema_i) *ema_i = ema_one(*ema_i, pi, decay);
}

// norm_out3 = { sqrt(prev_sq * use_prev + sum(part[0..nb))), min(1, max_norm / (norm + 1e-6)), that sum of squares }: the f64 sum of the f32 partials in a fixed
// order (optim.hip::norm_final_kernel, one wave).  Returns 0 or -5.
int norm_final_launch(const float* part, float* norm_out3, int nb, float max_norm, int use_prev, hipStream_t stream);

}  // namespace dmvae_optim
