// What the LightningDiT row kernels of csrc/dit.hip, dit_variants.hip and dit_stack.hip have in common, stated once: the sweep dispatch, the argument rules of
// the adaLN entries, the blocks-per-sample rule, the RMSNorm row-statistics kernel, the per-element backward expressions that the per-block kernels and the
// fused boundary kernel both evaluate, and the second reduction stage of the modulate backward.
#pragma once
#include "common.h"
#include <type_traits>

namespace dmvae_dit_rows {

constexpr int MAX_SWEEPS = 8;   // C <= 2048: a row of 8 x 256 channels, four per lane; the row kernels are instantiated per sweep count SW = ceil(C / 256)
constexpr int MAX_BPS = 32;     // blocks per sample of the two-stage backward kernels: rows of their partial sums (4 waves x 2 rows each at N = 256 tokens)

// f(std::integral_constant<int, SW>{}) with SW = ceil(c / 256), one instantiation per sweep count 1 .. 8; returns what f returns (the C ABI's int).
// c is validated first (row_width_ok): any other count is an error, never a neighbouring instantiation.
template <class F>
static inline int by_sweeps(int c, F&& f) {
  switch ((c + 255) / 256) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
    case 8: return f(std::integral_constant<int, 8>{});
  }
  dmvae_set_error("by_sweeps: width %d outside 4 .. %d", c, MAX_SWEEPS * 256);
  return -22;
}

// Argument rules of the seven adaLN row entries (16- or 8-byte accesses per lane: everything a multiple of 4 channels, every chunk inside its modulation row).
static inline bool row_width_ok(int c) { return c % 4 == 0 && c >= 4 && c <= MAX_SWEEPS * 256; }
// shift_off < 0: no shift chunk
static inline bool mod_offsets_ok(int c, int mod_stride, int shift_off, int scale_off) {
  return scale_off >= 0 && scale_off % 4 == 0 && (shift_off < 0 || (shift_off % 4 == 0 && shift_off + c <= mod_stride)) && mod_stride % 4 == 0 &&
         scale_off + c <= mod_stride;
}
static inline bool gate_offset_ok(int c, int gate_stride, int gate_off) {
  return gate_off >= 0 && gate_off % 4 == 0 && gate_stride % 4 == 0 && gate_off + c <= gate_stride;
}

// Blocks per sample of the backward kernels that walk a sample's rows: enough blocks to fill the chip (~1024), few enough that the per-block partial sums stay
// small next to the rows a block walks -- 32 at batch 16 (2 rows per wave at 256 tokens), 16 at batch 64.
static inline int blocks_per_sample(int batch) {
  const int bps = 1024 / batch;
  return bps > MAX_BPS ? MAX_BPS : (bps < 4 ? 4 : bps);
}

// RMSNorm + modulate backward, stage (A): one wave per row -> rstd and m2 = mean_c(g * xhat), g = da * w * bf16(1 + scale).  Internal linkage: each translation
// unit that launches it (dit.hip, dit_stack.hip) carries its own copy of this one definition.
static __global__ __launch_bounds__(256) void rmsnorm_rowstat_kernel(const bf16* __restrict__ da, const float* __restrict__ x, const float* __restrict__ w,
                                                                     const bf16* __restrict__ mod, float2* __restrict__ rowstat, int rows, int N, int C,
                                                                     int stride, int scale_off, float eps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const bf16* mrow = mod + (size_t)(row / N) * stride + scale_off;
  float ss = 0.f, s2 = 0.f;
  for (int c = lane * 4; c < C; c += 256) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + (size_t)row * C + c);
    const bf16x4 d = *reinterpret_cast<const bf16x4*>(da + (size_t)row * C + c);
    const f32x4 gw = *reinterpret_cast<const f32x4*>(w + c);
    const bf16x4 sc = *reinterpret_cast<const bf16x4*>(mrow + c);
#pragma unroll
    for (int e = 0; e < 4; e++) {
      ss += v[e] * v[e];
      s2 += (float)d[e] * gw[e] * (float)(bf16)(1.f + (float)sc[e]) * v[e];
    }
  }
  const float rs = rsqrtf(wave_sum(ss) / (float)C + eps);
  const float m2 = wave_sum(s2) * rs / (float)C;
  if (lane == 0) rowstat[row] = make_float2(rs, m2);
}

// Stage (B), one element: a = bf16(n * w * m + shift), n = x * rs, m = bf16(1 + scale[b]), st = (rs, m2) of the row ->
//   dx: the term added to the stream gradient, rs * (g - n * m2), g = da * w * m;  dshift, dscale, dw: the element's terms of the three column sums.
struct rms_bwd_terms { float dx, dshift, dscale, dw; };
__device__ __forceinline__ rms_bwd_terms rmsnorm_modulate_bwd_terms(float xv, float dv, float gw, float gm, float2 st) {
  const float nh = xv * st.x;
  const float g = dv * gw * gm;
  return {st.x * (g - nh * st.y), dv, dv * nh * gw, dv * gm * nh};
}

// Gated residual x_out = x + bf16(gate[b] * y), one element: dy = bf16(gate * dx_out); the element's term of dgate[b][c] = sum_n dx_out * y.
__device__ __forceinline__ bf16 gated_residual_bwd_dy(float gate, float dx) { return (bf16)(gate * dx); }
__device__ __forceinline__ float gated_residual_bwd_dgate(float dx, float y) { return dx * y; }

// Stage (C), grid (C/256, B): dmod[b][shift_off + c] = sum_blk part[b][blk][0][c] (skipped when shift_off < 0), dmod[b][scale_off + c] = ... [1] ..., the blocks
// in order.  WPART (RMSNorm: part has a third plane, the norm weight's): wpart[b][c] = sum_blk part[b][blk][2][c].
template <bool WPART>
__global__ void modulate_bwd_final_kernel(const float* __restrict__ part, float* __restrict__ dmod, float* __restrict__ wpart, int bps, int C, int stride,
                                          int shift_off, int scale_off) {
  constexpr int PLANES = WPART ? 3 : 2;
  const int c = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (c >= C) return;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  for (int k = 0; k < bps; k++) {
    const float* q = part + ((size_t)b * bps + k) * PLANES * C;
    s0 += q[c]; s1 += q[C + c];
    if constexpr (WPART) s2 += q[2 * C + c];
  }
  if (shift_off >= 0) dmod[(size_t)b * stride + shift_off + c] = s0;
  dmod[(size_t)b * stride + scale_off + c] = s1;
  if constexpr (WPART) wpart[(size_t)b * C + c] = s2;
}

}  // namespace dmvae_dit_rows
