// Kernels of the LightningDiT block VARIANTS (diffusion/lightningdit/lightningdit.py:183-252: the constructor's use_rmsnorm / wo_shift / use_swiglu / use_rope /
// use_qknorm switches away from their defaults).  Same conventions as csrc/dit.hip: residual stream f32, Linear operands / results bf16, a bf16 rounding exactly
// where the reference's autocast(bf16) graph rounds.
//
//   layernorm_modulate : a = bf16( (x - mean) * rsqrt(var + eps) * f32(bf16(1 + scale[b])) + shift[b] )      (nn.LayerNorm(C, elementwise_affine=False) + modulate)
//                        plain, fused with the preceding gated residual x += bf16(gate[b] * r) in place, and the out-of-place form of the training route
//   head_split         : qkv [B][N][3][H][D] -> q, k [B*H][N][Dp] (zero-padded), v [B*H][N][D] with norm in {none, rms} and rope in {off, on}
//   gelu_tanh          : y = bf16( 0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3))) )                          (nn.GELU(approximate="tanh") of timm's Mlp)
//
// and their backward kernels.  The LayerNorm entries share dit_rows.h with csrc/dit.hip: the sweep dispatch by_sweeps (the row kernels here are instantiated per
// SW = ceil(C / 256)), the width / modulation-offset / gate-offset rules, the blocks-per-sample rule and the backward's last stage modulate_bwd_final_kernel<false>.
// Tests: tests/test_gpu_dit_variants.py against tests/dit_variants_spec.py.
#include "common.h"
#include "dit_rows.h"
#include "dmvae_hip.h"

using namespace dmvae_dit_rows;
namespace dmvae_dit_var {

// Row statistics of a row held in registers, one wave per row.  mean first, then the variance as the sum of squared DEVIATIONS taken from the registers -- never
// E[x^2] - mean^2: the residual stream is f32 and its rows can carry a large common offset.  The deviations are re-centred once (d -= mean(d)): x - mean is exact
// for values within a factor of two of the mean, so what is left of the f32 error of the first mean goes with it.
template <int SW>
__device__ __forceinline__ void ln_center(f32x4 (&v)[SW], int lane, int C, float& m0_out, float& m1_out, float& rs, float eps) {
#pragma clang fp contract(off)
  // channels past the row's end hold zeros on entry and are put back to zero after every subtraction: selects, not branches -- the arithmetic is the same for
  // every lane and the row stays in registers
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < SW; k++) s += (v[k][0] + v[k][1]) + (v[k][2] + v[k][3]);
  const float m0 = wave_sum(s) / (float)C;
  float s1 = 0.f;
#pragma unroll
  for (int k = 0; k < SW; k++) {
    const bool in = k * 256 + lane * 4 < C;
#pragma unroll
    for (int e = 0; e < 4; e++) v[k][e] = in ? v[k][e] - m0 : 0.f;
    s1 += (v[k][0] + v[k][1]) + (v[k][2] + v[k][3]);
  }
  const float m1 = wave_sum(s1) / (float)C;
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < SW; k++) {
    const bool in = k * 256 + lane * 4 < C;
#pragma unroll
    for (int e = 0; e < 4; e++) v[k][e] = in ? v[k][e] - m1 : 0.f;
    ss += (v[k][0] * v[k][0] + v[k][1] * v[k][1]) + (v[k][2] * v[k][2] + v[k][3] * v[k][3]);
  }
  m0_out = m0; m1_out = m1;
  rs = rsqrtf(wave_sum(ss) / (float)C + eps);
}

// one wave per row, four rows per workgroup; mod: [B][stride] bf16, shift_off < 0: no shift.
// RES: first x[row] += bf16(gate[b] * r[row]), written to xo (== x: in place), then the norm of the updated row.  Both instantiations evaluate the expressions
// exactly as written (no contraction): the fused form gives the bits of the gated residual followed by the plain kernel.
template <bool RES, int SW>
__global__ __launch_bounds__(256) void layernorm_modulate_kernel(const float* x, const bf16* __restrict__ mod, bf16* __restrict__ y, int rows, int rows_per_sample,
                                                                 int C, int stride, int shift_off, int scale_off, float eps, const bf16* __restrict__ r,
                                                                 const bf16* __restrict__ gmod, int gstride, int gate_off, float* xo) {
#pragma clang fp contract(off)
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* xr = x + (size_t)row * C;
  const int b = row / rows_per_sample;
  // No value leaves a divergent branch: a lane past the row's end loads the row's last four channels (a valid address) and selects zeros; only stores are
  // predicated.  (With the loads under `if (c < C)` the compiler keeps a copy of the row per branch: 256 VGPRs.)
  f32x4 v[SW];
#pragma unroll
  for (int k = 0; k < SW; k++) {
    const int c = k * 256 + lane * 4;
    const bool in = c < C;
    const int cc = in ? c : C - 4;
    f32x4 t = *reinterpret_cast<const f32x4*>(xr + cc);
    if constexpr (RES) {
      const bf16x4 rv = *reinterpret_cast<const bf16x4*>(r + (size_t)row * C + cc);
      const bf16x4 g = *reinterpret_cast<const bf16x4*>(gmod + (size_t)b * gstride + gate_off + cc);
#pragma unroll
      for (int e = 0; e < 4; e++) t[e] += (float)(bf16)((float)g[e] * (float)rv[e]);
      if (in) *reinterpret_cast<f32x4*>(xo + (size_t)row * C + c) = t;
    }
#pragma unroll
    for (int e = 0; e < 4; e++) v[k][e] = in ? t[e] : 0.f;
  }
  float m0, m1, rs;
  ln_center(v, lane, C, m0, m1, rs, eps);
  const bf16* mrow = mod + (size_t)b * stride;
  bf16* yr = y + (size_t)row * C;
#pragma unroll
  for (int k = 0; k < SW; k++) {
    const int c = k * 256 + lane * 4;
    if (c < C) {
      const bf16x4 sc = *reinterpret_cast<const bf16x4*>(mrow + scale_off + c);
      bf16x4 sh = {(bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f};
      if (shift_off >= 0) sh = *reinterpret_cast<const bf16x4*>(mrow + shift_off + c);
      bf16x4 o;
#pragma unroll
      for (int e = 0; e < 4; e++)   // `1 + scale` is a bf16 tensor in the reference's autocast graph: rounded before it multiplies the f32 norm
        o[e] = (bf16)(v[k][e] * rs * (float)(bf16)(1.f + (float)sc[e]) + (float)sh[e]);
      *reinterpret_cast<bf16x4*>(yr + c) = o;
    }
  }
}

// ---- backward: a = bf16(xh * m + shift), xh = (x - mean) * rs, m = bf16(1 + scale[b]) ------------------------------------------------------------------
//   g = da * m;  dx += rs * (g - mean_c(g) - xh * mean_c(g * xh));  dscale[b] = sum_n da * xh;  dshift[b] = sum_n da.
// (A) one wave per row -> (the two parts of the mean, rs), (mean(g), mean(g * xh)); (B) one thread per four columns walking its block's rows, partial sums part[B][bps][2][C];
// (C) dit_rows.h::modulate_bwd_final_kernel<false>: dmod[b] = the sum of the sample's partials in block order: a fixed order, identical run to run.
template <int SW>
__global__ __launch_bounds__(256) void layernorm_rowstat_kernel(const bf16* __restrict__ da, const float* __restrict__ x, const bf16* __restrict__ mod,
                                                                float4* __restrict__ rowstat, int rows, int N, int C, int stride, int scale_off, float eps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  f32x4 v[SW];
#pragma unroll
  for (int k = 0; k < SW; k++) {      // as in the forward: clamped address and a select, no value out of a divergent branch
    const int c = k * 256 + lane * 4;
    const bool in = c < C;
    const f32x4 t = *reinterpret_cast<const f32x4*>(x + (size_t)row * C + (in ? c : C - 4));
#pragma unroll
    for (int e = 0; e < 4; e++) v[k][e] = in ? t[e] : 0.f;
  }
  float m0, m1, rs;
  ln_center(v, lane, C, m0, m1, rs, eps);
  const bf16* mrow = mod + (size_t)(row / N) * stride + scale_off;
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int k = 0; k < SW; k++) {
    const int c = k * 256 + lane * 4;
    const bool in = c < C;
    const int cc = in ? c : C - 4;
    const bf16x4 d = *reinterpret_cast<const bf16x4*>(da + (size_t)row * C + cc);
    const bf16x4 sc = *reinterpret_cast<const bf16x4*>(mrow + cc);
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const float g = in ? (float)d[e] * (float)(bf16)(1.f + (float)sc[e]) : 0.f;
      s1 += g;
      s2 += g * (v[k][e] * rs);
    }
  }
  s1 = wave_sum(s1) / (float)C;
  s2 = wave_sum(s2) / (float)C;
  if (lane == 0) { rowstat[2 * (size_t)row] = make_float4(m0, m1, rs, 0.f); rowstat[2 * (size_t)row + 1] = make_float4(s1, s2, 0.f, 0.f); }
}

__global__ __launch_bounds__(512) void layernorm_modulate_bwd_apply_kernel(const bf16* __restrict__ da, const float* __restrict__ x, const bf16* __restrict__ mod,
                                                                           const float4* __restrict__ rowstat, float* __restrict__ dx_io, float* __restrict__ part,
                                                                           int N, int C, int stride, int scale_off) {
  const int b = blockIdx.y, c = threadIdx.x * 4;
  if (c >= C) return;
  const bf16x4 sc = *reinterpret_cast<const bf16x4*>(mod + (size_t)b * stride + scale_off + c);
  f32x4 gm, a0 = {0, 0, 0, 0}, a1 = {0, 0, 0, 0};
#pragma unroll
  for (int e = 0; e < 4; e++) gm[e] = (float)(bf16)(1.f + (float)sc[e]);
  const int rpb = (N + gridDim.x - 1) / gridDim.x;
  const int n1 = min(N, (int)(blockIdx.x + 1) * rpb);
  for (int n = blockIdx.x * rpb; n < n1; n++) {
    const size_t row = (size_t)b * N + n;
    const float4 st = rowstat[2 * row], sm = rowstat[2 * row + 1];      // (m0, m1, rs, -), (mean g, mean g xh, -, -)
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + row * C + c);
    const bf16x4 d = *reinterpret_cast<const bf16x4*>(da + row * C + c);
    f32x4 o = *reinterpret_cast<const f32x4*>(dx_io + row * C + c);
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const float xh = ((v[e] - st.x) - st.y) * st.z, dv = (float)d[e];      // the two-step centring of ln_center: the same deviation, to the bit
      o[e] += st.z * (dv * gm[e] - sm.x - xh * sm.y);
      a0[e] += dv; a1[e] += dv * xh;
    }
    *reinterpret_cast<f32x4*>(dx_io + row * C + c) = o;
  }
  float* po = part + ((size_t)b * gridDim.x + blockIdx.x) * 2 * C;
  *reinterpret_cast<f32x4*>(po + c) = a0;
  *reinterpret_cast<f32x4*>(po + C + c) = a1;
}

// ---- head split -------------------------------------------------------------------------------------------------------------------------------------------
// one wave per (token, head); lane j < D/2 owns the feature pair (2j, 2j+1).  norm: per-head RMSNorm, the normalised value rounded to bf16 before the f32 weight
// multiplies (rms_norm.py:75-76); rope: t * cos + rotate_half(t) * sin in f32 on the (normalised or raw) bf16 value; one rounding to bf16 where SDPA takes its
// operands.  Neither: a relayout.  Padding columns [D, Dp) of q and k are written as zeros.
__global__ __launch_bounds__(256) void head_split_kernel(const bf16* __restrict__ qkv, const float* __restrict__ qw, const float* __restrict__ kw,
                                                         const float* __restrict__ cosb, const float* __restrict__ sinb, bf16* __restrict__ qo,
                                                         bf16* __restrict__ ko, bf16* __restrict__ vo, int tokens, int N, int H, int D, int Dp, int norm, int rope,
                                                         float eps) {
#pragma clang fp contract(off)
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= tokens * H) return;
  const int tok = row / H, h = row - tok * H;
  const int b = tok / N, n = tok - b * N;
  const bool live = 2 * lane < D, pad = 2 * lane >= D && 2 * lane < Dp;
  const bf16* base = qkv + (size_t)tok * 3 * H * D;
  float q0 = 0.f, q1 = 0.f, k0 = 0.f, k1 = 0.f;
  bf16x2 vv = {(bf16)0.f, (bf16)0.f};
  if (live) {
    const bf16x2 a = *reinterpret_cast<const bf16x2*>(base + (size_t)h * D + 2 * lane);
    const bf16x2 c = *reinterpret_cast<const bf16x2*>(base + (size_t)(H + h) * D + 2 * lane);
    vv = *reinterpret_cast<const bf16x2*>(base + (size_t)(2 * H + h) * D + 2 * lane);
    q0 = (float)a[0]; q1 = (float)a[1]; k0 = (float)c[0]; k1 = (float)c[1];
  }
  if (norm) {     // wave-uniform
    const float rq = rsqrtf(wave_sum(q0 * q0 + q1 * q1) / (float)D + eps);
    const float rk = rsqrtf(wave_sum(k0 * k0 + k1 * k1) / (float)D + eps);
    if (live) {
      const float wq0 = qw[2 * lane], wq1 = qw[2 * lane + 1], wk0 = kw[2 * lane], wk1 = kw[2 * lane + 1];
      q0 = (float)(bf16)(q0 * rq) * wq0; q1 = (float)(bf16)(q1 * rq) * wq1;
      k0 = (float)(bf16)(k0 * rk) * wk0; k1 = (float)(bf16)(k1 * rk) * wk1;
    }
  }
  if (rope && live) {
    const float c0 = cosb[(size_t)n * D + 2 * lane], c1 = cosb[(size_t)n * D + 2 * lane + 1];
    const float s0 = sinb[(size_t)n * D + 2 * lane], s1 = sinb[(size_t)n * D + 2 * lane + 1];
    const float a0 = q0 * c0 - q1 * s0, a1 = q1 * c1 + q0 * s1;
    const float e0 = k0 * c0 - k1 * s0, e1 = k1 * c1 + k0 * s1;
    q0 = a0; q1 = a1; k0 = e0; k1 = e1;
  }
  const size_t o = ((size_t)(b * H + h) * N + n);
  if (live) {
    const bf16x2 qq = {(bf16)q0, (bf16)q1}, kk = {(bf16)k0, (bf16)k1};
    *reinterpret_cast<bf16x2*>(qo + o * Dp + 2 * lane) = qq;
    *reinterpret_cast<bf16x2*>(ko + o * Dp + 2 * lane) = kk;
    *reinterpret_cast<bf16x2*>(vo + o * D + 2 * lane) = vv;
  } else if (pad) {
    const bf16x2 z = {(bf16)0.f, (bf16)0.f};
    *reinterpret_cast<bf16x2*>(qo + o * Dp + 2 * lane) = z;
    *reinterpret_cast<bf16x2*>(ko + o * Dp + 2 * lane) = z;
  }
}

// Backward: dq, dk [B*H][N][Dp], dv [B*H][N][D] -> dqkv [B][N][3][H][D] bf16 through the transposed rotation and the RMSNorm; part [gridDim.x][2][D]: the block's
// partial sums of the two norm weights' gradients (part == NULL: none wanted -- frozen weights or no norm).
__global__ __launch_bounds__(256) void head_split_bwd_kernel(const bf16* __restrict__ dq, const bf16* __restrict__ dk, const bf16* __restrict__ dv,
                                                             const bf16* __restrict__ qkv, const float* __restrict__ qw, const float* __restrict__ kw,
                                                             const float* __restrict__ cosb, const float* __restrict__ sinb, bf16* __restrict__ dqkv,
                                                             float* __restrict__ part, int tokens, int N, int H, int D, int Dp, int norm, int rope, float eps) {
  __shared__ float red[4][4][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool live = 2 * lane < D;
  float gq0 = 0.f, gq1 = 0.f, gk0 = 0.f, gk1 = 0.f;
  float wq0 = 0.f, wq1 = 0.f, wk0 = 0.f, wk1 = 0.f;
  if (norm && live) { wq0 = qw[2 * lane]; wq1 = qw[2 * lane + 1]; wk0 = kw[2 * lane]; wk1 = kw[2 * lane + 1]; }
  for (int row = blockIdx.x * 4 + wave; row < tokens * H; row += gridDim.x * 4) {
    const int tok = row / H, h = row - tok * H;
    const int b = tok / N, n = tok - b * N;
    const size_t o = ((size_t)(b * H + h) * N + n);
    const bf16* base = qkv + (size_t)tok * 3 * H * D;
    bf16* dbase = dqkv + (size_t)tok * 3 * H * D;
    float e0 = 0.f, e1 = 0.f, f0 = 0.f, f1 = 0.f;      // d(q), d(k) before the rotation
    bf16x2 dvv = {(bf16)0.f, (bf16)0.f};
    if (live) {
      const bf16x2 ga = *reinterpret_cast<const bf16x2*>(dq + o * Dp + 2 * lane);
      const bf16x2 gc = *reinterpret_cast<const bf16x2*>(dk + o * Dp + 2 * lane);
      dvv = *reinterpret_cast<const bf16x2*>(dv + o * D + 2 * lane);
      e0 = (float)ga[0]; e1 = (float)ga[1]; f0 = (float)gc[0]; f1 = (float)gc[1];
      if (rope) {   // transpose of the pair rotation: out0 = a0*c0 - a1*s0, out1 = a1*c1 + a0*s1
        const float c0 = cosb[(size_t)n * D + 2 * lane], c1 = cosb[(size_t)n * D + 2 * lane + 1];
        const float s0 = sinb[(size_t)n * D + 2 * lane], s1 = sinb[(size_t)n * D + 2 * lane + 1];
        const float t0 = e0 * c0 + e1 * s1, t1 = e1 * c1 - e0 * s0;
        const float u0 = f0 * c0 + f1 * s1, u1 = f1 * c1 - f0 * s0;
        e0 = t0; e1 = t1; f0 = u0; f1 = u1;
      }
    }
    if (norm) {     // wave-uniform
      float q0 = 0.f, q1 = 0.f, k0 = 0.f, k1 = 0.f;
      if (live) {
        const bf16x2 a = *reinterpret_cast<const bf16x2*>(base + (size_t)h * D + 2 * lane);
        const bf16x2 c = *reinterpret_cast<const bf16x2*>(base + (size_t)(H + h) * D + 2 * lane);
        q0 = (float)a[0]; q1 = (float)a[1]; k0 = (float)c[0]; k1 = (float)c[1];
      }
      const float rq = rsqrtf(wave_sum(q0 * q0 + q1 * q1) / (float)D + eps);
      const float rk = rsqrtf(wave_sum(k0 * k0 + k1 * k1) / (float)D + eps);
      const float nq0 = q0 * rq, nq1 = q1 * rq, nk0 = k0 * rk, nk1 = k1 * rk;
      if (part) { gq0 += e0 * (float)(bf16)nq0; gq1 += e1 * (float)(bf16)nq1; gk0 += f0 * (float)(bf16)nk0; gk1 += f1 * (float)(bf16)nk1; }
      e0 *= wq0; e1 *= wq1; f0 *= wk0; f1 *= wk1;         // d(normalised)
      const float mq = wave_sum(e0 * nq0 + e1 * nq1) / (float)D, mk = wave_sum(f0 * nk0 + f1 * nk1) / (float)D;
      e0 = rq * (e0 - nq0 * mq); e1 = rq * (e1 - nq1 * mq);
      f0 = rk * (f0 - nk0 * mk); f1 = rk * (f1 - nk1 * mk);
    }
    if (live) {
      const bf16x2 oq = {(bf16)e0, (bf16)e1}, ok = {(bf16)f0, (bf16)f1};
      *reinterpret_cast<bf16x2*>(dbase + (size_t)h * D + 2 * lane) = oq;
      *reinterpret_cast<bf16x2*>(dbase + (size_t)(H + h) * D + 2 * lane) = ok;
      *reinterpret_cast<bf16x2*>(dbase + (size_t)(2 * H + h) * D + 2 * lane) = dvv;
    }
  }
  if (!part) return;      // kernel-uniform
  red[wave][0][lane] = gq0; red[wave][1][lane] = gq1; red[wave][2][lane] = gk0; red[wave][3][lane] = gk1;
  __syncthreads();
  if (threadIdx.x < 2 * D) {            // part[blk][0][d] = dq_weight, part[blk][1][d] = dk_weight
    const int which = threadIdx.x / D, d = threadIdx.x - which * D;
    const int slot = which * 2 + (d & 1), ln = d >> 1;
    part[((size_t)blockIdx.x * 2 + which) * D + d] = (red[0][slot][ln] + red[1][slot][ln]) + (red[2][slot][ln] + red[3][slot][ln]);
  }
}

// part [nblk][2][D] -> o0[d], o1[d]: one thread per output, the blocks in order (nblk <= 2048 rows of 2 D floats)
__global__ void head_split_wsum_kernel(const float* __restrict__ part, float* __restrict__ o0, float* __restrict__ o1, int nblk, int D, int accumulate) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * D) return;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int b = 0;
  for (; b + 3 < nblk; b += 4) {
    a0 += part[(size_t)b * 2 * D + i]; a1 += part[(size_t)(b + 1) * 2 * D + i]; a2 += part[(size_t)(b + 2) * 2 * D + i]; a3 += part[(size_t)(b + 3) * 2 * D + i];
  }
  for (; b < nblk; b++) a0 += part[(size_t)b * 2 * D + i];
  const float t = (a0 + a1) + (a2 + a3);
  const int which = i / D, d = i - which * D;
  float* o = which ? o1 : o0;
  o[d] = (accumulate ? o[d] : 0.f) + t;
}

// ---- tanh-GELU --------------------------------------------------------------------------------------------------------------------------------------------
// 0.5 x (1 + tanh u) = x * sigmoid(2u), u = sqrt(2/pi) (x + 0.044715 x^3): the same function without the 1 + tanh cancellation of the negative tail.  With
// e = exp(-2|u|) in (0, 1] and r = 1 / (1 + e): sigmoid(2|u|) = r, sigmoid(-2|u|) = e r, and their product s (1 - s) = e r^2 -- nothing overflows, nothing cancels.
// Non-finite inputs as torch's formula: NaN -> NaN, +inf -> +inf, -inf -> NaN (inf * 0); x^3 overflowing takes the same limits.
struct gelu_parts { float s, ss; };   // s = sigmoid(2u), ss = s (1 - s)
__device__ __forceinline__ gelu_parts gelu_tanh_parts(float x) {
  const float u = 0.7978845608028654f * (x + 0.044715f * (x * x * x));
  const float e = __expf(-2.0f * fabsf(u));
  const float r = __builtin_amdgcn_rcpf(1.0f + e);
  gelu_parts p;
  p.s = u >= 0.f ? r : e * r;      // NaN: e and r are NaN, so is either branch
  p.ss = e * r * r;
  return p;
}
__device__ __forceinline__ float gelu_tanh_f(float x) { return x * gelu_tanh_parts(x).s; }
// d/dx [x s(2u)] = s + x * 2 s (1 - s) * du/dx,  du/dx = sqrt(2/pi) (1 + 3 * 0.044715 x^2)
__device__ __forceinline__ float gelu_tanh_grad_f(float x) {
  const gelu_parts p = gelu_tanh_parts(x);
  return p.s + x * (2.0f * p.ss) * (0.7978845608028654f * (1.0f + 0.134145f * (x * x)));
}

// nvec 16-byte vectors, then the n - 8 nvec elements of the tail one by one
__global__ void gelu_tanh_fwd_kernel(const bf16* __restrict__ x, bf16* __restrict__ y, size_t n, size_t nvec) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (size_t)gridDim.x * blockDim.x) {
    const bf16x8 a = reinterpret_cast<const bf16x8*>(x)[i];
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; e++) o[e] = (bf16)gelu_tanh_f((float)a[e]);
    reinterpret_cast<bf16x8*>(y)[i] = o;
  }
  for (size_t i = nvec * 8 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) y[i] = (bf16)gelu_tanh_f((float)x[i]);
}

__global__ void gelu_tanh_bwd_kernel(const bf16* __restrict__ dy, const bf16* __restrict__ x, bf16* __restrict__ dx, size_t n, size_t nvec) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (size_t)gridDim.x * blockDim.x) {
    const bf16x8 a = reinterpret_cast<const bf16x8*>(x)[i], d = reinterpret_cast<const bf16x8*>(dy)[i];
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; e++) o[e] = (bf16)((float)d[e] * gelu_tanh_grad_f((float)a[e]));
    reinterpret_cast<bf16x8*>(dx)[i] = o;
  }
  for (size_t i = nvec * 8 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    dx[i] = (bf16)((float)dy[i] * gelu_tanh_grad_f((float)x[i]));
}

}  // namespace dmvae_dit_var
using namespace dmvae_dit_var;

extern "C" int dmvae_layernorm_modulate_bf16(const void* x, const void* mod, void* y, int rows, int rows_per_sample, int c, int mod_stride, int shift_off,
                                             int scale_off, float eps, hipStream_t stream) {
  DMVAE_CHECK_ARG(x && mod && y && rows > 0 && rows_per_sample > 0, "layernorm_modulate_bf16: bad argument");
  DMVAE_CHECK_ARG(row_width_ok(c), "layernorm_modulate_bf16: width must be a multiple of 4 up to 2048 (got %d)", c);
  DMVAE_CHECK_ARG(mod_offsets_ok(c, mod_stride, shift_off, scale_off), "layernorm_modulate_bf16: modulation offsets must be multiples of 4 inside the row");
  return by_sweeps(c, [&](auto sw) {
    hipLaunchKernelGGL((layernorm_modulate_kernel<false, decltype(sw)::value>), dim3((rows + 3) / 4), dim3(256), 0, stream, (const float*)x, (const bf16*)mod,
                       (bf16*)y, rows, rows_per_sample, c, mod_stride, shift_off, scale_off, eps, (const bf16*)nullptr, (const bf16*)nullptr, 0, 0, (float*)nullptr);
    DMVAE_CHECK_LAUNCH();
    return 0;
  });
}

// x_out == x_in: in place (the inference route); x_out another buffer: the training route keeps the stream before the update for its backward pass
extern "C" int dmvae_gated_residual_layernorm_modulate(const void* x_in, void* x_out, const void* r, const void* gate_mod, int gate_stride, int gate_off,
                                                       const void* mod, void* y, int rows, int rows_per_sample, int c, int mod_stride, int shift_off,
                                                       int scale_off, float eps, hipStream_t stream) {
  DMVAE_CHECK_ARG(x_in && x_out && r && gate_mod && mod && y && rows > 0 && rows_per_sample > 0, "gated_residual_layernorm_modulate: bad argument");
  DMVAE_CHECK_ARG(row_width_ok(c), "gated_residual_layernorm_modulate: width must be a multiple of 4 up to 2048 (got %d)", c);
  DMVAE_CHECK_ARG(mod_offsets_ok(c, mod_stride, shift_off, scale_off) && gate_offset_ok(c, gate_stride, gate_off),
                  "gated_residual_layernorm_modulate: modulation offsets must be multiples of 4 inside the row");
  return by_sweeps(c, [&](auto sw) {
    hipLaunchKernelGGL((layernorm_modulate_kernel<true, decltype(sw)::value>), dim3((rows + 3) / 4), dim3(256), 0, stream, (const float*)x_in, (const bf16*)mod,
                       (bf16*)y, rows, rows_per_sample, c, mod_stride, shift_off, scale_off, eps, (const bf16*)r, (const bf16*)gate_mod, gate_stride, gate_off,
                       (float*)x_out);
    DMVAE_CHECK_LAUNCH();
    return 0;
  });
}

extern "C" size_t dmvae_layernorm_modulate_bwd_workspace(int batch, int seq, int c) {
  if (batch <= 0 || seq <= 0 || c <= 0) return 0;
  return (size_t)batch * MAX_BPS * 2 * (size_t)c * sizeof(float) + (size_t)batch * (size_t)seq * 2 * sizeof(float4);
}

extern "C" int dmvae_layernorm_modulate_bwd(const void* da, const void* x, const void* mod, void* dx_io, void* dmod, void* workspace, size_t workspace_bytes,
                                            int batch, int seq, int c, int mod_stride, int shift_off, int scale_off, float eps, hipStream_t stream) {
  DMVAE_CHECK_ARG(da && x && mod && dx_io && dmod && workspace && batch > 0 && seq > 0, "layernorm_modulate_bwd: bad argument");
  DMVAE_CHECK_ARG(row_width_ok(c), "layernorm_modulate_bwd: width must be a multiple of 4 up to 2048 (got %d)", c);
  DMVAE_CHECK_ARG(mod_offsets_ok(c, mod_stride, shift_off, scale_off), "layernorm_modulate_bwd: modulation offsets must be multiples of 4 inside the row");
  DMVAE_CHECK_ARG(workspace_bytes >= dmvae_layernorm_modulate_bwd_workspace(batch, seq, c), "layernorm_modulate_bwd: workspace too small");
  DMVAE_CHECK_ARG((size_t)batch * (size_t)seq <= 0x7fffffffu - 4, "layernorm_modulate_bwd: too many rows");
  const int bps = blocks_per_sample(batch);
  float4* rowstat = reinterpret_cast<float4*>((float*)workspace + (size_t)batch * MAX_BPS * 2 * (size_t)c);   // 16-byte aligned: the offset is a multiple of 4 floats
  const int rows = batch * seq;
  const int rc = by_sweeps(c, [&](auto sw) {
    hipLaunchKernelGGL(layernorm_rowstat_kernel<decltype(sw)::value>, dim3((rows + 3) / 4), dim3(256), 0, stream, (const bf16*)da, (const float*)x,
                       (const bf16*)mod, rowstat, rows, seq, c, mod_stride, scale_off, eps);
    DMVAE_CHECK_LAUNCH();
    return 0;
  });
  if (rc) return rc;
  const int bt = ((c / 4) + 63) / 64 * 64;
  hipLaunchKernelGGL(layernorm_modulate_bwd_apply_kernel, dim3(bps, batch), dim3(bt), 0, stream, (const bf16*)da, (const float*)x, (const bf16*)mod, rowstat,
                     (float*)dx_io, (float*)workspace, seq, c, mod_stride, scale_off);
  DMVAE_CHECK_LAUNCH();
  hipLaunchKernelGGL(modulate_bwd_final_kernel<false>, dim3((c + 255) / 256, batch), dim3(256), 0, stream, (const float*)workspace, (float*)dmod, (float*)nullptr,
                     bps, c, mod_stride, shift_off, scale_off);
  DMVAE_CHECK_LAUNCH();
  return 0;
}

static bool hs_dims_ok(int head_dim, int head_dim_padded) {
  return head_dim % 2 == 0 && head_dim >= 2 && head_dim_padded >= head_dim && head_dim_padded % 2 == 0 && head_dim_padded <= 128;
}

extern "C" int dmvae_head_split_bf16(const void* qkv, const void* q_weight, const void* k_weight, const void* cos_table, const void* sin_table, void* q_out,
                                     void* k_out, void* v_out, int batch, int seq, int heads, int head_dim, int head_dim_padded, int norm_kind, int rope,
                                     float eps, hipStream_t stream) {
  DMVAE_CHECK_ARG(qkv && q_out && k_out && v_out && batch > 0 && seq > 0 && heads > 0, "head_split_bf16: bad argument");
  DMVAE_CHECK_ARG((norm_kind == 0 || norm_kind == 1) && (rope == 0 || rope == 1), "head_split_bf16: norm kind is 0 (none) or 1 (rms), rope 0 or 1");
  DMVAE_CHECK_ARG((!norm_kind || (q_weight && k_weight)) && (!rope || (cos_table && sin_table)), "head_split_bf16: null norm weight or rotary table");
  DMVAE_CHECK_ARG(hs_dims_ok(head_dim, head_dim_padded), "head_split_bf16: head dim must be even, padded head dim <= 128 (got %d, %d)", head_dim, head_dim_padded);
  DMVAE_CHECK_ARG((size_t)batch * seq * heads <= 0x7fffffffu - 4, "head_split_bf16: too many rows");
  const int tokens = batch * seq;
  hipLaunchKernelGGL(head_split_kernel, dim3((tokens * heads + 3) / 4), dim3(256), 0, stream, (const bf16*)qkv, (const float*)q_weight, (const float*)k_weight,
                     (const float*)cos_table, (const float*)sin_table, (bf16*)q_out, (bf16*)k_out, (bf16*)v_out, tokens, seq, heads, head_dim, head_dim_padded,
                     norm_kind, rope, eps);
  DMVAE_CHECK_LAUNCH();
  return 0;
}

// blocks of the backward's first stage = rows of its partial-sum array [nblk][2][head_dim] f32 (the workspace when the norm weights' gradients are wanted)
extern "C" int dmvae_head_split_bwd_nblk(int batch, int seq, int heads) {
  if (batch <= 0 || seq <= 0 || heads <= 0) return 0;
  const size_t rows = (size_t)batch * seq * heads;
  const size_t nblk = (rows + 3) / 4;
  return (int)(nblk > 2048 ? 2048 : nblk);
}

// dq_weight / dk_weight NULL (both): dqkv only -- no norm, or frozen norm weights; the workspace is then not used
extern "C" int dmvae_head_split_bwd(const void* dq, const void* dk, const void* dv, const void* qkv, const void* q_weight, const void* k_weight,
                                    const void* cos_table, const void* sin_table, void* dqkv, void* dq_weight, void* dk_weight, void* workspace,
                                    size_t workspace_bytes, int batch, int seq, int heads, int head_dim, int head_dim_padded, int norm_kind, int rope, float eps,
                                    int accumulate, hipStream_t stream) {
  DMVAE_CHECK_ARG(dq && dk && dv && dqkv && batch > 0 && seq > 0 && heads > 0, "head_split_bwd: bad argument");
  DMVAE_CHECK_ARG((norm_kind == 0 || norm_kind == 1) && (rope == 0 || rope == 1), "head_split_bwd: norm kind is 0 (none) or 1 (rms), rope 0 or 1");
  DMVAE_CHECK_ARG((!norm_kind || (qkv && q_weight && k_weight)) && (!rope || (cos_table && sin_table)), "head_split_bwd: null qkv, norm weight or rotary table");
  DMVAE_CHECK_ARG(hs_dims_ok(head_dim, head_dim_padded), "head_split_bwd: head dim must be even, padded head dim <= 128 (got %d, %d)", head_dim, head_dim_padded);
  DMVAE_CHECK_ARG((size_t)batch * seq * heads <= 0x7fffffffu - 4, "head_split_bwd: too many rows");
  DMVAE_CHECK_ARG((dq_weight == nullptr) == (dk_weight == nullptr) && (!dq_weight || norm_kind), "head_split_bwd: the two weight gradients come together, with a norm");
  const int tokens = batch * seq;
  const int nblk = dmvae_head_split_bwd_nblk(batch, seq, heads);
  const bool wgrad = dq_weight != nullptr;
  DMVAE_CHECK_ARG(!wgrad || (workspace && workspace_bytes >= (size_t)nblk * 2 * head_dim * sizeof(float)), "head_split_bwd: workspace too small");
  hipLaunchKernelGGL(head_split_bwd_kernel, dim3(nblk), dim3(256), 0, stream, (const bf16*)dq, (const bf16*)dk, (const bf16*)dv, (const bf16*)qkv,
                     (const float*)q_weight, (const float*)k_weight, (const float*)cos_table, (const float*)sin_table, (bf16*)dqkv,
                     wgrad ? (float*)workspace : (float*)nullptr, tokens, seq, heads, head_dim, head_dim_padded, norm_kind, rope, eps);
  DMVAE_CHECK_LAUNCH();
  if (wgrad) {
    hipLaunchKernelGGL(head_split_wsum_kernel, dim3((2 * head_dim + 63) / 64), dim3(64), 0, stream, (const float*)workspace, (float*)dq_weight, (float*)dk_weight,
                       nblk, head_dim, accumulate);
    DMVAE_CHECK_LAUNCH();
  }
  return 0;
}

static size_t gelu_nvec(const void* a, const void* b, const void* c, size_t n) {
  const uintptr_t bits = (uintptr_t)a | (uintptr_t)b | (uintptr_t)c;
  return (bits & 15) ? 0 : n / 8;      // a view that does not start on a 16-byte boundary: element by element
}

extern "C" int dmvae_gelu_tanh_fwd(const void* x, void* y, size_t n, hipStream_t stream) {
  DMVAE_CHECK_ARG(x && y, "gelu_tanh_fwd: null pointer");
  if (n == 0) return 0;
  const size_t nvec = gelu_nvec(x, y, nullptr, n);
  hipLaunchKernelGGL(gelu_tanh_fwd_kernel, dim3(grid_for(nvec ? nvec : n, 256, 4096)), dim3(256), 0, stream, (const bf16*)x, (bf16*)y, n, nvec);
  DMVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int dmvae_gelu_tanh_bwd(const void* dy, const void* x, void* dx, size_t n, hipStream_t stream) {
  DMVAE_CHECK_ARG(dy && x && dx, "gelu_tanh_bwd: null pointer");
  if (n == 0) return 0;
  const size_t nvec = gelu_nvec(dy, x, dx, n);
  hipLaunchKernelGGL(gelu_tanh_bwd_kernel, dim3(grid_for(nvec ? nvec : n, 256, 4096)), dim3(256), 0, stream, (const bf16*)dy, (const bf16*)x, (bf16*)dx, n, nvec);
  DMVAE_CHECK_LAUNCH();
  return 0;
}
