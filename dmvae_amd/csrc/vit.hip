// Elementwise kernels of the frozen ViT encoder forward (models/vae.py:52-53 -> timm VisionTransformer blocks; block algebra as
// in the reference's vendored models/dino_layers/block.py:89-115): the f32 residual stream stays in HBM, everything that
// feeds a GEMM is bf16.  Both are HBM-bound row kernels (16-B accesses, one wave per row, f32 statistics).
//   layernorm_f32_bf16 : y = bf16( (x - mean) * rstd * gamma + beta )      replaces nn.LayerNorm (f32 under autocast) + the bf16 cast
//   scale_residual_f32 : x += gamma * float(y)                              replaces LayerScale (dino_layers/layer_scale.py:15-26) + the
//                                                                          residual add (f32 under autocast type promotion)
#include "common.h"
#include "dmvae_hip.h"

namespace dmvae_vit {

// one wave per row; C = SWEEPS * 256 (4 floats per lane per sweep) + TAIL * 128 (a last half sweep of 2 floats per lane: ViT-S, C = 384 = 256 + 128), C <= 4096.
// TAIL = false compiles to exactly the sweeps-only kernel: the widths that are multiples of 256 keep their bits.
// RES: the LayerScale + residual add that precedes every LayerNorm but the first (x += ls * r, the previous branch's output r in bf16) in the same pass --
// the f32 residual stream is read and written once instead of read-written by one kernel and read again by the next (bit-identical to the two kernels).
template <int SWEEPS, bool RES = false, bool TAIL = false>
__global__ __launch_bounds__(256) void layernorm_kernel(float* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, bf16* __restrict__ y, int rows, float eps,
                                                        const bf16* __restrict__ r = nullptr, const float* __restrict__ ls = nullptr) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  constexpr int C = SWEEPS * 256 + (TAIL ? 128 : 0), T0 = SWEEPS * 256;   // T0: first column of the half sweep
  float* xr = x + (size_t)row * C;
  f32x4 v[SWEEPS];
  f32x2 vt = {0.f, 0.f};
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < SWEEPS; k++) {
    v[k] = *reinterpret_cast<const f32x4*>(xr + k * 256 + lane * 4);
    if constexpr (RES) {
      const bf16x4 rv = *reinterpret_cast<const bf16x4*>(r + (size_t)row * C + k * 256 + lane * 4);
      const f32x4 g = *reinterpret_cast<const f32x4*>(ls + k * 256 + lane * 4);
#pragma unroll
      for (int e = 0; e < 4; e++) v[k][e] = fmaf(g[e], (float)rv[e], v[k][e]);
      *reinterpret_cast<f32x4*>(xr + k * 256 + lane * 4) = v[k];
    }
    s += (v[k][0] + v[k][1]) + (v[k][2] + v[k][3]);
  }
  if constexpr (TAIL) {
    vt = *reinterpret_cast<const f32x2*>(xr + T0 + lane * 2);
    if constexpr (RES) {
      const bf16x2 rv = *reinterpret_cast<const bf16x2*>(r + (size_t)row * C + T0 + lane * 2);
      const f32x2 g = *reinterpret_cast<const f32x2*>(ls + T0 + lane * 2);
#pragma unroll
      for (int e = 0; e < 2; e++) vt[e] = fmaf(g[e], (float)rv[e], vt[e]);
      *reinterpret_cast<f32x2*>(xr + T0 + lane * 2) = vt;
    }
    s += vt[0] + vt[1];
  }
  const float mean = wave_sum(s) * (1.f / C);
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < SWEEPS; k++)
#pragma unroll
    for (int e = 0; e < 4; e++) { const float d = v[k][e] - mean; ss += d * d; }
  if constexpr (TAIL) {
#pragma unroll
    for (int e = 0; e < 2; e++) { const float d = vt[e] - mean; ss += d * d; }
  }
  const float rstd = rsqrtf(wave_sum(ss) * (1.f / C) + eps);
  bf16* yr = y + (size_t)row * C;
#pragma unroll
  for (int k = 0; k < SWEEPS; k++) {
    const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + k * 256 + lane * 4);
    const f32x4 b = *reinterpret_cast<const f32x4*>(beta + k * 256 + lane * 4);
    bf16x4 o;
#pragma unroll
    for (int e = 0; e < 4; e++) o[e] = (bf16)((v[k][e] - mean) * rstd * g[e] + b[e]);
    *reinterpret_cast<bf16x4*>(yr + k * 256 + lane * 4) = o;
  }
  if constexpr (TAIL) {
    const f32x2 g = *reinterpret_cast<const f32x2*>(gamma + T0 + lane * 2);
    const f32x2 b = *reinterpret_cast<const f32x2*>(beta + T0 + lane * 2);
    bf16x2 o;
#pragma unroll
    for (int e = 0; e < 2; e++) o[e] = (bf16)((vt[e] - mean) * rstd * g[e] + b[e]);
    *reinterpret_cast<bf16x2*>(yr + T0 + lane * 2) = o;
  }
}

__global__ __launch_bounds__(256) void scale_residual_kernel(float* __restrict__ x, const bf16* __restrict__ y, const float* __restrict__ gamma,
                                                             size_t n8, int c8) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % c8) * 8;
    const bf16x8 v = reinterpret_cast<const bf16x8*>(y)[i];
    f32x4 a = reinterpret_cast<const f32x4*>(x)[2 * i], b = reinterpret_cast<const f32x4*>(x)[2 * i + 1];
    const f32x4 g0 = *reinterpret_cast<const f32x4*>(gamma + c), g1 = *reinterpret_cast<const f32x4*>(gamma + c + 4);
#pragma unroll
    for (int e = 0; e < 4; e++) { a[e] = fmaf(g0[e], (float)v[e], a[e]); b[e] = fmaf(g1[e], (float)v[4 + e], b[e]); }
    reinterpret_cast<f32x4*>(x)[2 * i] = a;
    reinterpret_cast<f32x4*>(x)[2 * i + 1] = b;
  }
}

// P[r][:] = softmax(scale * S[r][:]) for bf16 scores (the rounded QK^T of the encoder's attention), f32 inside, bf16 out; one wave
// per row, cols <= 512.  Replaces the scale multiply, the f32 up-cast, softmax and the bf16 down-cast (four ATen kernels).
__global__ __launch_bounds__(256) void softmax_bf16_kernel(const bf16* __restrict__ s, bf16* __restrict__ p, size_t rows, int cols, float scale) {
  const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const bf16* sr = s + row * cols;
  float v[8];
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const int c = lane + k * 64;
    v[k] = c < cols ? (float)sr[c] * scale : -INFINITY;
    m = fmaxf(m, v[k]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < 8; k++) { v[k] = __expf(v[k] - m); sum += v[k]; }
  const float inv = 1.f / wave_sum(sum);
  bf16* pr = p + row * cols;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const int c = lane + k * 64;
    if (c < cols) pr[c] = (bf16)(v[k] * inv);
  }
}

}  // namespace dmvae_vit
using namespace dmvae_vit;

extern "C" int dmvae_layernorm_f32_bf16(const void* x, const void* gamma, const void* beta, void* y, int rows, int c, float eps,
                                        hipStream_t stream) {
  DMVAE_CHECK_ARG(x && gamma && beta && y && rows > 0, "layernorm_f32_bf16: bad argument");
  DMVAE_CHECK_ARG(c == 256 || c == 384 || c == 512 || c == 768 || c == 1024 || c == 1280 || c == 1536,
                  "layernorm_f32_bf16: width must be 384 or a multiple of 256 up to 1536 (got %d)", c);
  const dim3 grid((rows + 3) / 4), block(256);
  if (c == 384) {
    hipLaunchKernelGGL((layernorm_kernel<1, false, true>), grid, block, 0, stream, (float*)x, (const float*)gamma, (const float*)beta, (bf16*)y, rows, eps, nullptr, nullptr);
    DMVAE_CHECK_LAUNCH();
    return 0;
  }
  switch (c / 256) {
    case 1: hipLaunchKernelGGL(layernorm_kernel<1>, grid, block, 0, stream, (float*)x, (const float*)gamma, (const float*)beta, (bf16*)y, rows, eps, nullptr, nullptr); break;
    case 2: hipLaunchKernelGGL(layernorm_kernel<2>, grid, block, 0, stream, (float*)x, (const float*)gamma, (const float*)beta, (bf16*)y, rows, eps, nullptr, nullptr); break;
    case 3: hipLaunchKernelGGL(layernorm_kernel<3>, grid, block, 0, stream, (float*)x, (const float*)gamma, (const float*)beta, (bf16*)y, rows, eps, nullptr, nullptr); break;
    case 4: hipLaunchKernelGGL(layernorm_kernel<4>, grid, block, 0, stream, (float*)x, (const float*)gamma, (const float*)beta, (bf16*)y, rows, eps, nullptr, nullptr); break;
    case 5: hipLaunchKernelGGL(layernorm_kernel<5>, grid, block, 0, stream, (float*)x, (const float*)gamma, (const float*)beta, (bf16*)y, rows, eps, nullptr, nullptr); break;
    default: hipLaunchKernelGGL(layernorm_kernel<6>, grid, block, 0, stream, (float*)x, (const float*)gamma, (const float*)beta, (bf16*)y, rows, eps, nullptr, nullptr); break;
  }
  DMVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int dmvae_scale_residual_layernorm(void* x, const void* r, const void* ls_gamma, const void* gamma, const void* beta, void* y, int rows, int c,
                                              float eps, hipStream_t stream) {
  DMVAE_CHECK_ARG(x && r && ls_gamma && gamma && beta && y && rows > 0, "scale_residual_layernorm: bad argument");
  DMVAE_CHECK_ARG(c == 256 || c == 384 || c == 512 || c == 768 || c == 1024 || c == 1280 || c == 1536,
                  "scale_residual_layernorm: width must be 384 or a multiple of 256 up to 1536 (got %d)", c);
  const dim3 grid((rows + 3) / 4), block(256);
  if (c == 384) {
    hipLaunchKernelGGL((layernorm_kernel<1, true, true>), grid, block, 0, stream, (float*)x, (const float*)gamma, (const float*)beta, (bf16*)y, rows, eps,
                       (const bf16*)r, (const float*)ls_gamma);
    DMVAE_CHECK_LAUNCH();
    return 0;
  }
#define DMVAE_SRLN(S) hipLaunchKernelGGL((layernorm_kernel<S, true>), grid, block, 0, stream, (float*)x, (const float*)gamma, (const float*)beta, (bf16*)y, rows, eps, \
                                         (const bf16*)r, (const float*)ls_gamma)
  switch (c / 256) {
    case 1: DMVAE_SRLN(1); break;
    case 2: DMVAE_SRLN(2); break;
    case 3: DMVAE_SRLN(3); break;
    case 4: DMVAE_SRLN(4); break;
    case 5: DMVAE_SRLN(5); break;
    default: DMVAE_SRLN(6); break;
  }
#undef DMVAE_SRLN
  DMVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int dmvae_scale_residual_f32(void* x, const void* y, const void* gamma, size_t rows, int c, hipStream_t stream) {
  DMVAE_CHECK_ARG(x && y && gamma && c > 0 && c % 8 == 0, "scale_residual_f32: width must be a multiple of 8");
  if (rows == 0) return 0;
  const size_t n8 = rows * (size_t)(c / 8);
  size_t nb = (n8 + 255) / 256; if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(scale_residual_kernel, dim3((unsigned)nb), dim3(256), 0, stream, (float*)x, (const bf16*)y, (const float*)gamma, n8, c / 8);
  DMVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int dmvae_softmax_rows_bf16(const void* s, void* p, size_t rows, int cols, float scale, hipStream_t stream) {
  DMVAE_CHECK_ARG(s && p && cols > 0 && cols <= 512, "softmax_rows_bf16: cols must be in 1..512 (got %d)", cols);
  if (rows == 0) return 0;
  hipLaunchKernelGGL(softmax_bf16_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, (const bf16*)s, (bf16*)p, rows, cols, scale);
  DMVAE_CHECK_LAUNCH();
  return 0;
}
