// Convolution along the TOKEN axis of token-major bf16 activations [B][L][C] (C -> C channels, odd kernel size ks <= 9, zero padding ks / 2 per sample):
//
//   y[b][l][co] = bias[co] + sum_t sum_ci x[b][l + t - ks/2][ci] * W[co][ci][t]
//
// the Conv1d(C, C, ks, padding = ks / 2) of the DINOv2 discriminator's heads (reference: models/dinodisc.py:73-105, applied there to [B, C, L]; ks = 9 from
// train_tokenizer.py:307-312), stated on the layout the ViT's tokens already have, so that nothing is transposed between the backbone and the heads.
//
//   forward / input gradient : ONE kernel.  The input gradient dx[b][l][ci] = sum_t sum_co dy[b][l - t + ks/2][co] * W[co][ci][t] is the same convolution of dy
//       with the taps reversed and the channel roles swapped, so it runs on a second pack of the weight.  A token's operand rows are read where they lie: the
//       row for tap t is the neighbouring token's row, a row outside the sample is a zero fragment -- no ks-times-expanded operand exists anywhere.
//       Workgroup = 64 tokens of one sample x 128 output channels, wave = 32 x 64 (2 x 4 v_mfma_f32_16x16x32_bf16 accumulators), fragments straight from global
//       memory (L1 / L2 serve the ks-fold re-reads), f32 accumulation in a fixed order.  A sample's result does not depend on the batch it is in.
//   weight + bias gradient   : dW[co][ci][t] = sum_{b,l} dy[b][l][co] * x[b][l + t - ks/2][ci]: the reduction runs over tokens, the slow axis of both operands.
//       32-token chunks of dy (64 co) and x (64 ci, + ks - 1 halo rows) are staged in LDS; a wave owns 16 co x 64 ci x all taps.  The chunks are dealt to
//       `splits` workgroups per tile in contiguous ranges, each writes its partial sums, a second kernel adds them in split order: no atomics, reruns identical.
//   pack                     : both operand packs, bf16 [C_out][ks][C_in] (forward) and [C_in][ks reversed][C_out] (input gradient), from the f32 Conv1d weight
//       divided by the spectral norm's sigma (a device scalar; NULL = 1) in one pass.
#include "common.h"
#include "dmvae_hip.h"

namespace dmvae_conv_tokens {

constexpr int MAX_KS = 9;
constexpr int WG_SPLITS_MAX = 16;
constexpr int DB_PARTS = 64;

// w: f32 [C][C][ks] (Conv1d: out, in, tap).  wf[co][t][ci] = w[co][ci][t] / sigma;  wd[ci][t][co] = w[co][ci][ks - 1 - t] / sigma (an f32 division per element: the
// value torch's W / sigma has).
__global__ __launch_bounds__(256) void pack_kernel(const float* __restrict__ w, const float* __restrict__ sigma, bf16* __restrict__ wf, bf16* __restrict__ wd,
                                                   int C, int ks) {
  const size_t n = (size_t)C * C * ks;
  const float sg = sigma ? sigma[0] : 1.0f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const int t = (int)(i % ks);
    const size_t oc = i / ks;
    const int ci = (int)(oc % C), co = (int)(oc / C);
    const bf16 v = (bf16)(w[i] / sg);
    wf[((size_t)co * ks + t) * C + ci] = v;
    wd[((size_t)ci * ks + (ks - 1 - t)) * C + co] = v;
  }
}

// y[b][l][n] = bias[n] + sum_t sum_k x[b][l + t - ks/2][k] * w[n][t][k].  grid (ceil(L / 64), ceil(C / 128), B), 4 waves = 2 (tokens) x 2 (channels).
// res (or NULL): a bf16 tensor of y's shape added in f32 before the one rounding (the input gradient's second summand where the conv's input also feeds a skip).
// The epilogue is a template parameter.  EPI_PLAIN: y = bf16(acc + bias + res).  EPI_BNACT: an eval-mode BatchNorm + LeakyReLU(0.2) on the conv's result
// (constant statistics: a per-channel affine map), y = bf16(leaky((acc + bias - mean) * rsqrt(var + eps) * gamma + beta)) in f32 with the one rounding; the four
// per-channel f32 vectors are read as the bias is, a float4 per four channels.
enum { EPI_PLAIN = 0, EPI_BNACT = 1 };
struct BnAct {
  const float* mean;
  const float* var;
  const float* gamma;
  const float* beta;
  float eps;
};

template <int EPI>
__global__ __launch_bounds__(256) void conv_tokens_kernel(const bf16* __restrict__ x, const bf16* __restrict__ w, const float* __restrict__ bias,
                                                          const bf16* __restrict__ res, bf16* __restrict__ y, int L, int C, int ks, BnAct bn) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, kc = (lane >> 4) * 8;
  const int l0 = blockIdx.x * 64 + (wave & 1) * 32, n0 = blockIdx.y * 128 + (wave >> 1) * 64;
  if (l0 >= L || n0 >= C) return;                       // wave-uniform; the kernel has no barrier
  const int p = ks >> 1;
  const bf16* xb = x + (size_t)blockIdx.z * L * C;
  const bf16* wp[4];
#pragma unroll
  for (int g = 0; g < 4; g++) {
    const int n = n0 + g * 16 + r;
    wp[g] = w + (size_t)(n < C ? n : C - 1) * ks * C + kc;      // channel rows past C: a valid row, never stored
  }
  f32x4 acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int g = 0; g < 4; g++) acc[i][g] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int t = 0; t < ks; t++) {
    const bf16* xp[2];
    bool ok[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
      const int src = l0 + i * 16 + r + t - p;          // the token whose row tap t multiplies
      ok[i] = src >= 0 && src < L;
      xp[i] = xb + (size_t)(ok[i] ? src : 0) * C + kc;
    }
#pragma unroll 2
    for (int k = 0; k < C; k += 32) {
      bf16x8 xf[2], wf[4];
#pragma unroll
      for (int i = 0; i < 2; i++) {
        xf[i] = *reinterpret_cast<const bf16x8*>(xp[i] + k);
        if (!ok[i]) xf[i] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};   // a row outside the sample is the zero padding
      }
#pragma unroll
      for (int g = 0; g < 4; g++) wf[g] = *reinterpret_cast<const bf16x8*>(wp[g] + (size_t)t * C + k);
#pragma unroll
      for (int i = 0; i < 2; i++)
#pragma unroll
        for (int g = 0; g < 4; g++) acc[i][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[g], xf[i], acc[i][g], 0, 0, 0);
    }
  }
  // lane l holds token l0 + 16 i + (l & 15), channels n0 + 16 g + 4 (l >> 4) + j
#pragma unroll
  for (int i = 0; i < 2; i++) {
    const int l = l0 + i * 16 + r;
    if (l >= L) continue;
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const int n = n0 + g * 16 + (lane >> 4) * 4;
      if (n >= C) continue;                              // C % 32 == 0: a group of four is inside or outside as a whole
      f32x4 b = {0.f, 0.f, 0.f, 0.f};
      if (bias) b = *reinterpret_cast<const f32x4*>(bias + n);
      const size_t off = ((size_t)blockIdx.z * L + l) * C + n;
      bf16x4 o;
      if constexpr (EPI == EPI_BNACT) {
        const f32x4 mu = *reinterpret_cast<const f32x4*>(bn.mean + n), va = *reinterpret_cast<const f32x4*>(bn.var + n);
        const f32x4 ga = *reinterpret_cast<const f32x4*>(bn.gamma + n), be = *reinterpret_cast<const f32x4*>(bn.beta + n);
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const float v = (acc[i][g][j] + b[j] - mu[j]) * rsqrtf(va[j] + bn.eps) * ga[j] + be[j];
          o[j] = (bf16)(v > 0.f ? v : 0.2f * v);
        }
      } else {
        if (res) {
          const bf16x4 rv = *reinterpret_cast<const bf16x4*>(res + off);
#pragma unroll
          for (int j = 0; j < 4; j++) b[j] += (float)rv[j];
        }
#pragma unroll
        for (int j = 0; j < 4; j++) o[j] = (bf16)(acc[i][g][j] + b[j]);
      }
      *reinterpret_cast<bf16x4*>(y + off) = o;
    }
  }
}

constexpr int WG_ROW = 66;    // LDS row stride in bf16 (33 dwords): the four 8-token groups of a fragment read land 8 banks apart

// part[split][t][co][ci] = sum over the split's chunks of dy[tok][co] * x[tok + t - KS/2][ci].  grid (C / 64 ci tiles, C / 64 co tiles, splits).
template <int KS>
__global__ __launch_bounds__(256) void wgrad_kernel(const bf16* __restrict__ dy, const bf16* __restrict__ x, float* __restrict__ part, int B, int L, int C,
                                                    int chunks_per_sample, int chunks_per_split) {
  __shared__ __attribute__((aligned(16))) bf16 sdy[32 * WG_ROW];
  __shared__ __attribute__((aligned(16))) bf16 sx[(32 + KS - 1) * WG_ROW];
  constexpr int P = KS / 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int ci0 = blockIdx.x * 64, co0 = blockIdx.y * 64;
  const int total = B * chunks_per_sample;
  const int c_begin = blockIdx.z * chunks_per_split, c_end = min(total, c_begin + chunks_per_split);
  f32x4 acc[4][KS];
#pragma unroll
  for (int f = 0; f < 4; f++)
#pragma unroll
    for (int t = 0; t < KS; t++) acc[f][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int ch = c_begin; ch < c_end; ch++) {             // block-uniform bounds: every thread reaches both barriers
    const int b = ch / chunks_per_sample, l0 = (ch - b * chunks_per_sample) * 32;
    const bf16* dyb = dy + (size_t)b * L * C;
    const bf16* xb = x + (size_t)b * L * C;
    __syncthreads();                                     // the previous chunk's reads are done
    for (int i = threadIdx.x; i < 32 * 8; i += 256) {    // dy: 32 rows x 8 pieces of 8 channels
      const int row = i >> 3, c8 = (i & 7) * 8, l = l0 + row;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (l < L) v = *reinterpret_cast<const uint4*>(dyb + (size_t)l * C + co0 + c8);
      unsigned* d = reinterpret_cast<unsigned*>(sdy + row * WG_ROW + c8);
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    for (int i = threadIdx.x; i < (32 + KS - 1) * 8; i += 256) {   // x: rows l0 - P ... l0 + 31 + P, zero outside the sample
      const int row = i >> 3, c8 = (i & 7) * 8, l = l0 + row - P;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (l >= 0 && l < L) v = *reinterpret_cast<const uint4*>(xb + (size_t)l * C + ci0 + c8);
      unsigned* d = reinterpret_cast<unsigned*>(sx + row * WG_ROW + c8);
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    __syncthreads();
    // A = dy^T: lane holds channel co0 + 16 wave + r at tokens 8 q + j;  B = x^T shifted by the tap: channel ci0 + 16 f + r at tokens 8 q + j + t
    bf16x8 af;
#pragma unroll
    for (int j = 0; j < 8; j++) af[j] = sdy[(8 * q + j) * WG_ROW + wave * 16 + r];
#pragma unroll
    for (int f = 0; f < 4; f++) {
      bf16 col[8 + KS - 1];
#pragma unroll
      for (int j = 0; j < 8 + KS - 1; j++) col[j] = sx[(8 * q + j) * WG_ROW + f * 16 + r];
#pragma unroll
      for (int t = 0; t < KS; t++) {
        bf16x8 bfr;
#pragma unroll
        for (int j = 0; j < 8; j++) bfr[j] = col[j + t];
        acc[f][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bfr, acc[f][t], 0, 0, 0);
      }
    }
  }
  // lane holds co = co0 + 16 wave + 4 q + j, ci = ci0 + 16 f + r
  float* pz = part + (size_t)blockIdx.z * KS * C * C;
#pragma unroll
  for (int f = 0; f < 4; f++)
#pragma unroll
    for (int t = 0; t < KS; t++)
#pragma unroll
      for (int j = 0; j < 4; j++) pz[((size_t)t * C + co0 + wave * 16 + q * 4 + j) * C + ci0 + f * 16 + r] = acc[f][t][j];
}

// dw[co][ci][t] = sum_s part[s][t][co][ci], in split order
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw, int C, int ks, int splits) {
  const size_t n = (size_t)ks * C * C;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    float s = 0.f;
    for (int z = 0; z < splits; z++) s += part[(size_t)z * n + i];
    const int ci = (int)(i % C);
    const size_t tc = i / C;
    const int co = (int)(tc % C), t = (int)(tc / C);
    dw[((size_t)co * C + ci) * ks + t] = s;
  }
}

// part[blockIdx.y][c] = sum of dy's rows of this block's range; grid (C / 64, DB_PARTS), 4 row groups x 64 channels, combined in a fixed order
__global__ __launch_bounds__(256) void dbias_parts_kernel(const bf16* __restrict__ dy, float* __restrict__ part, size_t rows, int C) {
  __shared__ float red[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), grp = threadIdx.x >> 6;
  const size_t per = (rows + DB_PARTS - 1) / DB_PARTS;
  const size_t r0 = blockIdx.y * per, r1 = r0 + per < rows ? r0 + per : rows;
  float a = 0.f;
#pragma unroll 4
  for (size_t row = r0 + grp; row < r1; row += 4) a += (float)dy[row * C + c];
  red[grp][threadIdx.x & 63] = a;
  __syncthreads();
  if (grp == 0) part[(size_t)blockIdx.y * C + c] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}
__global__ __launch_bounds__(64) void dbias_final_kernel(const float* __restrict__ part, float* __restrict__ db, int C) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= C) return;
  float s = 0.f;
  for (int i = 0; i < DB_PARTS; i++) s += part[(size_t)i * C + c];
  db[c] = s;
}

static bool shape_ok(int b, int l, int c, int ks) {
  return b > 0 && b <= 65535 && l > 0 && c >= 384 && c % 32 == 0 && c <= 4096 && ks >= 1 && ks <= MAX_KS && (ks & 1) && (long long)b * l * c < (1LL << 31);
}
static int wgrad_splits(int b, int l) {
  const int total = b * ((l + 31) / 32);
  return total < WG_SPLITS_MAX ? total : WG_SPLITS_MAX;
}

static int launch_conv(const void* x, const void* w, const void* bias, const void* res, void* y, int b, int l, int c, int ks, hipStream_t stream,
                       const BnAct* bn = nullptr) {
  const dim3 grid((l + 63) / 64, (c + 127) / 128, b);
  if (bn)
    hipLaunchKernelGGL(conv_tokens_kernel<EPI_BNACT>, grid, dim3(256), 0, stream, (const bf16*)x, (const bf16*)w, (const float*)bias, (const bf16*)res, (bf16*)y, l,
                       c, ks, *bn);
  else
    hipLaunchKernelGGL(conv_tokens_kernel<EPI_PLAIN>, grid, dim3(256), 0, stream, (const bf16*)x, (const bf16*)w, (const float*)bias, (const bf16*)res, (bf16*)y, l,
                       c, ks, BnAct{nullptr, nullptr, nullptr, nullptr, 0.f});
  DMVAE_CHECK_LAUNCH();
  return 0;
}

}  // namespace dmvae_conv_tokens
using namespace dmvae_conv_tokens;

#define CONV_TOKENS_SHAPE_MSG "C must be a multiple of 32 in 384..4096, ks odd in 1..9, 1 <= B <= 65535, L >= 1 and B*L*C < 2^31 (got B %d L %d C %d ks %d)"

extern "C" int dmvae_conv_tokens_pack(const void* w, const void* sigma, void* w_fwd, void* w_dgrad, int c, int ks, hipStream_t stream) {
  DMVAE_CHECK_ARG(w && w_fwd && w_dgrad, "conv_tokens_pack: bad argument");
  DMVAE_CHECK_ARG(shape_ok(1, 1, c, ks), "conv_tokens_pack: " CONV_TOKENS_SHAPE_MSG, 1, 1, c, ks);
  hipLaunchKernelGGL(pack_kernel, dim3(grid_for((size_t)c * c * ks, 256, 2048)), dim3(256), 0, stream, (const float*)w, (const float*)sigma, (bf16*)w_fwd,
                     (bf16*)w_dgrad, c, ks);
  DMVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int dmvae_conv_tokens_fwd(const void* x, const void* w_fwd, const void* bias, void* y, int b, int l, int c, int ks, hipStream_t stream) {
  DMVAE_CHECK_ARG(x && w_fwd && y, "conv_tokens_fwd: bad argument");
  DMVAE_CHECK_ARG(shape_ok(b, l, c, ks), "conv_tokens_fwd: " CONV_TOKENS_SHAPE_MSG, b, l, c, ks);
  return launch_conv(x, w_fwd, bias, nullptr, y, b, l, c, ks, stream);
}

extern "C" int dmvae_conv_tokens_fwd_bnact(const void* x, const void* w_fwd, const void* bias, const void* running_mean, const void* running_var,
                                           const void* gamma, const void* beta, float eps, void* y, int b, int l, int c, int ks, hipStream_t stream) {
  DMVAE_CHECK_ARG(x && w_fwd && y && running_mean && running_var && gamma && beta, "conv_tokens_fwd_bnact: bad argument");
  DMVAE_CHECK_ARG(shape_ok(b, l, c, ks), "conv_tokens_fwd_bnact: " CONV_TOKENS_SHAPE_MSG, b, l, c, ks);
  const BnAct bn{(const float*)running_mean, (const float*)running_var, (const float*)gamma, (const float*)beta, eps};
  return launch_conv(x, w_fwd, bias, nullptr, y, b, l, c, ks, stream, &bn);
}

extern "C" int dmvae_conv_tokens_dgrad(const void* dy, const void* w_dgrad, const void* dres, void* dx, int b, int l, int c, int ks, hipStream_t stream) {
  DMVAE_CHECK_ARG(dy && w_dgrad && dx, "conv_tokens_dgrad: bad argument");
  DMVAE_CHECK_ARG(shape_ok(b, l, c, ks), "conv_tokens_dgrad: " CONV_TOKENS_SHAPE_MSG, b, l, c, ks);
  return launch_conv(dy, w_dgrad, nullptr, dres, dx, b, l, c, ks, stream);
}

extern "C" size_t dmvae_conv_tokens_wgrad_workspace(int b, int l, int c, int ks) {
  if (!shape_ok(b, l, c, ks) || c % 64 != 0) return 0;
  return ((size_t)wgrad_splits(b, l) * ks * c * c + (size_t)DB_PARTS * c) * sizeof(float);
}

extern "C" int dmvae_conv_tokens_wgrad(const void* dy, const void* x, void* dw, void* dbias, void* workspace, size_t workspace_bytes, int b, int l, int c, int ks,
                                       hipStream_t stream) {
  DMVAE_CHECK_ARG(dy && x && dw && workspace, "conv_tokens_wgrad: bad argument");
  DMVAE_CHECK_ARG(shape_ok(b, l, c, ks), "conv_tokens_wgrad: " CONV_TOKENS_SHAPE_MSG, b, l, c, ks);
  DMVAE_CHECK_ARG(c % 64 == 0, "conv_tokens_wgrad: C must be a multiple of 64 (got %d)", c);
  DMVAE_CHECK_ARG(workspace_bytes >= dmvae_conv_tokens_wgrad_workspace(b, l, c, ks), "conv_tokens_wgrad: workspace too small");
  const int cps = (l + 31) / 32, total = b * cps, splits = wgrad_splits(b, l), per = (total + splits - 1) / splits;
  float* part = (float*)workspace;
  const dim3 grid(c / 64, c / 64, splits);
#define DMVAE_CTW(K) hipLaunchKernelGGL(wgrad_kernel<K>, grid, dim3(256), 0, stream, (const bf16*)dy, (const bf16*)x, part, b, l, c, cps, per)
  switch (ks) {
    case 1: DMVAE_CTW(1); break;
    case 3: DMVAE_CTW(3); break;
    case 5: DMVAE_CTW(5); break;
    case 7: DMVAE_CTW(7); break;
    default: DMVAE_CTW(9); break;
  }
#undef DMVAE_CTW
  DMVAE_CHECK_LAUNCH();
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(grid_for((size_t)ks * c * c, 256, 2048)), dim3(256), 0, stream, part, (float*)dw, c, ks, splits);
  DMVAE_CHECK_LAUNCH();
  if (dbias) {
    float* bp = part + (size_t)splits * ks * c * c;
    hipLaunchKernelGGL(dbias_parts_kernel, dim3(c / 64, DB_PARTS), dim3(256), 0, stream, (const bf16*)dy, bp, (size_t)b * l, c);
    DMVAE_CHECK_LAUNCH();
    hipLaunchKernelGGL(dbias_final_kernel, dim3(c / 64), dim3(64), 0, stream, bp, (float*)dbias, c);
    DMVAE_CHECK_LAUNCH();
  }
  return 0;
}
