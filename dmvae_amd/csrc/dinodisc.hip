// The small passes around the heads of the DINOv2 discriminator (reference: models/dinodisc.py:166-193), on the layout the ViT's residual stream has:
//
//   tap       act[b][l][:] = bf16(t[b][1 + l][:] + t[b][0][:])            patch tokens + class token of the un-normed f32 stream t [B][1 + L][C]  (dinodisc.py:181-185)
//   un-tap    dt[b][1 + l][:] = dact[b][l][:],  dt[b][0][:] = sum_l dact[b][l][:]      its adjoint, the class row summed in f32 in a fixed order
//   tail      logit[r] = <(a[r] + h[r]) / sqrt 2, w> + bias                the ResidualBlock's (fn(x) + x) / sqrt 2 (dinodisc.py:13-20) and the closing C -> 1 conv of
//                                                                          kernel size 1 (dinodisc.py:138) in one pass over the two bf16 operands; f32 logits
//   tail bwd  da = dh = bf16(dlogit[r] * w / sqrt 2);  dw = sum_r dlogit[r] (a[r] + h[r]) / sqrt 2;  dbias = sum_r dlogit[r]      per-block partial sums + a
//                                                                          fixed-order second stage (no atomics)
//   bnact bwd g[r][c] = bf16(dy[r][c] * (y[r][c] > 0 ? 1 : 0.2) * gamma[c] * rsqrt(running_var[c] + eps))      the backward of an eval-mode BatchNorm + LeakyReLU(0.2)
//                                                                          (constant statistics) from the stored bf16 output y: LeakyReLU keeps the sign
// All five are HBM-bound single passes.
#include "common.h"
#include "dmvae_hip.h"

namespace dmvae_dinodisc {

constexpr float RSQRT2 = 0.70710678118654752f;
constexpr int TAIL_MAX_BLOCKS = 256;
constexpr int TAIL_MAXK = 8;          // C <= 1024: a lane holds 2 channels of every 128

__global__ __launch_bounds__(256) void tap_kernel(const float* __restrict__ t, bf16* __restrict__ act, int B, int L, int C) {
  const int c4 = C / 4;
  const size_t n = (size_t)B * L * c4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const int c = (int)(i % c4) * 4;
    const size_t bl = i / c4;
    const int l = (int)(bl % L), b = (int)(bl / L);
    const float* tb = t + (size_t)b * (L + 1) * C;
    const f32x4 p = *reinterpret_cast<const f32x4*>(tb + (size_t)(1 + l) * C + c), k = *reinterpret_cast<const f32x4*>(tb + c);
    bf16x4 o;
#pragma unroll
    for (int e = 0; e < 4; e++) o[e] = (bf16)(p[e] + k[e]);
    *reinterpret_cast<bf16x4*>(act + bl * C + c) = o;
  }
}

// grid (C / 64, B); 4 row groups x 64 channels
__global__ __launch_bounds__(256) void untap_kernel(const bf16* __restrict__ dact, float* __restrict__ dt, int L, int C) {
  __shared__ float red[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), grp = threadIdx.x >> 6, b = blockIdx.y;
  const bf16* src = dact + (size_t)b * L * C;
  float* dst = dt + (size_t)b * (L + 1) * C;
  float a = 0.f;
  for (int l = grp; l < L; l += 4) {
    const float v = (float)src[(size_t)l * C + c];
    dst[(size_t)(1 + l) * C + c] = v;
    a += v;
  }
  red[grp][threadIdx.x & 63] = a;
  __syncthreads();
  if (grp == 0) dst[c] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// one wave per row; lane holds channels 128 k + 2 lane, + 1
__global__ __launch_bounds__(256) void tail_fwd_kernel(const bf16* __restrict__ a, const bf16* __restrict__ h, const float* __restrict__ w,
                                                       const float* __restrict__ bias, float* __restrict__ logit, size_t rows, int C) {
  const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  float s = 0.f;
  for (int c = lane * 2; c < C; c += 128) {
    const bf16x2 av = *reinterpret_cast<const bf16x2*>(a + row * C + c), hv = *reinterpret_cast<const bf16x2*>(h + row * C + c);
    const f32x2 wv = *reinterpret_cast<const f32x2*>(w + c);
    s = fmaf((float)av[0] + (float)hv[0], wv[0], s);
    s = fmaf((float)av[1] + (float)hv[1], wv[1], s);
  }
  s = wave_sum(s);
  if (lane == 0) logit[row] = fmaf(s, RSQRT2, bias ? bias[0] : 0.f);
}

// part[blk][C + 1]: the block's sums of dlogit (a + h) per channel and, last, of dlogit.  a / h NULL: no parameter sums (frozen heads)
__global__ __launch_bounds__(256) void tail_bwd_kernel(const float* __restrict__ dlogit, const bf16* __restrict__ a, const bf16* __restrict__ h,
                                                       const float* __restrict__ w, bf16* __restrict__ dah, float* __restrict__ part, size_t rows, int C) {
  extern __shared__ float red[];      // [4][C + 1]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nk = C / 128;
  f32x2 wv[TAIL_MAXK], acc[TAIL_MAXK];
  float accb = 0.f;
#pragma unroll
  for (int k = 0; k < TAIL_MAXK; k++) {
    acc[k] = f32x2{0.f, 0.f};
    wv[k] = f32x2{0.f, 0.f};
    if (k < nk) { wv[k] = *reinterpret_cast<const f32x2*>(w + k * 128 + lane * 2); wv[k][0] *= RSQRT2; wv[k][1] *= RSQRT2; }
  }
  for (size_t row = (size_t)blockIdx.x * 4 + wave; row < rows; row += (size_t)gridDim.x * 4) {
    const float d = dlogit[row];
    accb += d;
#pragma unroll
    for (int k = 0; k < TAIL_MAXK; k++)
      if (k < nk) {
        const size_t off = row * C + k * 128 + lane * 2;
        if (dah) {
          bf16x2 o = {(bf16)(d * wv[k][0]), (bf16)(d * wv[k][1])};
          *reinterpret_cast<bf16x2*>(dah + off) = o;
        }
        if (part) {
          const bf16x2 av = *reinterpret_cast<const bf16x2*>(a + off), hv = *reinterpret_cast<const bf16x2*>(h + off);
          acc[k][0] = fmaf(d, (float)av[0] + (float)hv[0], acc[k][0]);
          acc[k][1] = fmaf(d, (float)av[1] + (float)hv[1], acc[k][1]);
        }
      }
  }
  if (!part) return;                   // block-uniform
  float* rw = red + wave * (C + 1);
#pragma unroll
  for (int k = 0; k < TAIL_MAXK; k++)
    if (k < nk) { rw[k * 128 + lane * 2] = acc[k][0]; rw[k * 128 + lane * 2 + 1] = acc[k][1]; }
  if (lane == 0) rw[C] = accb;
  __syncthreads();
  for (int i = threadIdx.x; i <= C; i += 256)
    part[(size_t)blockIdx.x * (C + 1) + i] = (red[i] + red[(C + 1) + i]) + (red[2 * (C + 1) + i] + red[3 * (C + 1) + i]);
}

__global__ __launch_bounds__(256) void tail_bwd_final_kernel(const float* __restrict__ part, float* __restrict__ dw, float* __restrict__ dbias, int nblk, int C) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i > C) return;
  float s = 0.f;
  for (int b = 0; b < nblk; b++) s += part[(size_t)b * (C + 1) + i];
  if (i < C) dw[i] = s * RSQRT2;
  else if (dbias) dbias[0] = s;
}

// bf16x8 pieces; C % 8 == 0, so a piece lies in one row
__global__ __launch_bounds__(256) void bnact_bwd_kernel(const bf16* __restrict__ dy, const bf16* __restrict__ y, const float* __restrict__ gamma,
                                                        const float* __restrict__ var, float eps, bf16* __restrict__ g, size_t rows, int C) {
  const int c8 = C / 8;
  const size_t n = rows * c8;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const int c = (int)(i % c8) * 8;
    const bf16x8 dv = *reinterpret_cast<const bf16x8*>(dy + i * 8), yv = *reinterpret_cast<const bf16x8*>(y + i * 8);
    bf16x8 o;
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const f32x4 ga = *reinterpret_cast<const f32x4*>(gamma + c + 4 * h), va = *reinterpret_cast<const f32x4*>(var + c + 4 * h);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int e = 4 * h + j;
        o[e] = (bf16)((float)dv[e] * ((float)yv[e] > 0.f ? 1.0f : 0.2f) * ga[j] * rsqrtf(va[j] + eps));
      }
    }
    *reinterpret_cast<bf16x8*>(g + i * 8) = o;
  }
}

static int tail_blocks(size_t rows) {
  const size_t nb = (rows + 3) / 4;
  return (int)(nb < (size_t)TAIL_MAX_BLOCKS ? nb : (size_t)TAIL_MAX_BLOCKS);
}

}  // namespace dmvae_dinodisc
using namespace dmvae_dinodisc;

extern "C" int dmvae_dino_tap(const void* t, void* act, int b, int l, int c, hipStream_t stream) {
  DMVAE_CHECK_ARG(t && act && b > 0 && l > 0 && c > 0 && c % 4 == 0, "dino_tap: B, L >= 1 and C a multiple of 4 (got B %d L %d C %d)", b, l, c);
  hipLaunchKernelGGL(tap_kernel, dim3(grid_for((size_t)b * l * (c / 4), 256, 4096)), dim3(256), 0, stream, (const float*)t, (bf16*)act, b, l, c);
  DMVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int dmvae_dino_untap(const void* dact, void* dt, int b, int l, int c, hipStream_t stream) {
  DMVAE_CHECK_ARG(dact && dt && b > 0 && b <= 65535 && l > 0 && c > 0 && c % 64 == 0, "dino_untap: 1 <= B <= 65535, L >= 1 and C a multiple of 64 (got B %d L %d C %d)",
                  b, l, c);
  hipLaunchKernelGGL(untap_kernel, dim3(c / 64, b), dim3(256), 0, stream, (const bf16*)dact, (float*)dt, l, c);
  DMVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int dmvae_dino_tail_fwd(const void* a, const void* h, const void* w, const void* bias, void* logit, size_t rows, int c, hipStream_t stream) {
  DMVAE_CHECK_ARG(a && h && w && logit && rows > 0 && rows < (1u << 31), "dino_tail_fwd: bad argument");
  DMVAE_CHECK_ARG(c > 0 && c % 128 == 0 && c <= 128 * TAIL_MAXK, "dino_tail: C must be a multiple of 128 up to 1024 (got %d)", c);
  hipLaunchKernelGGL(tail_fwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, (const bf16*)a, (const bf16*)h, (const float*)w, (const float*)bias,
                     (float*)logit, rows, c);
  DMVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t dmvae_dino_tail_bwd_workspace(size_t rows, int c) {
  if (rows == 0 || c <= 0 || c % 128 != 0 || c > 128 * TAIL_MAXK) return 0;
  return (size_t)tail_blocks(rows) * (c + 1) * sizeof(float);
}

extern "C" int dmvae_dino_tail_bwd(const void* dlogit, const void* a, const void* h, const void* w, void* dah, void* dw, void* dbias, void* workspace,
                                   size_t workspace_bytes, size_t rows, int c, hipStream_t stream) {
  DMVAE_CHECK_ARG(dlogit && w && rows > 0 && rows < (1u << 31) && (dah || dw), "dino_tail_bwd: bad argument");
  DMVAE_CHECK_ARG(c > 0 && c % 128 == 0 && c <= 128 * TAIL_MAXK, "dino_tail: C must be a multiple of 128 up to 1024 (got %d)", c);
  DMVAE_CHECK_ARG(!dw || (a && h && workspace && workspace_bytes >= dmvae_dino_tail_bwd_workspace(rows, c)), "dino_tail_bwd: the parameter sums need a, h and the workspace");
  const int nblk = tail_blocks(rows);
  hipLaunchKernelGGL(tail_bwd_kernel, dim3(nblk), dim3(256), dw ? 4 * (size_t)(c + 1) * sizeof(float) : 0, stream, (const float*)dlogit, (const bf16*)a,
                     (const bf16*)h, (const float*)w, (bf16*)dah, dw ? (float*)workspace : nullptr, rows, c);
  DMVAE_CHECK_LAUNCH();
  if (dw) {
    hipLaunchKernelGGL(tail_bwd_final_kernel, dim3((c + 1 + 255) / 256), dim3(256), 0, stream, (const float*)workspace, (float*)dw, (float*)dbias, nblk, c);
    DMVAE_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" int dmvae_dino_bnact_bwd(const void* dy, const void* y, const void* gamma, const void* running_var, float eps, void* g, size_t rows, int c,
                                    hipStream_t stream) {
  DMVAE_CHECK_ARG(dy && y && gamma && running_var && g && rows > 0 && c > 0 && c % 8 == 0 && rows * (size_t)c < ((size_t)1 << 31),
                  "dino_bnact_bwd: rows >= 1, C a multiple of 8 and rows * C < 2^31 (got rows %zu C %d)", rows, c);
  hipLaunchKernelGGL(bnact_bwd_kernel, dim3(grid_for(rows * (size_t)(c / 8), 256, 4096)), dim3(256), 0, stream, (const bf16*)dy, (const bf16*)y, (const float*)gamma,
                     (const float*)running_var, eps, (bf16*)g, rows, c);
  DMVAE_CHECK_LAUNCH();
  return 0;
}
