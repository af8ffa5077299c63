// SSIM of evaluation/metrics.py:16-23 (torchmetrics' StructuralSimilarityIndexMeasure at its defaults: 11 x 11 Gaussian window, sigma 1.5, k1 0.01, k2 0.03,
// reduction 'none') with the window moments in f64, one pass over the two images, the same bits from every run.
//
// Two facts about the torchmetrics algorithm (reflect-pad by 5, filter p, t, p^2, t^2, p t depthwise, form the SSIM map, crop 5 from every side, mean) shape
// the kernel; both were checked in f64 on the CPU (tests/ssim_spec.py, tests/test_ssim_cpu.py):
//   1. The padding never reaches the result.  After the crop every surviving output pixel's window lies wholly inside the unpadded image: the metric is a
//      VALID 11 x 11 filter over the raw H x W image averaged over its (H - 10) x (W - 10) outputs (the two formulations agree to <= 4e-13, the noise
//      between two f64 summation orders).  Hence H, W >= 11 (torchmetrics returns NaN from an empty mean below that; here it is an argument error) and no
//      reflect logic: output (oy, ox) reads rows oy .. oy + 10, columns ox .. ox + 10.
//   2. The clamp question is moot in f64.  Newer torchmetrics clamp the two variances at 0, older ones do not; in f64 the clamp changed no value by one bit
//      on any input tried, so there is none here.
//
// tile_kernel: one workgroup of 256 threads per (plane, 32 x 16 output tile).  The 42 x 26 input halo of both images goes to LDS as f32 (elements widened
// to f32, `(x + 1.0f) * 0.5f` in f32 when from_pm1 -- the reference's add(1).mul(0.5) on f32 tensors bit for bit -- 9.2 KB at a row pitch of 44); a thread
// issues its five loads per image before it uses the first, and a pixel past the image's edge is stored as 0 and never read from memory (the load goes to
// element 0 of the plane instead).  Everything after that is f64.  The horizontal pass gives a thread four adjacent output columns of one halo row: the 14
// pixels under the four windows are read once, their products p p, t t, p t formed once, and the five row sums of 26 x 32 positions written to LDS (33.3 KB;
// 42.5 KB in all, under the 64 KB that need no opt-in).  The vertical pass gives each thread two vertically adjacent outputs of one column (12 rows read for
// 2 x 11 taps; a wave reads 2 x 256 contiguous bytes per row: no bank conflict), forms the SSIM value with no FMA contraction (identical images give exactly
// 1), and zeroes outputs past (H - 10, W - 10).  The workgroup's sum is taken in a fixed order (xor-shuffle tree inside a wave, then the four waves in order)
// and stored to partial[plane * tiles + tile]: no atomics.
// finalize_kernel: one workgroup per image sums its C * tiles partials -- contiguous, since plane = b * C + c -- in a fixed order and divides by
// C (H - 10) (W - 10).  An image's value depends on its own pixels and the shape alone: the same bits alone or inside any batch.
// Planes x tiles lie flat on grid.x (2^31 - 1 blocks), never on an axis capped at 65535.
#include <math.h>

#include "common.h"
#include "dmvae_hip.h"

namespace dmvae_ssim_impl {

constexpr int WIN = 11;                   // window width; output (oy, ox) covers input rows oy .. oy + WIN - 1
constexpr int TW = 32, TH = 16;           // output tile
constexpr int IW = TW + WIN - 1;          // 42
constexpr int IH = TH + WIN - 1;          // 26
constexpr int IWP = 44;                   // f32 row pitch of the halo in LDS: every row starts 16-B aligned
constexpr int OPT = 4;                    // adjacent output columns per thread in the horizontal pass

struct Params {
  double g[WIN];                          // 1-D window weights; the 2-D window is their outer product
  double c1, c2;
};

__host__ __device__ inline size_t tiles_of(int h, int w) {
  return (size_t)((w - (WIN - 1) + TW - 1) / TW) * (size_t)((h - (WIN - 1) + TH - 1) / TH);
}

__device__ __forceinline__ double ssim_value(double mp, double mt, double epp, double ett, double ept, double c1, double c2) {
#pragma clang fp contract(off)
  const double mpp = mp * mp, mtt = mt * mt, mpt = mp * mt;
  const double sp = epp - mpp, st = ett - mtt, spt = ept - mpt;
  const double num = (2.0 * mpt + c1) * (2.0 * spt + c2);
  const double den = ((mpp + mtt) + c1) * ((sp + st) + c2);
  return num / den;
}

template <typename T>
__global__ __launch_bounds__(256) void tile_kernel(const T* __restrict__ a, const T* __restrict__ b, int h, int w, int tiles_x, unsigned tiles, int from_pm1,
                                                   Params p, double* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) float in[2][IH][IWP];
  __shared__ double hb[5][IH][TW];
  __shared__ double wsum[4];
  const int t = threadIdx.x;
  const unsigned tile = blockIdx.x % tiles;
  const size_t plane = blockIdx.x / tiles;
  const int y0 = (int)(tile / (unsigned)tiles_x) * TH, x0 = (int)(tile % (unsigned)tiles_x) * TW;
  const T* __restrict__ pa = a + plane * (size_t)h * (size_t)w;
  const T* __restrict__ pb = b + plane * (size_t)h * (size_t)w;

  // halo load: every thread's loads are issued before the first is used (one latency per tile, not one per pass of a loop).  A position outside the halo
  // or past the image's edge reads element 0 of the plane instead -- always inside it, so nothing outside the two images is read -- and is stored as 0.
  constexpr int NLD = (IH * IW + 255) / 256;
  T ra[NLD], rb[NLD];
  bool ok[NLD];
#pragma unroll
  for (int u = 0; u < NLD; u++) {
    const int i = t + 256 * u, r = i / IW, c = i - r * IW;
    const int y = y0 + r, x = x0 + c;
    ok[u] = i < IH * IW && y < h && x < w;
    const size_t o = ok[u] ? (size_t)y * (size_t)w + (size_t)x : 0;
    ra[u] = pa[o];
    rb[u] = pb[o];
  }
#pragma unroll
  for (int u = 0; u < NLD; u++) {
    const int i = t + 256 * u, r = i / IW, c = i - r * IW;
    float va = (float)ra[u], vb = (float)rb[u];
    if (from_pm1) {
      va = __fmul_rn(__fadd_rn(va, 1.0f), 0.5f);
      vb = __fmul_rn(__fadd_rn(vb, 1.0f), 0.5f);
    }
    if (i < IH * IW) {
      in[0][r][c] = ok[u] ? va : 0.f;
      in[1][r][c] = ok[u] ? vb : 0.f;
    }
  }
  __syncthreads();

  // horizontal pass: thread -> (halo row r, output columns c0 .. c0 + 3).  The 14 pixels under the four windows are read once (three 16-B reads and one 8-B
  // read per image) and their three products formed once; pixel j adds into output o with weight g[j - o], taps in ascending order for every output.
  if (t < IH * (TW / OPT)) {
    const int r = t / (TW / OPT), c0 = (t % (TW / OPT)) * OPT;
    float fa[OPT + WIN - 1], fb[OPT + WIN - 1];
#pragma unroll
    for (int v = 0; v < 3; v++) {
      const float4 qa = *reinterpret_cast<const float4*>(&in[0][r][c0 + 4 * v]), qb = *reinterpret_cast<const float4*>(&in[1][r][c0 + 4 * v]);
      fa[4 * v] = qa.x, fa[4 * v + 1] = qa.y, fa[4 * v + 2] = qa.z, fa[4 * v + 3] = qa.w;
      fb[4 * v] = qb.x, fb[4 * v + 1] = qb.y, fb[4 * v + 2] = qb.z, fb[4 * v + 3] = qb.w;
    }
    const float2 ta = *reinterpret_cast<const float2*>(&in[0][r][c0 + 12]), tb = *reinterpret_cast<const float2*>(&in[1][r][c0 + 12]);
    fa[12] = ta.x, fa[13] = ta.y, fb[12] = tb.x, fb[13] = tb.y;
    double acc[OPT][5];
#pragma unroll
    for (int o = 0; o < OPT; o++)
#pragma unroll
      for (int q = 0; q < 5; q++) acc[o][q] = 0.0;
#pragma unroll
    for (int j = 0; j < OPT + WIN - 1; j++) {
      const double x = (double)fa[j], y = (double)fb[j];
      const double v[5] = {x, y, x * x, y * y, x * y};
#pragma unroll
      for (int o = 0; o < OPT; o++) {
        if (j - o >= 0 && j - o < WIN) {
#pragma unroll
          for (int q = 0; q < 5; q++) acc[o][q] += p.g[j - o] * v[q];
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 5; q++)
#pragma unroll
      for (int o = 0; o < OPT; o++) hb[q][r][c0 + o] = acc[o][q];
  }
  __syncthreads();

  const int col = t & 31, rg = t >> 5;                        // 32 columns x 8 row pairs
  double m0[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, m1[5] = {0.0, 0.0, 0.0, 0.0, 0.0};      // vertical pass: outputs (2 rg, col) and (2 rg + 1, col)
#pragma unroll
  for (int j = 0; j < WIN + 1; j++) {
#pragma unroll
    for (int q = 0; q < 5; q++) {
      const double v = hb[q][2 * rg + j][col];
      if (j < WIN) m0[q] += p.g[j] * v;
      if (j > 0) m1[q] += p.g[j - 1] * v;
    }
  }
  const int ox = x0 + col, oy = y0 + 2 * rg;
  double s = 0.0;
  if (ox < w - (WIN - 1)) {
    const double v0 = ssim_value(m0[0], m0[1], m0[2], m0[3], m0[4], p.c1, p.c2);
    const double v1 = ssim_value(m1[0], m1[1], m1[2], m1[3], m1[4], p.c1, p.c2);
    if (oy < h - (WIN - 1)) s = v0;
    if (oy + 1 < h - (WIN - 1)) s += v1;
  }
  s = block_sum_f64(s, wsum);
  if (t == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void finalize_kernel(const double* __restrict__ partial, size_t per_image, double count, double* __restrict__ out) {
  __shared__ double wsum[4];
  const double s = sum_partials_f64(partial + (size_t)blockIdx.x * per_image, per_image, wsum);
  if (threadIdx.x == 0) out[blockIdx.x] = s / count;
}

}  // namespace dmvae_ssim_impl

extern "C" size_t dmvae_ssim_workspace(size_t batch, int channels, int h, int w) {
  using namespace dmvae_ssim_impl;
  if (channels < 1 || h < WIN || w < WIN) return 0;
  return batch * (size_t)channels * tiles_of(h, w) * sizeof(double);
}

extern "C" int dmvae_ssim(const void* a, const void* b, int is_bf16, size_t batch, int channels, int h, int w, int from_pm1, double data_range, void* workspace,
                          void* out, hipStream_t stream) {
  using namespace dmvae_ssim_impl;
  DMVAE_CHECK_ARG(a && b && workspace && out, "ssim: NULL pointer");
  DMVAE_CHECK_ARG(h >= WIN && w >= WIN, "ssim: h >= 11 and w >= 11 required (the 11 x 11 window has no output below that), got h %d w %d", h, w);
  DMVAE_CHECK_ARG(channels >= 1, "ssim: channels >= 1 required, got %d", channels);
  DMVAE_CHECK_ARG(batch >= 1, "ssim: batch >= 1 required");
  DMVAE_CHECK_ARG(__builtin_isfinite(data_range) && data_range > 0.0, "ssim: data_range must be finite and positive, got %g", data_range);
  const size_t tiles = tiles_of(h, w);
  DMVAE_CHECK_ARG(batch <= 0x7fffffffull / tiles / (size_t)channels, "ssim: batch %zu x channels %d x %zu tiles exceed the grid's 2^31 - 1 blocks", batch, channels,
                  tiles);
  Params p;
  double sum = 0.0;
  for (int i = 0; i < WIN; i++) {
    const double d = (double)(i - WIN / 2) / 1.5;
    p.g[i] = exp(-(d * d) / 2.0);
    sum += p.g[i];
  }
  for (int i = 0; i < WIN; i++) p.g[i] /= sum;
  p.c1 = (0.01 * data_range) * (0.01 * data_range);
  p.c2 = (0.03 * data_range) * (0.03 * data_range);
  const int tiles_x = (w - (WIN - 1) + TW - 1) / TW;
  const dim3 grid((unsigned)(batch * (size_t)channels * tiles)), block(256);
  double* ws = (double*)workspace;
  if (is_bf16) hipLaunchKernelGGL(tile_kernel<bf16>, grid, block, 0, stream, (const bf16*)a, (const bf16*)b, h, w, tiles_x, (unsigned)tiles, from_pm1, p, ws);
  else hipLaunchKernelGGL(tile_kernel<float>, grid, block, 0, stream, (const float*)a, (const float*)b, h, w, tiles_x, (unsigned)tiles, from_pm1, p, ws);
  DMVAE_CHECK_LAUNCH();
  const double count = (double)channels * (double)(h - (WIN - 1)) * (double)(w - (WIN - 1));
  hipLaunchKernelGGL(finalize_kernel, dim3((unsigned)batch), block, 0, stream, (const double*)ws, (size_t)channels * tiles, count, (double*)out);
  DMVAE_CHECK_LAUNCH();
  return 0;
}
