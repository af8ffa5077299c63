// The two kernels the evaluation LPIPS (evaluation/metrics.py:26-29: torchmetrics' LearnedPerceptualImagePatchSimilarity, net_type 'alex') needs beside the
// exact-f32 convolution and the 3 x 3 pool of csrc/inception.hip: the input pass and the head.  The library cannot be run where this package is developed;
// both kernels restate its published definition (dmvae_amd/models/lpips_alex.py, tests/lpips_eval_spec.py).
//
// dmvae_lpips_input: one thread per output element of y [2 B][H][W][3] (NHWC f32): rows 0 .. B are x1, rows B .. 2 B are x2, both [B][3][H][W] (NCHW, f32 or
// bf16 widened exactly), y = (x - shift[ch]) / scale[ch]: the library's ScalingLayer, one f32 subtraction and one IEEE f32 division, nothing contracted.  Both
// LPIPS branches then run through the trunk as ONE batch of 2 B images.
//
// dmvae_lpips_head: per pair i (image i against image pairs + i of f [2 pairs][h][w][c], NHWC f32) the level's value
//   d = mean_{pixels} sum_c lin[c] (n1[c] - n2[c])^2,   n = f * (1 / sqrt(eps + sum_c f[c]^2))
// with every element widened to f64 on load and everything after that in f64.  A bandwidth-bound reduction: every byte of f is read once, nothing normalised
// is written.  The plan is a function of (h, w, c) alone (plan_for): a group of L = min(64, pow2ceil(c / 4)) lanes owns one pixel, lane g of it the channel
// quads g, g + L, ... (R = ceil(c / 4 / L) <= 4 float4 per side, kept in registers between the two channel sums); a workgroup of 256 threads owns
// 256 / L pixels per iteration and `iters` iterations, about 32 KB of f per workgroup.  Orders: a lane adds its own channels ascending, the L lanes of a group
// an xor-shuffle tree (every lane ends with the same bits), a group its pixels in iteration order, the groups of a workgroup block_sum_f64's tree (common.h); the workgroup's
// sum goes to partial[pair * nb + block] and finalize_kernel -- one workgroup per pair -- adds the nb partials in a fixed order, divides by h w and stores or
// (accumulate) adds to out[pair].  No atomics: an image pair's value depends on its own features and the shape alone, the same bits alone, at any position
// of any batch, and on every run.  dmvae_lpips_head_form is the same kernel with the normalisation selected: form 0 the one above (the same bits as
// dmvae_lpips_head), form 1 n = f * (1 / (sqrt(sum_c f[c]^2) + eps)), the reference's own normalize_tensor (utils/lpips.py:156-158; the evaluation twin of
// the training loss, dmvae_amd/models/lpips_eval.py).  The difference is formed as n1 - n2 and then squared with contraction off: swapping the halves changes no bit, and
// identical halves give exactly 0.0.  eps > 0 is required, so a pixel whose channels are all zero on both sides gives n = 0 / sqrt(eps) = 0 and adds 0.
//   A pixel past h w is never loaded and adds nothing; a channel quad past c / 4 (c / 4 no multiple of L) likewise.  Nothing outside f's 2 pairs h w c
// elements and lin's c elements is read; partial[pairs * nb] and out[pairs] are all that is written.
#include <math.h>

#include "common.h"
#include "dmvae_hip.h"

namespace dmvae_lpips_eval {

constexpr int MAXR = 4;                          // float4 per lane and side: c <= 4 * 64 * MAXR
constexpr int C_MAX = 4 * 64 * MAXR;             // 1024
constexpr size_t BLOCK_BYTES = 32768;            // of f per workgroup, about
constexpr size_t GRID_MAX = 0x7fffffffull;

struct Plan {
  int L, R, gpb, iters;                          // lanes per pixel, float4 per lane, pixel groups per workgroup, iterations per workgroup
  size_t hw, nb;                                 // pixels per image, workgroups (= partials) per pair
};

inline bool plan_for(int h, int w, int c, Plan* p) {
  if (h < 1 || w < 1 || h > 32768 || w > 32768 || c < 4 || c % 4 || c > C_MAX) return false;
  const int q = c / 4;
  int L = 1;
  while (L < q && L < 64) L <<= 1;
  p->L = L, p->R = (q + L - 1) / L, p->gpb = 256 / L;
  const size_t want = BLOCK_BYTES / (8 * (size_t)c);      // pixels of both sides in BLOCK_BYTES
  p->iters = (int)(want / (size_t)p->gpb);
  if (p->iters < 1) p->iters = 1;
  p->hw = (size_t)h * (size_t)w;
  const size_t ppb = (size_t)p->gpb * (size_t)p->iters;
  p->nb = (p->hw + ppb - 1) / ppb;
  return true;
}

// FORM 0: r = 1 / sqrt(eps + s) (torchmetrics' normalisation); FORM 1: r = 1 / (sqrt(s) + eps) (the reference's own normalize_tensor, utils/lpips.py:156-158).
// The one changed operation; every load, order and sum is shared.
template <int R, int FORM>
__global__ __launch_bounds__(256) void head_kernel(const float* __restrict__ f, const float* __restrict__ lin, size_t pairs, size_t hw, int c, int L, int iters,
                                                   unsigned nb, double eps, double* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ double wsum[4];
  const int t = threadIdx.x, gl = t & (L - 1), g = t / L, gpb = 256 / L, q = c >> 2;
  const size_t pair = blockIdx.x / nb;
  const unsigned blk = blockIdx.x % nb;
  const float* __restrict__ f1 = f + pair * hw * (size_t)c;
  const float* __restrict__ f2 = f + (pairs + pair) * hw * (size_t)c;

  bool live[R];
  double wl[R][4];
#pragma unroll
  for (int j = 0; j < R; j++) {
    const int idx = j * L + gl;
    live[j] = idx < q;
    const float4 v = live[j] ? *reinterpret_cast<const float4*>(lin + 4 * idx) : make_float4(0.f, 0.f, 0.f, 0.f);
    wl[j][0] = (double)v.x, wl[j][1] = (double)v.y, wl[j][2] = (double)v.z, wl[j][3] = (double)v.w;
  }

  double acc = 0.0;
  for (int it = 0; it < iters; it++) {
    const size_t p = ((size_t)blk * (size_t)iters + (size_t)it) * (size_t)gpb + (size_t)g;
    const bool ok = p < hw;
    float4 a[R], b[R];
#pragma unroll
    for (int j = 0; j < R; j++) {
      a[j] = b[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (ok && live[j]) {
        const size_t o = p * (size_t)c + 4 * (size_t)(j * L + gl);
        a[j] = *reinterpret_cast<const float4*>(f1 + o);
        b[j] = *reinterpret_cast<const float4*>(f2 + o);
      }
    }
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int j = 0; j < R; j++) {
      const double x[4] = {(double)a[j].x, (double)a[j].y, (double)a[j].z, (double)a[j].w};
      const double y[4] = {(double)b[j].x, (double)b[j].y, (double)b[j].z, (double)b[j].w};
#pragma unroll
      for (int e = 0; e < 4; e++) {
        s1 += x[e] * x[e];                                             // the square of an f32 is exact in f64
        s2 += y[e] * y[e];
      }
    }
    for (int o = L >> 1; o > 0; o >>= 1) {
      s1 += __shfl_xor(s1, o, 64);
      s2 += __shfl_xor(s2, o, 64);
    }
    const double r1 = FORM == 0 ? 1.0 / sqrt(eps + s1) : 1.0 / (sqrt(s1) + eps), r2 = FORM == 0 ? 1.0 / sqrt(eps + s2) : 1.0 / (sqrt(s2) + eps);
    double v = 0.0;
#pragma unroll
    for (int j = 0; j < R; j++) {
      const double x[4] = {(double)a[j].x, (double)a[j].y, (double)a[j].z, (double)a[j].w};
      const double y[4] = {(double)b[j].x, (double)b[j].y, (double)b[j].z, (double)b[j].w};
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const double d = x[e] * r1 - y[e] * r2;
        const double dd = d * d;
        v += wl[j][e] * dd;
      }
    }
    for (int o = L >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (ok) acc += v;
  }
  const double s = block_sum_f64(gl == 0 ? acc : 0.0, wsum);
  if (t == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void finalize_kernel(const double* __restrict__ partial, size_t nb, double count, int accumulate, double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double wsum[4];
  const double s = sum_partials_f64(partial + (size_t)blockIdx.x * nb, nb, wsum);
  if (threadIdx.x == 0) {
    const double v = s / count;
    out[blockIdx.x] = accumulate ? out[blockIdx.x] + v : v;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void input_kernel(const T* __restrict__ x1, const T* __restrict__ x2, float* __restrict__ y, size_t total, size_t hw, size_t batch) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const size_t ch = i % 3, pix = i / 3, b = pix / hw, p = pix - b * hw;
  const T* __restrict__ src = b < batch ? x1 : x2;
  const float v = (float)src[((b < batch ? b : b - batch) * 3 + ch) * hw + p];
  const float shift = ch == 0 ? -.030f : ch == 1 ? -.088f : -.188f;
  const float scale = ch == 0 ? .458f : ch == 1 ? .448f : .450f;
  y[i] = __fdiv_rn(__fsub_rn(v, shift), scale);
}

}  // namespace dmvae_lpips_eval

extern "C" int dmvae_lpips_input(const void* x1, const void* x2, int is_bf16, float* y, int batch, int h, int w, hipStream_t stream) {
  using namespace dmvae_lpips_eval;
  DMVAE_CHECK_ARG(x1 && x2 && y, "lpips_input: NULL pointer");
  DMVAE_CHECK_ARG(batch >= 1 && h >= 1 && w >= 1 && h <= 32768 && w <= 32768, "lpips_input: batch >= 1 and 1 <= h, w <= 32768 required, got %d x %d x %d", batch,
                  h, w);
  const size_t hw = (size_t)h * w, total = 2 * (size_t)batch * hw * 3;
  DMVAE_CHECK_ARG((total + 255) / 256 <= GRID_MAX, "lpips_input: %zu outputs exceed the grid's 2^31 - 1 blocks of 256", total);
  const dim3 grid((unsigned)((total + 255) / 256));
  if (is_bf16) hipLaunchKernelGGL(input_kernel<bf16>, grid, dim3(256), 0, stream, (const bf16*)x1, (const bf16*)x2, y, total, hw, (size_t)batch);
  else hipLaunchKernelGGL(input_kernel<float>, grid, dim3(256), 0, stream, (const float*)x1, (const float*)x2, y, total, hw, (size_t)batch);
  DMVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t dmvae_lpips_head_workspace(size_t pairs, int h, int w, int c) {
  using namespace dmvae_lpips_eval;
  Plan p;
  if (pairs < 1 || !plan_for(h, w, c, &p) || pairs > GRID_MAX / p.nb) return 0;
  return pairs * p.nb * sizeof(double);
}

namespace dmvae_lpips_eval {

// dmvae_lpips_head (form 0, named "lpips_head") and dmvae_lpips_head_form: one validation, one plan, one launch sequence.
static int head_launch(const char* name, const float* f, const float* lin, size_t pairs, int h, int w, int c, double eps, int form, int accumulate,
                       void* workspace, double* out, hipStream_t stream) {
  DMVAE_CHECK_ARG(f && lin && workspace && out, "%s: NULL pointer", name);
  DMVAE_CHECK_ARG(form == 0 || form == 1, "%s: form must be 0 (f / sqrt(eps + sum f^2)) or 1 (f / (sqrt(sum f^2) + eps)), got %d", name, form);
  DMVAE_CHECK_ARG(pairs >= 1 && h >= 1 && w >= 1 && h <= 32768 && w <= 32768, "%s: pairs >= 1 and 1 <= h, w <= 32768 required, got %zu x %d x %d", name, pairs,
                  h, w);
  DMVAE_CHECK_ARG(c >= 4 && c % 4 == 0 && c <= C_MAX, "%s: c must be a multiple of 4 in [4, %d], got %d", name, C_MAX, c);
  DMVAE_CHECK_ARG(__builtin_isfinite(eps) && eps > 0.0, "%s: eps must be finite and positive (an all-zero pixel is 0 / sqrt(eps)), got %g", name, eps);
  Plan p;
  DMVAE_CHECK_ARG(plan_for(h, w, c, &p), "%s: no plan for %d x %d x %d", name, h, w, c);
  DMVAE_CHECK_ARG(pairs <= GRID_MAX / p.nb, "%s: %zu pairs x %zu workgroups exceed the grid's 2^31 - 1 blocks", name, pairs, p.nb);
  const dim3 grid((unsigned)(pairs * p.nb)), block(256);
  double* ws = (double*)workspace;
#define DMVAE_LPIPS_HEAD(R_, F_) \
  hipLaunchKernelGGL((head_kernel<R_, F_>), grid, block, 0, stream, f, lin, pairs, p.hw, c, p.L, p.iters, (unsigned)p.nb, eps, ws)
#define DMVAE_LPIPS_HEAD_R(F_) \
  switch (p.R) {               \
    case 1: DMVAE_LPIPS_HEAD(1, F_); break; \
    case 2: DMVAE_LPIPS_HEAD(2, F_); break; \
    case 3: DMVAE_LPIPS_HEAD(3, F_); break; \
    default: DMVAE_LPIPS_HEAD(4, F_); break; \
  }
  if (form == 0) { DMVAE_LPIPS_HEAD_R(0) } else { DMVAE_LPIPS_HEAD_R(1) }
#undef DMVAE_LPIPS_HEAD_R
#undef DMVAE_LPIPS_HEAD
  DMVAE_CHECK_LAUNCH();
  hipLaunchKernelGGL(finalize_kernel, dim3((unsigned)pairs), block, 0, stream, (const double*)ws, p.nb, (double)p.hw, accumulate != 0, out);
  DMVAE_CHECK_LAUNCH();
  return 0;
}

}  // namespace dmvae_lpips_eval

extern "C" int dmvae_lpips_head(const float* f, const float* lin, size_t pairs, int h, int w, int c, double eps, int accumulate, void* workspace, double* out,
                                hipStream_t stream) {
  return dmvae_lpips_eval::head_launch("lpips_head", f, lin, pairs, h, w, c, eps, 0, accumulate, workspace, out, stream);
}

extern "C" int dmvae_lpips_head_form(const float* f, const float* lin, size_t pairs, int h, int w, int c, double eps, int form, int accumulate, void* workspace,
                                     double* out, hipStream_t stream) {
  return dmvae_lpips_eval::head_launch("lpips_head_form", f, lin, pairs, h, w, c, eps, form, accumulate, workspace, out, stream);
}
