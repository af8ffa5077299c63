// The arithmetic around the Inception network in the evaluation tail of sample_50k.py:174-209 and evaluation/fid.py:8-48 (torch-fidelity's FID / Inception
// Score over the sampled images): the uint8 -> f32 resize to the network's input size, and the Inception Score of its logits.  The network's own kernels are
// csrc/inception.hip (dmvae_amd/fidelity.py takes the network as a module).  torch-fidelity is on none of the machines this was developed on: the two definitions below
// restate its published `interpolate_bilinear_2d_like_tensorflow1x` (align_corners=False) and `isc_features_to_metric`, tests/fidelity_spec.py restates them in
// numpy, and agreement with the library itself has not been run.
//
// dmvae_resize_tf1_bilinear: one thread per output element, outputs flat on grid.x (2^31 - 1 blocks of 256).  The TF1 rule has no half-pixel offset: source
// coordinate o * (in / out), the scale being the double quotient rounded to f32 (what `arange(f32) * (in / out)` multiplies by); floor, the next sample clamped
// to the edge, x first, then y, then (v - 128) / 128.  Every operation is f32, rounded once, no FMA contraction: the output equals the index-select form bit
// for bit.  The grid limit keeps s < 2^20, where fl(o * fl(in / s)) < in for every o < s (the product is below in (1 - 2^-20)(1 + 2^-23)): the first tap is
// inside the image by arithmetic; it is clamped all the same, so that no input could make the kernel read outside it.
//
// dmvae_inception_score: three launches, everything f64 after the exact widening of each logit, no atomics, every sum in an order that (n, classes, splits)
// fix.  Position j of the ordered sequence reads row r(j) = order[j] (j itself without a table) and owns slot j of the workspace, so a table and physically
// reordered rows give the same bits.
//   row_kernel       one wave per position: m = max_c x, lse = m + log sum_c exp(x - m), e = sum_c p log p with p = exp(x - lse) (a term with p == 0 adds 0).
//                    Lane l takes classes l, l + 64, ... in ascending order; the 64 lanes are combined by an xor-shuffle tree.
//   marginal_kernel  one workgroup of 16 waves per (split, 64 classes): wave w sums p over the split's positions j0 + w, j0 + w + 16, ... in ascending order
//                    (a 256-B run of a row per wave and position), the 16 partial sums are added in wave order and divided by n_k.
//   finalize_kernel  one workgroup per split: exp((1 / n_k) sum_j e_j - sum_c q log q), both sums strided over 256 threads in ascending order and combined by
//                    the fixed tree of block_sum_f64 (common.h).  Algebraically the mean over j of sum_c p (log p - log q), the reference's per-row KL form.
// Nothing past row n or past column `classes` of a row is read: a lane past the last class reads nothing (row_kernel) or the last class (marginal_kernel,
// dropped).  The table's entries are NOT checked here (dmvae_amd/ops.py checks them on the device before the launch).
#include <math.h>

#include "common.h"
#include "dmvae_hip.h"

namespace dmvae_fidelity {

constexpr int RW = 16;                    // waves of a marginal_kernel workgroup: positions of a split are dealt to them round-robin
constexpr int CAP = 1 << 16;              // workgroups of the two grid-stride kernels

template <typename T>
__device__ __forceinline__ double widen(T v) { return (double)v; }
template <>
__device__ __forceinline__ double widen<bf16>(bf16 v) { return (double)(float)v; }

__device__ __forceinline__ float tap(const uint8_t* __restrict__ img, size_t plane_base, size_t y, size_t x, size_t sy, size_t sx) {
  return (float)img[plane_base + y * sy + x * sx];
}

__global__ __launch_bounds__(256) void resize_kernel(const uint8_t* __restrict__ img, float* __restrict__ out, size_t total, int c, int h, int w, int s, int nhwc,
                                                     float scale_y, float scale_x) {
#pragma clang fp contract(off)
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= total) return;
  const int ox = (int)(p % (size_t)s), oy = (int)((p / (size_t)s) % (size_t)s);
  const size_t plane = p / ((size_t)s * (size_t)s);
  const size_t b = plane / (size_t)c, ch = plane % (size_t)c;
  // element (y, x) of this plane is img[base + y * sy + x * sx]
  const size_t base = nhwc ? b * (size_t)h * (size_t)w * (size_t)c + ch : plane * (size_t)h * (size_t)w;
  const size_t sy = nhwc ? (size_t)w * (size_t)c : (size_t)w, sx = nhwc ? (size_t)c : 1;
  const float gy = (float)oy * scale_y, gx = (float)ox * scale_x;
  int y0 = (int)gy, x0 = (int)gx;
  y0 = y0 > h - 1 ? h - 1 : y0;           // never taken below s = 2^20 (header comment)
  x0 = x0 > w - 1 ? w - 1 : x0;
  const int y1 = y0 + 1 > h - 1 ? h - 1 : y0 + 1, x1 = x0 + 1 > w - 1 ? w - 1 : x0 + 1;
  const float dy = gy - (float)y0, dx = gx - (float)x0;
  const float a = tap(img, base, y0, x0, sy, sx), bb = tap(img, base, y0, x1, sy, sx);
  const float cc = tap(img, base, y1, x0, sy, sx), d = tap(img, base, y1, x1, sy, sx);
  const float top = a + (bb - a) * dx;
  const float bot = cc + (d - cc) * dx;
  out[p] = ((top + (bot - top) * dy) - 128.0f) / 128.0f;
}

__host__ __device__ inline size_t split_start(size_t k, size_t n, size_t splits) { return k * n / splits; }      // k <= splits <= n < 2^31: no overflow

template <typename T>
__global__ __launch_bounds__(256) void row_kernel(const T* __restrict__ x, const int64_t* __restrict__ order, size_t n, int classes, size_t ld,
                                                  double* __restrict__ lse, double* __restrict__ ent) {
  const size_t j = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= n) return;                      // whole waves leave: the shuffles below run with all 64 lanes
  const int lane = threadIdx.x & 63;
  const T* __restrict__ row = x + (order ? (size_t)order[j] : j) * ld;
  double m = -INFINITY;
  for (int c = lane; c < classes; c += 64) m = fmax(m, widen(row[c]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
  double s = 0.0;
  for (int c = lane; c < classes; c += 64) s += exp(widen(row[c]) - m);
  const double l = m + log(wave_sum_f64(s));
  double e = 0.0;
  for (int c = lane; c < classes; c += 64) {
    const double lp = widen(row[c]) - l, p = exp(lp);
    e += p == 0.0 ? 0.0 : p * lp;          // p == 0 (a logit more than 745 below the row's lse): the term's limit, not 0 * -inf
  }
  e = wave_sum_f64(e);
  if (lane == 0) {
    lse[j] = l;
    ent[j] = e;
  }
}

template <typename T>
__global__ __launch_bounds__(64 * RW) void marginal_kernel(const T* __restrict__ x, const int64_t* __restrict__ order, size_t n, int classes, size_t ld, size_t splits,
                                                           const double* __restrict__ lse, double* __restrict__ marg) {
  __shared__ double part[RW][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const size_t chunks = ((size_t)classes + 63) / 64, units = splits * chunks;
  for (size_t u = blockIdx.x; u < units; u += gridDim.x) {
    const size_t k = u / chunks;
    const int c = (int)(u % chunks) * 64 + lane;
    const int cr = c < classes ? c : classes - 1;             // a lane past the last class reads the last class; its sum is dropped
    const size_t j0 = split_start(k, n, splits), j1 = split_start(k + 1, n, splits);
    double s = 0.0;
#pragma unroll 4
    for (size_t j = j0 + wv; j < j1; j += RW) {
      const size_t r = order ? (size_t)order[j] : j;
      s += exp(widen(x[r * ld + cr]) - lse[j]);
    }
    part[wv][lane] = s;
    __syncthreads();
    if (wv == 0 && c < classes) {
      double t = part[0][lane];
#pragma unroll
      for (int i = 1; i < RW; i++) t += part[i][lane];
      marg[k * (size_t)classes + c] = t / (double)(j1 - j0);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void finalize_kernel(const double* __restrict__ ent, const double* __restrict__ marg, size_t n, int classes, size_t splits,
                                                       double* __restrict__ scores) {
  __shared__ double wsum[4];
  for (size_t k = blockIdx.x; k < splits; k += gridDim.x) {
    const size_t j0 = split_start(k, n, splits), j1 = split_start(k + 1, n, splits);
    const double a = sum_partials_f64(ent + j0, j1 - j0, wsum);
    double b = 0.0;
    for (int c = threadIdx.x; c < classes; c += 256) {
      const double q = marg[k * (size_t)classes + c];
      b += q == 0.0 ? 0.0 : q * log(q);
    }
    __syncthreads();                       // block_sum_f64's rule: wsum is written again, every thread has read a's four wave sums
    b = block_sum_f64(b, wsum);
    __syncthreads();                       // the same, for the next split's first sum
    if (threadIdx.x == 0) scores[k] = exp(a / (double)(j1 - j0) - b);
  }
}

inline bool is_args_ok(size_t n, int classes, size_t splits) {
  return classes >= 2 && classes <= 65536 && n <= 0x7fffffffull && splits >= 1 && splits <= n;
}

}  // namespace dmvae_fidelity

extern "C" int dmvae_resize_tf1_bilinear(const uint8_t* img, size_t batch, int channels, int h, int w, int nhwc, int s, float* out, hipStream_t stream) {
  using namespace dmvae_fidelity;
  DMVAE_CHECK_ARG(img && out, "resize_tf1_bilinear: NULL pointer");
  DMVAE_CHECK_ARG(batch >= 1 && channels >= 1, "resize_tf1_bilinear: batch >= 1 and channels >= 1 required, got channels %d", channels);
  DMVAE_CHECK_ARG(h >= 1 && w >= 1, "resize_tf1_bilinear: h >= 1 and w >= 1 required, got h %d w %d", h, w);
  DMVAE_CHECK_ARG(s >= 1, "resize_tf1_bilinear: s >= 1 required, got %d", s);
  const size_t per_image = (size_t)channels * (size_t)s * (size_t)s;                  // may wrap: used only once s * s <= limit / channels has held
  DMVAE_CHECK_ARG((size_t)s * (size_t)s <= (0x7fffffffull * 256) / (size_t)channels && batch <= (0x7fffffffull * 256) / per_image,
                  "resize_tf1_bilinear: batch %zu x channels %d x %d x %d outputs exceed the grid's 2^31 - 1 blocks of 256", batch, channels, s, s);
  const size_t total = batch * per_image;
  const float scale_y = (float)((double)h / (double)s), scale_x = (float)((double)w / (double)s);
  hipLaunchKernelGGL(resize_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, img, out, total, channels, h, w, s, nhwc, scale_y, scale_x);
  DMVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t dmvae_inception_score_workspace(size_t n, int classes, size_t splits) {
  using namespace dmvae_fidelity;
  if (!is_args_ok(n, classes, splits)) return 0;
  return (2 * n + splits * (size_t)classes) * sizeof(double);
}

extern "C" int dmvae_inception_score(const void* logits, int dtype, size_t n, int classes, size_t ld, const int64_t* order, size_t splits, void* workspace,
                                     double* scores, hipStream_t stream) {
  using namespace dmvae_fidelity;
  DMVAE_CHECK_ARG(logits && workspace && scores, "inception_score: NULL pointer");
  DMVAE_CHECK_ARG(dtype >= 0 && dtype <= 2, "inception_score: dtype must be 0 (f32), 1 (bf16) or 2 (f64), got %d", dtype);
  DMVAE_CHECK_ARG(classes >= 2 && classes <= 65536, "inception_score: classes must lie in [2, 65536], got %d", classes);
  DMVAE_CHECK_ARG(n >= 1 && n <= 0x7fffffffull, "inception_score: n must lie in [1, 2^31 - 1], got %zu", n);
  DMVAE_CHECK_ARG(splits >= 1 && splits <= n, "inception_score: splits must lie in [1, n = %zu], got %zu", n, splits);
  DMVAE_CHECK_ARG(ld >= (size_t)classes, "inception_score: leading dimension %zu < classes %d", ld, classes);
  double* lse = (double*)workspace;
  double* ent = lse + n;
  double* marg = ent + n;
  const dim3 rows((unsigned)((n + 3) / 4));
  const int mgrid = grid_for(splits * (((size_t)classes + 63) / 64), 1, CAP), fgrid = grid_for(splits, 1, CAP);
#define DMVAE_IS_LAUNCH(T)                                                                                                                               \
  do {                                                                                                                                                   \
    hipLaunchKernelGGL(row_kernel<T>, rows, dim3(256), 0, stream, (const T*)logits, order, n, classes, ld, lse, ent);                                    \
    DMVAE_CHECK_LAUNCH();                                                                                                                                \
    hipLaunchKernelGGL(marginal_kernel<T>, dim3(mgrid), dim3(64 * RW), 0, stream, (const T*)logits, order, n, classes, ld, splits, (const double*)lse, marg); \
    DMVAE_CHECK_LAUNCH();                                                                                                                                \
  } while (0)
  if (dtype == 0) DMVAE_IS_LAUNCH(float);
  else if (dtype == 1) DMVAE_IS_LAUNCH(bf16);
  else DMVAE_IS_LAUNCH(double);
#undef DMVAE_IS_LAUNCH
  hipLaunchKernelGGL(finalize_kernel, dim3(fgrid), dim3(256), 0, stream, (const double*)ent, (const double*)marg, n, classes, splits, scores);
  DMVAE_CHECK_LAUNCH();
  return 0;
}
