// The input pipeline of utils/build_dataset.py:55-66 on the device: RandomHorizontalFlip, Resize(mid, LANCZOS), RandomCrop / CenterCrop, ToTensor and
// x + x - 1 in one pass over a ragged pack of decoded uint8 HWC images, held to PIL's bytes.
//
// PIL's 8-bit resampler (libImaging/Resample.c) is integer arithmetic on tables derived in double: per output index a first source index, a tap count and
// 22-bit fixed-point coefficients; each pass is clamp((2^21 + sum_j k_j * pixel_j) >> 22, 0, 255) in int32, horizontal first, and the horizontal result is
// rounded to uint8 before the vertical pass reads it.  dmvae_lanczos_table builds those tables on the HOST, with libm's sin (what PIL calls: another sin may
// differ in the last ulp, and the last ulp can move a 22-bit coefficient), only for the output indices the crop window touches.
//
// image_preprocess_kernel: one workgroup per (image, band of ROWS output rows, 256 output columns); a thread owns one output column x 3 channels and keeps
// the band's vertical sums in int32 registers.  The workgroup walks the band's source rows once, SRC rows at a time (the x coefficients are loaded once per
// SRC rows): per source row a thread forms its horizontal value, rounds it to uint8 in a register and adds ky * h into those of its row accumulators whose
// tap range holds that source row (the range test is uniform over the workgroup: a scalar branch).  No intermediate image goes to HBM; tap counts are loop
// bounds read from the table, nothing is unrolled to a fixed count.  The source is read as bytes at (row * W + col) * 3 + c with row < H and col < W: never
// past an image's last byte, whatever the pack holds there.  A flip mirrors the SOURCE column (torchvision flips before it resizes; the truncated tables
// are not mirror-symmetric by construction).  A pass whose in == out is skipped as PIL skips it: its table offset is -1 and the pixel is taken as it is.
#include <errno.h>
#include <math.h>

#include "common.h"
#include "dmvae_hip.h"

namespace dmvae_data {

constexpr int PRECISION_BITS = 32 - 8 - 2;      // Resample.c: 22
constexpr int ROWS = 16;                         // output rows per workgroup
constexpr int SRC = 4;                           // source rows per load of the x coefficients
constexpr int REC = DMVAE_IMAGE_RECORD_WORDS;

// Resample.c: sinc_filter / lanczos_filter, operation for operation
static inline double sinc_filter(double x) {
  if (x == 0.0) return 1.0;
  x = x * M_PI;
  return sin(x) / x;
}
static inline double lanczos_filter(double x) {
  if (-3.0 <= x && x < 3.0) return sinc_filter(x) * sinc_filter(x / 3);
  return 0.0;
}

static inline int kmax_for(int in, int out) {
  double filterscale = (double)in / out;
  if (filterscale < 1.0) filterscale = 1.0;
  return (int)ceil(3.0 * filterscale) * 2 + 1;    // Resample.c: ksize
}

__device__ __forceinline__ int clip8(int v) {
  v >>= PRECISION_BITS;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

template <bool F32>
__global__ __launch_bounds__(256) void image_preprocess_kernel(const uint8_t* __restrict__ pack, const int64_t* __restrict__ table,
                                                               const int32_t* __restrict__ taps, int S, void* __restrict__ outv) {
  const int64_t* __restrict__ rec = table + (size_t)blockIdx.z * REC;
  const uint8_t* __restrict__ src = pack + rec[0];
  const int H = (int)rec[1], W = (int)rec[2];
  const int top = (int)rec[5], left = (int)rec[6];
  const bool flip = rec[7] != 0;
  const int64_t xoff = rec[8], yoff = rec[9];
  const int kmx = (int)rec[10], kmy = (int)rec[11];
  const int x = blockIdx.x * blockDim.x + threadIdx.x;  // output column inside the crop
  const int y0 = blockIdx.y * ROWS;                   // first output row of the band
  const bool col_ok = x < S;
  const int xc = col_ok ? x : S - 1;                  // a thread past the last column walks the last column's taps and stores nothing

  // x taps of this thread's column: first source column, count, coefficients (none when the horizontal pass is skipped)
  int xlo, xn;
  const int32_t* __restrict__ kx = nullptr;
  if (xoff >= 0) {
    const int32_t* __restrict__ t = taps + xoff;
    xlo = t[xc];
    xn = t[S + xc];
    kx = t + 2 * (size_t)S + (size_t)xc * kmx;
  } else {
    xlo = left + xc;
    xn = 1;
  }
  // y taps of the band's rows (uniform over the workgroup); a row past S gets an empty range
  int ylo[ROWS], yn[ROWS];
  const int32_t* __restrict__ ty = yoff >= 0 ? taps + yoff : nullptr;
#pragma unroll
  for (int r = 0; r < ROWS; r++) {
    const int y = y0 + r;
    if (y >= S) { ylo[r] = 0; yn[r] = 0; }
    else if (ty) { ylo[r] = ty[y]; yn[r] = ty[S + y]; }
    else { ylo[r] = top + y; yn[r] = 1; }
  }
  const int last = (y0 + ROWS <= S ? ROWS : S - y0) - 1;
  int sy0 = ylo[0], sy1 = ylo[0] + yn[0];
#pragma unroll
  for (int r = 1; r < ROWS; r++)
    if (r <= last) sy1 = ylo[r] + yn[r];               // first index and first index + count never decrease along an axis

  int acc[ROWS][3];
#pragma unroll
  for (int r = 0; r < ROWS; r++) acc[r][0] = acc[r][1] = acc[r][2] = 1 << (PRECISION_BITS - 1);

  for (int sy = sy0; sy < sy1; sy += SRC) {
    // horizontal pass of SRC source rows at this thread's column; a row past the band's last is read as that last row and used by nobody
    const uint8_t* __restrict__ rowp[SRC];
#pragma unroll
    for (int g = 0; g < SRC; g++) {
      const int row = sy + g < sy1 ? sy + g : sy1 - 1;
      rowp[g] = src + (size_t)row * (size_t)W * 3;
    }
    int h[SRC][3];
    if (kx) {
#pragma unroll
      for (int g = 0; g < SRC; g++) h[g][0] = h[g][1] = h[g][2] = 1 << (PRECISION_BITS - 1);
      for (int j = 0; j < xn; j++) {
        const int k = kx[j];
        const int sx = flip ? W - 1 - (xlo + j) : xlo + j;
#pragma unroll
        for (int g = 0; g < SRC; g++) {
          const uint8_t* __restrict__ p = rowp[g] + (size_t)sx * 3;
          h[g][0] += k * (int)p[0];
          h[g][1] += k * (int)p[1];
          h[g][2] += k * (int)p[2];
        }
      }
#pragma unroll
      for (int g = 0; g < SRC; g++) {
        h[g][0] = clip8(h[g][0]);                      // PIL stores the horizontal result as uint8: the vertical pass reads the rounded value
        h[g][1] = clip8(h[g][1]);
        h[g][2] = clip8(h[g][2]);
      }
    } else {
      const int sx = flip ? W - 1 - xlo : xlo;
#pragma unroll
      for (int g = 0; g < SRC; g++) {
        const uint8_t* __restrict__ p = rowp[g] + (size_t)sx * 3;
        h[g][0] = p[0];
        h[g][1] = p[1];
        h[g][2] = p[2];
      }
    }
    // vertical pass: every output row of the band whose tap range holds the source row takes ky * h
#pragma unroll
    for (int g = 0; g < SRC; g++) {
      const int row = sy + g;
#pragma unroll
      for (int r = 0; r < ROWS; r++) {
        const int j = row - ylo[r];
        if (j >= 0 && j < yn[r]) {
          const int k = ty ? ty[2 * (size_t)S + (size_t)(y0 + r) * kmy + j] : 1 << PRECISION_BITS;   // a skipped pass: the value itself after the shift
          acc[r][0] += k * h[g][0];
          acc[r][1] += k * h[g][1];
          acc[r][2] += k * h[g][2];
        }
      }
    }
  }

  if (!col_ok) return;
  const size_t b = blockIdx.z;
#pragma unroll
  for (int r = 0; r < ROWS; r++) {
    const int y = y0 + r;
    if (y >= S) break;
    const int u0 = clip8(acc[r][0]), u1 = clip8(acc[r][1]), u2 = clip8(acc[r][2]);
    if (F32) {
      // ToTensor (a true division by 255), then x + x, then + (-1): transforms.ToTensor and normalize_01_into_pm1, NCHW
      float* __restrict__ o = (float*)outv + ((b * 3) * (size_t)S + y) * (size_t)S + x;
      const size_t plane = (size_t)S * S;
      const float v0 = (float)u0 / 255.0f, v1 = (float)u1 / 255.0f, v2 = (float)u2 / 255.0f;
      o[0] = (v0 + v0) + -1.0f;
      o[plane] = (v1 + v1) + -1.0f;
      o[2 * plane] = (v2 + v2) + -1.0f;
    } else {
      uint8_t* __restrict__ o = (uint8_t*)outv + ((b * (size_t)S + y) * (size_t)S + x) * 3;
      o[0] = (uint8_t)u0;
      o[1] = (uint8_t)u1;
      o[2] = (uint8_t)u2;
    }
  }
}

}  // namespace dmvae_data

extern "C" int dmvae_lanczos_kmax(int in, int out) {
  if (in < 1 || out < 1) { dmvae_set_error("lanczos_kmax: in >= 1 and out >= 1 required, got %d -> %d", in, out); return -EINVAL; }
  return dmvae_data::kmax_for(in, out);
}

#pragma clang fp contract(off)
extern "C" int dmvae_lanczos_table(int in, int out, int first, int count, int kmax, int32_t* lo, int32_t* n, int32_t* k) {
  using namespace dmvae_data;
  DMVAE_CHECK_ARG(lo && n && k, "lanczos_table: NULL pointer");
  DMVAE_CHECK_ARG(in >= 1 && out >= 1, "lanczos_table: in >= 1 and out >= 1 required, got %d -> %d", in, out);
  DMVAE_CHECK_ARG(count >= 1 && first >= 0 && (long long)first + count <= out, "lanczos_table: window [%d, %d + %d) outside [0, %d)", first, first, count, out);
  DMVAE_CHECK_ARG(kmax >= kmax_for(in, out), "lanczos_table: kmax %d < %d needed for %d -> %d", kmax, kmax_for(in, out), in, out);
  // Resample.c: precompute_coeffs + normalize_coeffs_8bpc, for the output indices first .. first + count - 1
  const double scale = (double)in / out;
  double filterscale = scale;
  if (filterscale < 1.0) filterscale = 1.0;
  const double support = 3.0 * filterscale;
  const double ss = 1.0 / filterscale;
  double w[64];
  double* wbuf = kmax <= 64 ? w : new double[kmax];
  for (int i = 0; i < count; i++) {
    const double center = (first + i + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; x++) {
      wbuf[x] = lanczos_filter((x + xmin - center + 0.5) * ss);
      ww += wbuf[x];
    }
    int32_t* ki = k + (size_t)i * kmax;
    for (int x = 0; x < xmax; x++) {
      const double v = ww != 0.0 ? wbuf[x] / ww : wbuf[x];
      ki[x] = v < 0 ? (int)(-0.5 + v * (1 << PRECISION_BITS)) : (int)(0.5 + v * (1 << PRECISION_BITS));
    }
    for (int x = xmax; x < kmax; x++) ki[x] = 0;
    lo[i] = xmin;
    n[i] = xmax;
  }
  if (wbuf != w) delete[] wbuf;
  return 0;
}

extern "C" int dmvae_image_preprocess(const uint8_t* pack, const int64_t* table, const int32_t* taps, int B, int S, void* out, int out_kind,
                                      hipStream_t stream) {
  using namespace dmvae_data;
  DMVAE_CHECK_ARG(pack && table && out, "image_preprocess: NULL pointer");      // taps may be NULL when no image of the batch is resized
  DMVAE_CHECK_ARG(B >= 1 && B <= 65535, "image_preprocess: 1 <= B <= 65535 required, got %d", B);
  DMVAE_CHECK_ARG(S >= 1 && S <= 16384, "image_preprocess: 1 <= S <= 16384 required, got %d", S);
  DMVAE_CHECK_ARG(out_kind == DMVAE_IMAGE_OUT_U8_NHWC || out_kind == DMVAE_IMAGE_OUT_F32_NCHW, "image_preprocess: out_kind must be 0 (U8_NHWC) or 1 (F32_NCHW), got %d",
                  out_kind);
  const int threads = S >= 256 ? 256 : (S + 63) / 64 * 64;
  const dim3 grid((S + threads - 1) / threads, (S + ROWS - 1) / ROWS, B), block(threads);
  if (out_kind == DMVAE_IMAGE_OUT_F32_NCHW) hipLaunchKernelGGL(image_preprocess_kernel<true>, grid, block, 0, stream, pack, table, taps, S, out);
  else hipLaunchKernelGGL(image_preprocess_kernel<false>, grid, block, 0, stream, pack, table, taps, S, out);
  DMVAE_CHECK_LAUNCH();
  return 0;
}
