// The kernels of the FID Inception-v3 feature extractor (dmvae_amd/models/inception.py: torch-fidelity's FeatureExtractorInceptionV3, the network behind
// evaluation/fid.py:8-48 and sample_50k.py:174-209), all on NHWC f32 activations: an exact-f32 implicit-GEMM convolution with the BatchNorm affine and the
// ReLU in its epilogue, the three 3 x 3 pools, the global average and the NCHW -> NHWC input pass.
//
// dmvae_conv2d_f32_fwd: M = B Ho Wo output pixels x N = Cout channels, K = kh kw Cin in the order (ky, kx, ci).  K is cut into chunks of 16 (one tap, 16
// channels; for a first layer's Cin = 3 one chunk is 4 taps x {3 channels, one zero}, which is exact: Inception's 3 x 3 stride 2 is 9 taps in 3 chunks, the
// evaluation LPIPS' AlexNet 11 x 11 stride 4 padding 2 is 121 taps in 31 chunks, the last holding one real tap and three zero ones).  A workgroup of four waves owns a 64 x 64 tile; wave
// v owns pixels 16 v .. 16 v + 15 of it and all 64 channels as four independent 16 x 16 accumulators of v_mfma_f32_16x16x4_f32, the only MFMA opcode of
// this file.  The weights are the MFMA's A operand (row = channel) and the activations its B operand (column = pixel): a lane then holds four CONSECUTIVE
// channels of one pixel, and the epilogue is one 16-B store per accumulator into the (wider) NHWC output.
//   One stage is four chunks: thread t loads the 64 B of pixel t & 63, chunk t >> 6 (four 16-B loads, zeros outside the image or past M) and a 16-B piece
// of each of the stage's four weight chunks, keeps them in registers while the previous stage is multiplied, and writes them to LDS between two barriers.
// An LDS row is the 16 k of one pixel (or channel) in the order lane group q = l >> 4 reads them: 16-B slot q holds k = q, q + 4, q + 8, q + 12, so that one
// ds_read_b128 per operand feeds the four MFMAs of a chunk and MFMA s multiplies k = 4 s .. 4 s + 3 in ascending order.  The activations are transposed
// into that order in registers; the weight operand is stored that way once, when the module packs it ([chunk][Cout][16], the checkpoint's bits).  The slot
// is XOR-ed with swz64(row) (common.h) against the bank conflicts of 64-B rows.
//   Each output is ONE chain acc = fma(w_k, x_k, acc) over k ascending from acc = 0 (the MFMA is that chain bit for bit), then y = fma(acc, scale, shift)
// and the optional max(y, 0).  No split-K, no atomics, and the tile an output falls into changes nothing about its chain: the value of a pixel depends on
// its own receptive field and the weights only -- not on the batch size, its position in the batch, or the grid -- and repeats bit for bit.
//   Nothing outside x's B H W Cin elements is read (every tap is range-checked, every row against M, every weight row against Cout); stores are made only
// for pixel < M and channel < Cout, at y[pixel * out_c_pitch + out_c_offset + channel].
//
// dmvae_pool2d_f32: one thread per (output pixel, 4 channels), taps in (ky, kx) raster order, taps outside the image skipped (a maximum never sees the
// padding; the average divides by the number of taps inside, count_include_pad=False).  dmvae_global_avgpool_f32: one thread per (image, channel), the
// H W values added in ascending order in f64, divided in f64, rounded once.  dmvae_inception_input: one thread per output element.
//
// dmvae_maxpool2d_f32: the stride-2 maximum pools without padding of the evaluation LPIPS' VGG16 (2 x 2) and SqueezeNet 1.1 (3 x 3, ceil_mode) trunks
// (dmvae_amd/models/lpips_eval.py), laid out as dmvae_pool2d_f32: one thread per (output pixel, 4 channels), float4 loads, every tap range-checked.  Those
// trunks' convolutions are forms the conv kernel already has: for Cin = 3 the loader walks (3, 3) padding 1 (VGG's first layer) tap by tap as it does
// (3, 3) stride 2, and a Fire module's two expands write their channel slices of one buffer through out_c_offset.
#include <math.h>

#include "common.h"
#include "dmvae_hip.h"

namespace dmvae_inception {

constexpr int BM = 64, BN = 64, KC = 16, CPS = 4;      // tile rows (pixels), tile columns (channels), k per chunk, chunks per stage

struct ConvArgs {
  const float* x;
  const float* w;
  const float* scale;
  const float* shift;
  float* y;
  size_t M;
  int H, W, Cin, Cout, kw, stride, ph, pw, Ho, Wo, relu, c_off, c_pitch, chunks, cpt;      // cpt: chunks per tap (Cin / 16; unused for Cin = 3)
};

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// the 16-B slot of lane group q in row `row` of a [rows][16] f32 LDS tile
__device__ __forceinline__ float4* slot(float* tile, int row, int q) { return reinterpret_cast<float4*>(tile + row * KC + ((q ^ swz64(row)) << 2)); }

template <bool CIN3>
__global__ __launch_bounds__(256, 2) void conv_kernel(const ConvArgs a) {
  __shared__ __attribute__((aligned(16))) float lds_x[CPS][BM * KC];
  __shared__ __attribute__((aligned(16))) float lds_w[CPS][BN * KC];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const size_t m0 = (size_t)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const int nsub = min(4, (a.Cout - n0) >> 4);                      // 16-channel accumulators of this tile that exist
  const int nstages = (a.chunks + CPS - 1) / CPS;

  // loader roles: activations -- pixel lrow, chunk lch of the stage; weights -- channel wrow, 16-B piece wpart of each of the stage's chunks
  const int lrow = t & 63, lch = t >> 6, wrow = t >> 2, wpart = t & 3;
  const size_t m = m0 + lrow;
  const bool mvalid = m < a.M;
  int iy0 = 0, ix0 = 0;
  const float* xb = a.x;
  if (mvalid) {
    const size_t per = (size_t)a.Ho * a.Wo, b = m / per, r = m - b * per;
    const int oy = (int)(r / a.Wo), ox = (int)(r - (size_t)oy * a.Wo);
    iy0 = oy * a.stride - a.ph;
    ix0 = ox * a.stride - a.pw;
    xb = a.x + b * (size_t)a.H * a.W * a.Cin;
  }
  const bool wvalid = n0 + wrow < a.Cout;
  const float* wb = a.w + ((size_t)(n0 + wrow)) * KC + wpart * 4;   // + chunk * Cout * 16

  float4 rx[4], rw[4];
  auto load_stage = [&](int st) {
    const int c = st * CPS + lch;
#pragma unroll
    for (int j = 0; j < 4; j++) rx[j] = zero4();
    if (mvalid && c < a.chunks) {
      if constexpr (CIN3) {
#pragma unroll
        for (int j = 0; j < 4; j++) {                               // k = 4 j + e: tap 4 c + j, channel e (e = 3: zero)
          const int tap = 4 * c + j, ky = tap / a.kw, kx = tap - ky * a.kw, iy = iy0 + ky, ix = ix0 + kx;
          if (tap < a.cpt && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {      // cpt holds the tap count here
            const float* p = xb + ((size_t)iy * a.W + ix) * 3;
            rx[j] = make_float4(p[0], p[1], p[2], 0.f);
          }
        }
      } else {
        const int tap = c / a.cpt, ci0 = (c - tap * a.cpt) * KC, ky = tap / a.kw, kx = tap - ky * a.kw, iy = iy0 + ky, ix = ix0 + kx;
        if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
          const float4* p = reinterpret_cast<const float4*>(xb + ((size_t)iy * a.W + ix) * a.Cin + ci0);
#pragma unroll
          for (int j = 0; j < 4; j++) rx[j] = p[j];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int cw = st * CPS + j;
      rw[j] = (wvalid && cw < a.chunks) ? *reinterpret_cast<const float4*>(wb + (size_t)cw * a.Cout * KC) : zero4();
    }
  };

  f32x4 acc[4];
#pragma unroll
  for (int i = 0; i < 4; i++) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool wave_live = m0 + (size_t)wv * 16 < a.M;
  const int frow = lane & 15, fq = lane >> 4;

  load_stage(0);
  for (int st = 0; st < nstages; st++) {
    __syncthreads();                                                // the previous stage's fragments have been read
    // slot q of the pixel's row: k = q, q + 4, q + 8, q + 12 = element q of the four loads
    *slot(lds_x[lch], lrow, 0) = make_float4(rx[0].x, rx[1].x, rx[2].x, rx[3].x);
    *slot(lds_x[lch], lrow, 1) = make_float4(rx[0].y, rx[1].y, rx[2].y, rx[3].y);
    *slot(lds_x[lch], lrow, 2) = make_float4(rx[0].z, rx[1].z, rx[2].z, rx[3].z);
    *slot(lds_x[lch], lrow, 3) = make_float4(rx[0].w, rx[1].w, rx[2].w, rx[3].w);
#pragma unroll
    for (int j = 0; j < 4; j++) *slot(lds_w[j], wrow, wpart) = rw[j];
    __syncthreads();
    if (st + 1 < nstages) load_stage(st + 1);                       // in flight under this stage's MFMAs
    if (wave_live) {
      const int nc = min(CPS, a.chunks - st * CPS);
      for (int c = 0; c < nc; c++) {
        const float4 xf = *slot(lds_x[c], wv * 16 + frow, fq);
        const float xs[4] = {xf.x, xf.y, xf.z, xf.w};
        float4 wf[4];
#pragma unroll
        for (int ns = 0; ns < 4; ns++) wf[ns] = ns < nsub ? *slot(lds_w[c], ns * 16 + frow, fq) : zero4();
#pragma unroll
        for (int s = 0; s < 4; s++) {
#pragma unroll
          for (int ns = 0; ns < 4; ns++) {
            if (ns < nsub) {
              const float ws = s == 0 ? wf[ns].x : s == 1 ? wf[ns].y : s == 2 ? wf[ns].z : wf[ns].w;
              acc[ns] = __builtin_amdgcn_mfma_f32_16x16x4f32(ws, xs[s], acc[ns], 0, 0, 0);
            }
          }
        }
      }
    }
  }

  // lane: pixel m0 + 16 wv + (lane & 15), channels n0 + 16 ns + 4 (lane >> 4) .. + 3 of accumulator ns
  const size_t mo = m0 + (size_t)wv * 16 + frow;
  if (mo < a.M) {
#pragma unroll
    for (int ns = 0; ns < 4; ns++) {
      if (ns < nsub) {
        const int n = n0 + ns * 16 + fq * 4;
        const float4 sc = a.scale ? *reinterpret_cast<const float4*>(a.scale + n) : make_float4(1.f, 1.f, 1.f, 1.f);
        const float4 sh = a.shift ? *reinterpret_cast<const float4*>(a.shift + n) : zero4();
        float4 r = make_float4(__builtin_fmaf(acc[ns][0], sc.x, sh.x), __builtin_fmaf(acc[ns][1], sc.y, sh.y), __builtin_fmaf(acc[ns][2], sc.z, sh.z),
                               __builtin_fmaf(acc[ns][3], sc.w, sh.w));
        if (a.relu) r = make_float4(fmaxf(r.x, 0.f), fmaxf(r.y, 0.f), fmaxf(r.z, 0.f), fmaxf(r.w, 0.f));
        *reinterpret_cast<float4*>(a.y + mo * (size_t)a.c_pitch + a.c_off + n) = r;
      }
    }
  }
}

// mode 0: max 3x3 stride 2 pad 0; 1: max 3x3 stride 1 pad 1; 2: average 3x3 stride 1 pad 1 over the taps inside the image
__global__ __launch_bounds__(256) void pool_kernel(const float* __restrict__ x, float* __restrict__ y, size_t total, int h, int w, int c, int ho, int wo, int mode,
                                                   int c_off, int c_pitch) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c4 = c >> 2;
  const int cc = (int)(i % (size_t)c4) * 4;
  const size_t pix = i / (size_t)c4;
  const int ox = (int)(pix % (size_t)wo), oy = (int)((pix / (size_t)wo) % (size_t)ho);
  const size_t b = pix / ((size_t)wo * ho);
  const int stride = mode == 0 ? 2 : 1, pad = mode == 0 ? 0 : 1;
  const float* xb = x + b * (size_t)h * w * c + cc;
  float4 r = mode == 2 ? zero4() : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
  int count = 0;
  for (int ky = 0; ky < 3; ky++) {
    const int iy = oy * stride - pad + ky;
    if (iy < 0 || iy >= h) continue;
    for (int kx = 0; kx < 3; kx++) {
      const int ix = ox * stride - pad + kx;
      if (ix < 0 || ix >= w) continue;
      const float4 v = *reinterpret_cast<const float4*>(xb + ((size_t)iy * w + ix) * c);
      if (mode == 2) r = make_float4(r.x + v.x, r.y + v.y, r.z + v.z, r.w + v.w);
      else r = make_float4(v.x > r.x ? v.x : r.x, v.y > r.y ? v.y : r.y, v.z > r.z ? v.z : r.z, v.w > r.w ? v.w : r.w);
      count++;
    }
  }
  if (mode == 2) {
    const float d = (float)count;                                   // >= 4 of the 9 taps are inside for every pixel of an image with h, w >= 2; >= 1 always
    r = make_float4(r.x / d, r.y / d, r.z / d, r.w / d);
  }
  *reinterpret_cast<float4*>(y + pix * (size_t)c_pitch + c_off + cc) = r;
}

// K x K maximum at stride 2 without padding (K = 2: floor, VGG16's pool; K = 3: ceil_mode, SqueezeNet 1.1's): every window starts inside the image (the host
// sizes ho, wo so), and a window that hangs over the bottom or right edge takes the maximum of the elements that exist -- its first element always does.
template <int K>
__global__ __launch_bounds__(256) void maxpool_kernel(const float* __restrict__ x, float* __restrict__ y, size_t total, int h, int w, int c, int ho, int wo,
                                                      int c_off, int c_pitch) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c4 = c >> 2;
  const int cc = (int)(i % (size_t)c4) * 4;
  const size_t pix = i / (size_t)c4;
  const int ox = (int)(pix % (size_t)wo), oy = (int)((pix / (size_t)wo) % (size_t)ho);
  const size_t b = pix / ((size_t)wo * ho);
  const float* xb = x + b * (size_t)h * w * c + cc;
  float4 r = *reinterpret_cast<const float4*>(xb + ((size_t)(2 * oy) * w + 2 * ox) * c);
#pragma unroll
  for (int ky = 0; ky < K; ky++) {
    const int iy = 2 * oy + ky;
    if (iy >= h) continue;
#pragma unroll
    for (int kx = 0; kx < K; kx++) {
      const int ix = 2 * ox + kx;
      if (ix >= w || (ky == 0 && kx == 0)) continue;
      const float4 v = *reinterpret_cast<const float4*>(xb + ((size_t)iy * w + ix) * c);
      r = make_float4(v.x > r.x ? v.x : r.x, v.y > r.y ? v.y : r.y, v.z > r.z ? v.z : r.z, v.w > r.w ? v.w : r.w);
    }
  }
  *reinterpret_cast<float4*>(y + pix * (size_t)c_pitch + c_off + cc) = r;
}

__global__ __launch_bounds__(256) void global_avgpool_kernel(const float* __restrict__ x, float* __restrict__ y, size_t total, int hw, int c) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const size_t b = i / (size_t)c, ch = i % (size_t)c;
  const float* p = x + b * (size_t)hw * c + ch;
  double s = 0.0;
  for (int j = 0; j < hw; j++) s += (double)p[(size_t)j * c];
  y[i] = (float)(s / (double)hw);
}

template <typename T>
__global__ __launch_bounds__(256) void input_kernel(const T* __restrict__ x, float* __restrict__ y, size_t total, size_t hw) {
#pragma clang fp contract(off)
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const size_t ch = i % 3, pix = i / 3, b = pix / hw, p = pix - b * hw;
  const T v = x[(b * 3 + ch) * hw + p];
  if constexpr (sizeof(T) == 1) y[i] = ((float)v - 128.0f) / 128.0f;
  else y[i] = v;
}

constexpr size_t GRID_MAX = 0x7fffffffull;

inline bool conv_form_ok(int kh, int kw, int stride, int ph, int pw) {
  if (kh == 1 && kw == 1) return stride == 1 && ph == 0 && pw == 0;
  if (kh == 3 && kw == 3) return (ph == 0 && pw == 0 && (stride == 1 || stride == 2)) || (ph == 1 && pw == 1 && stride == 1);
  if (kh == 5 && kw == 5) return stride == 1 && ph == 2 && pw == 2;
  if (kh == 1 && kw == 7) return stride == 1 && ph == 0 && pw == 3;
  if (kh == 7 && kw == 1) return stride == 1 && ph == 3 && pw == 0;
  if (kh == 1 && kw == 3) return stride == 1 && ph == 0 && pw == 1;
  if (kh == 3 && kw == 1) return stride == 1 && ph == 1 && pw == 0;
  return false;
}

}  // namespace dmvae_inception

extern "C" int dmvae_conv2d_f32_fwd(const float* x, const float* w_packed, const float* scale, const float* shift, float* y, int batch, int h, int w, int cin,
                                    int cout, int kh, int kw, int stride, int pad_h, int pad_w, int relu, int out_c_offset, int out_c_pitch,
                                    hipStream_t stream) {
  using namespace dmvae_inception;
  DMVAE_CHECK_ARG(x && w_packed && y, "conv2d_f32_fwd: NULL pointer (x, w_packed and y are required; scale and shift may be NULL)");
  const bool form11 = kh == 11 && kw == 11;                          // AlexNet's first layer (dmvae_amd/models/lpips_alex.py): one more form of the CIN3 loader
  DMVAE_CHECK_ARG(!form11 || (stride == 4 && pad_h == 2 && pad_w == 2),
                  "conv2d_f32_fwd: kernel (11, 11) is built at stride 4 padding (2, 2) only, got stride %d padding (%d, %d)", stride, pad_h, pad_w);
  DMVAE_CHECK_ARG(!form11 || cin == 3, "conv2d_f32_fwd: kernel (11, 11) is built for cin 3 only, got cin %d", cin);
  DMVAE_CHECK_ARG(form11 || conv_form_ok(kh, kw, stride, pad_h, pad_w),
                  "conv2d_f32_fwd: kernel (%d, %d) stride %d padding (%d, %d) is not built: 1x1; 3x3 stride 1 or 2 pad 0; 3x3 pad 1; 5x5 pad 2; (1,7) pad (0,3); "
                  "(7,1) pad (3,0); (1,3) pad (0,1); (3,1) pad (1,0)", kh, kw, stride, pad_h, pad_w);
  DMVAE_CHECK_ARG(cin == 3 || (cin >= 16 && cin % 16 == 0), "conv2d_f32_fwd: cin must be 3 or a multiple of 16, got %d", cin);
  DMVAE_CHECK_ARG(cout >= 16 && cout % 16 == 0, "conv2d_f32_fwd: cout must be a multiple of 16, got %d", cout);
  DMVAE_CHECK_ARG(batch >= 1 && h >= 1 && w >= 1 && h <= 32768 && w <= 32768, "conv2d_f32_fwd: batch >= 1 and 1 <= h, w <= 32768 required, got %d x %d x %d",
                  batch, h, w);
  DMVAE_CHECK_ARG(h + 2 * pad_h >= kh && w + 2 * pad_w >= kw, "conv2d_f32_fwd: a %d x %d image is smaller than the (%d, %d) kernel", h, w, kh, kw);
  DMVAE_CHECK_ARG(out_c_offset >= 0 && out_c_offset % 4 == 0 && out_c_pitch % 4 == 0 && (long long)out_c_offset + cout <= (long long)out_c_pitch,
                  "conv2d_f32_fwd: channels [%d, %d + %d) do not fit an output of pitch %d (offset and pitch multiples of 4)", out_c_offset, out_c_offset, cout,
                  out_c_pitch);
  ConvArgs a;
  a.x = x, a.w = w_packed, a.scale = scale, a.shift = shift, a.y = y;
  a.H = h, a.W = w, a.Cin = cin, a.Cout = cout, a.kw = kw, a.stride = stride, a.ph = pad_h, a.pw = pad_w;
  a.Ho = (h + 2 * pad_h - kh) / stride + 1, a.Wo = (w + 2 * pad_w - kw) / stride + 1;
  a.relu = relu != 0, a.c_off = out_c_offset, a.c_pitch = out_c_pitch;
  a.M = (size_t)batch * a.Ho * a.Wo;
  DMVAE_CHECK_ARG((a.M + BM - 1) / BM <= GRID_MAX, "conv2d_f32_fwd: %zu output pixels exceed the grid's 2^31 - 1 tiles of 64", a.M);
  const dim3 grid((unsigned)((a.M + BM - 1) / BM), (unsigned)((cout + BN - 1) / BN));
  if (cin == 3) {
    a.cpt = kh * kw;                                                // the tap count: a chunk is four taps
    a.chunks = (kh * kw + 3) / 4;
    hipLaunchKernelGGL(conv_kernel<true>, grid, dim3(256), 0, stream, a);
  } else {
    a.cpt = cin / KC;
    a.chunks = kh * kw * a.cpt;
    hipLaunchKernelGGL(conv_kernel<false>, grid, dim3(256), 0, stream, a);
  }
  DMVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int dmvae_pool2d_f32(const float* x, float* y, int mode, int batch, int h, int w, int c, int out_c_offset, int out_c_pitch, hipStream_t stream) {
  using namespace dmvae_inception;
  DMVAE_CHECK_ARG(x && y, "pool2d_f32: NULL pointer");
  DMVAE_CHECK_ARG(mode >= 0 && mode <= 2, "pool2d_f32: mode must be 0 (max 3x3 stride 2), 1 (max 3x3 stride 1 pad 1) or 2 (average 3x3 stride 1 pad 1), got %d",
                  mode);
  DMVAE_CHECK_ARG(batch >= 1 && h >= 1 && w >= 1 && h <= 32768 && w <= 32768, "pool2d_f32: batch >= 1 and 1 <= h, w <= 32768 required, got %d x %d x %d", batch, h,
                  w);
  DMVAE_CHECK_ARG(mode != 0 || (h >= 3 && w >= 3), "pool2d_f32: the stride-2 pool has no padding and needs h, w >= 3, got %d x %d", h, w);
  DMVAE_CHECK_ARG(c >= 4 && c % 4 == 0, "pool2d_f32: c must be a multiple of 4, got %d", c);
  DMVAE_CHECK_ARG(out_c_offset >= 0 && out_c_offset % 4 == 0 && out_c_pitch % 4 == 0 && (long long)out_c_offset + c <= (long long)out_c_pitch,
                  "pool2d_f32: channels [%d, %d + %d) do not fit an output of pitch %d (offset and pitch multiples of 4)", out_c_offset, out_c_offset, c,
                  out_c_pitch);
  const int ho = mode == 0 ? (h - 3) / 2 + 1 : h, wo = mode == 0 ? (w - 3) / 2 + 1 : w;
  const size_t total = (size_t)batch * ho * wo * (size_t)(c / 4);
  DMVAE_CHECK_ARG((total + 255) / 256 <= GRID_MAX, "pool2d_f32: %zu outputs exceed the grid's 2^31 - 1 blocks of 256", total);
  hipLaunchKernelGGL(pool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, x, y, total, h, w, c, ho, wo, mode, out_c_offset, out_c_pitch);
  DMVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int dmvae_maxpool2d_f32(const float* x, float* y, int batch, int h, int w, int c, int kernel, int stride, int ceil_mode, int out_c_offset,
                                   int out_c_pitch, hipStream_t stream) {
  using namespace dmvae_inception;
  DMVAE_CHECK_ARG(x && y, "maxpool2d_f32: NULL pointer");
  const bool form2 = kernel == 2 && stride == 2 && ceil_mode == 0, form3 = kernel == 3 && stride == 2 && ceil_mode == 1;
  DMVAE_CHECK_ARG(form2 || form3, "maxpool2d_f32: kernel %d stride %d ceil_mode %d is not built: kernel 2 stride 2 ceil_mode 0; kernel 3 stride 2 ceil_mode 1",
                  kernel, stride, ceil_mode);
  DMVAE_CHECK_ARG(batch >= 1 && h >= 1 && w >= 1 && h <= 32768 && w <= 32768, "maxpool2d_f32: batch >= 1 and 1 <= h, w <= 32768 required, got %d x %d x %d", batch,
                  h, w);
  DMVAE_CHECK_ARG(h >= kernel && w >= kernel, "maxpool2d_f32: the pool has no padding and needs h, w >= %d, got %d x %d", kernel, h, w);
  DMVAE_CHECK_ARG(c >= 4 && c % 4 == 0, "maxpool2d_f32: c must be a multiple of 4, got %d", c);
  DMVAE_CHECK_ARG(out_c_offset >= 0 && out_c_offset % 4 == 0 && out_c_pitch % 4 == 0 && (long long)out_c_offset + c <= (long long)out_c_pitch,
                  "maxpool2d_f32: channels [%d, %d + %d) do not fit an output of pitch %d (offset and pitch multiples of 4)", out_c_offset, out_c_offset, c,
                  out_c_pitch);
  const int ho = form2 ? h / 2 : (h - 2) / 2 + 1, wo = form2 ? w / 2 : (w - 2) / 2 + 1;      // ceil((h - 3) / 2) + 1 = (h - 2) / 2 + 1 for h >= 3
  const size_t pixels = (size_t)batch * ho * wo, quads = (size_t)(c / 4);      // < 2^61; the product is formed only once it is known to fit
  DMVAE_CHECK_ARG(pixels <= GRID_MAX * 256 / quads, "maxpool2d_f32: %zu pixels x %zu channel quads exceed the grid's 2^31 - 1 blocks of 256", pixels, quads);
  const size_t total = pixels * quads;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (form2) hipLaunchKernelGGL(maxpool_kernel<2>, grid, dim3(256), 0, stream, x, y, total, h, w, c, ho, wo, out_c_offset, out_c_pitch);
  else hipLaunchKernelGGL(maxpool_kernel<3>, grid, dim3(256), 0, stream, x, y, total, h, w, c, ho, wo, out_c_offset, out_c_pitch);
  DMVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int dmvae_global_avgpool_f32(const float* x, float* y, int batch, int h, int w, int c, hipStream_t stream) {
  using namespace dmvae_inception;
  DMVAE_CHECK_ARG(x && y, "global_avgpool_f32: NULL pointer");
  DMVAE_CHECK_ARG(batch >= 1 && h >= 1 && w >= 1 && c >= 1 && h <= 32768 && w <= 32768, "global_avgpool_f32: batch, c >= 1 and 1 <= h, w <= 32768 required, got "
                  "%d x %d x %d x %d", batch, h, w, c);
  const size_t total = (size_t)batch * c;
  DMVAE_CHECK_ARG((total + 255) / 256 <= GRID_MAX, "global_avgpool_f32: %zu outputs exceed the grid's 2^31 - 1 blocks of 256", total);
  hipLaunchKernelGGL(global_avgpool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, x, y, total, h * w, c);
  DMVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int dmvae_inception_input(const void* x, int is_u8, float* y, int batch, int h, int w, hipStream_t stream) {
  using namespace dmvae_inception;
  DMVAE_CHECK_ARG(x && y, "inception_input: NULL pointer");
  DMVAE_CHECK_ARG(batch >= 1 && h >= 1 && w >= 1 && h <= 32768 && w <= 32768, "inception_input: batch >= 1 and 1 <= h, w <= 32768 required, got %d x %d x %d",
                  batch, h, w);
  const size_t hw = (size_t)h * w, total = (size_t)batch * hw * 3;
  DMVAE_CHECK_ARG((total + 255) / 256 <= GRID_MAX, "inception_input: %zu outputs exceed the grid's 2^31 - 1 blocks of 256", total);
  const dim3 grid((unsigned)((total + 255) / 256));
  if (is_u8) hipLaunchKernelGGL(input_kernel<uint8_t>, grid, dim3(256), 0, stream, (const uint8_t*)x, y, total, hw);
  else hipLaunchKernelGGL(input_kernel<float>, grid, dim3(256), 0, stream, (const float*)x, y, total, hw);
  DMVAE_CHECK_LAUNCH();
  return 0;
}
