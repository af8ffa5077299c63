// The arithmetic around the FID's feature extractor (evaluation/fid.py:51-65 over torchmetrics' FrechetInceptionDistance): the f64 feature statistics
// sum += sum_n X[n, :], cov_sum += X^T X, and the bicubic resize to the extractor's input size with the uint8 quantisation folded in.  The extractor itself
// (InceptionV3) is not part of this library: dmvae_amd/fid.py takes it as a module.
//
// dmvae_fid_accumulate: X^T X on v_mfma_f64_16x16x4_f64.  A and B both come from X: lane l holds X[k0 + (l >> 4)][tile0 + (l & 15)] for either operand (one f64
// per lane, a 128-B run along F per 16 lanes for f64, 64 B for f32: no LDS staging), and the f64 form's C/D map is col = lane & 15, row = (lane >> 4) + 4 * reg
// -- NOT the bf16 / f32 maps of the other kernels.  A workgroup of four waves owns one 64 x 64 block (bi <= bj) of the upper triangle of cov_sum and its mirror
// image: wave w holds the 16 rows bi*64 + 16 w against the block's four 16-column tiles (in a diagonal block only the tiles at or right of its own).  N is
// walked in ascending order inside the wave, four rows per MFMA, with no atomics and no split over N: the grid depends on F alone, every element of the state
// has one owner, and the result is a function of (X, previous state) -- a second run gives the same bits.  The state is read from the upper triangle and added
// once, after the N loop; the owner writes the same f64 to [i][j] and [j][i] (the mirrored tile goes through LDS so that both stores are 128-B runs), and inside
// a diagonal tile the lower half takes the upper half's values, so cov_sum is exactly symmetric whatever the hardware does with a * b against b * a.
// The diagonal blocks own `sum`: each lane adds the A operands it loaded, the four lane groups are combined in a fixed order.
// The N loop has no branch and one wait: the raw loads of the next 16 rows are issued before the 16 MFMAs of this chunk; a row past N is read as row N - 1 --
// nothing past row N is ever read -- and becomes zero at the conversion; a tile the wave does not own (below the diagonal of a diagonal block, past F) runs on
// the A columns and is dropped.  (With a branch round every load the compiler waited for each load by itself: 4 - 5 x slower at N >= 256.)
//
// dmvae_fid_resize_u8: one thread per output pixel; F.interpolate(mode="bicubic", align_corners=False) as ATen's device kernel computes it (f32 scale
// in / out, source coordinate scale * (o + 0.5) - 0.5, Keys' weights with A = -0.75, taps clamped to the edge, rows first, then the column combination), then
// (x * 255).clamp(0, 255) and the truncation to uint8.  A bf16 image is rounded where the three ATen ops round: the interpolated value once, the product once.
#include "common.h"
#include "dmvae_hip.h"

namespace dmvae_fid {

typedef __attribute__((ext_vector_type(4))) double f64x4;

constexpr int BLK = 64;          // block of cov_sum per workgroup: 4 waves x 16 rows, 4 tiles of 16 columns
constexpr int KU = 4;            // MFMA k-steps (of 4 rows of X each) whose loads are issued together
constexpr int TLD = 17;          // f64 row pitch of a 16 x 16 tile in LDS (the transposed read walks a column)

// Raw loads of one chunk of 4 * KU rows: the A column and the four B columns of rows k0 + 4 u + lk.  A row past n is read as row n - 1 (always inside the
// buffer) and zeroed at the conversion: no branch and no wait between the loads.
template <typename T>
__device__ __forceinline__ void load_chunk(const T* __restrict__ x, size_t k0, size_t n, size_t ld, int lk, int col_a, const int (&col_b)[4], T (&ra)[KU],
                                           T (&rb)[KU][4]) {
#pragma unroll
  for (int u = 0; u < KU; u++) {
    const size_t row = k0 + 4 * u + lk;
    const T* __restrict__ p = x + (row < n ? row : n - 1) * ld;
    ra[u] = p[col_a];
#pragma unroll
    for (int j = 0; j < 4; j++) rb[u][j] = p[col_b[j]];
  }
}

template <typename T>
__global__ __launch_bounds__(256, 3) void accumulate_kernel(const T* __restrict__ x, size_t n, int f, size_t ld, double* __restrict__ sum,
                                                         double* __restrict__ cov, int nb) {
  __shared__ double tile[4][4][16 * TLD];
  // flat block index -> (bi, bj), bi <= bj, row-major over the upper triangle of the nb x nb block grid
  int bi = 0, rest = (int)blockIdx.x;
  while (rest >= nb - bi) { rest -= nb - bi; bi++; }
  const int bj = bi + rest;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int lc = lane & 15, lk = lane >> 4;
  const int r0 = bi * BLK + 16 * w;                           // this wave's rows of cov_sum
  const bool rows_ok = r0 < f;
  bool ok[4];
  int col_b[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    ok[j] = rows_ok && bj * BLK + 16 * j < f && (bi != bj || j >= w);
    col_b[j] = ok[j] ? bj * BLK + 16 * j + lc : r0 + lc;      // a tile this wave does not own runs on its A columns and is dropped: the loop has no branch
  }

  f64x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; j++) acc[j] = f64x4{0.0, 0.0, 0.0, 0.0};
  double colsum = 0.0;

  if (rows_ok) {
    T ra[KU], rb[KU][4];
    load_chunk(x, 0, n, ld, lk, r0 + lc, col_b, ra, rb);
    for (size_t k0 = 0; k0 < n; k0 += 4 * KU) {
      double a[KU], b[KU][4];
#pragma unroll
      for (int u = 0; u < KU; u++) {
        const bool in = k0 + 4 * u + lk < n;
        a[u] = in ? (double)ra[u] : 0.0;                      // bf16 -> f32 -> f64 and f32 -> f64 are exact
#pragma unroll
        for (int j = 0; j < 4; j++) b[u][j] = in ? (double)rb[u][j] : 0.0;
      }
      load_chunk(x, k0 + 4 * KU, n, ld, lk, r0 + lc, col_b, ra, rb);      // the next chunk's loads fly under this chunk's MFMAs (past the end: row n - 1 again)
#pragma unroll
      for (int u = 0; u < KU; u++) {
        colsum += a[u];
#pragma unroll
        for (int j = 0; j < 4; j++) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u][j], acc[j], 0, 0, 0);
      }
    }
  }

  // state add: element (row = lk + 4 reg, col = lc) of tile j
#pragma unroll
  for (int j = 0; j < 4; j++) {
    if (!ok[j]) continue;
    const int c0 = bj * BLK + 16 * j;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = lk + 4 * r;
      const double v = cov[(size_t)(r0 + row) * f + c0 + lc] + acc[j][r];
      acc[j][r] = v;
      tile[w][j][row * TLD + lc] = v;
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; j++) {
    if (!ok[j]) continue;
    const int c0 = bj * BLK + 16 * j;
    const bool diag = c0 == r0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = lk + 4 * r;
      if (diag) {                                             // the lower half of a diagonal tile is the upper half, read back transposed
        const double v = row <= lc ? acc[j][r] : tile[w][j][lc * TLD + row];
        cov[(size_t)(r0 + row) * f + c0 + lc] = v;
      } else {
        cov[(size_t)(r0 + row) * f + c0 + lc] = acc[j][r];
        cov[(size_t)(c0 + row) * f + r0 + lc] = tile[w][j][lc * TLD + row];      // mirrored tile: its element (row, lc) is this tile's (lc, row)
      }
    }
  }
  if (bi == bj && rows_ok) {                                  // the diagonal blocks own `sum`: lane groups combined 0 + 2, 1 + 3, then the two
    colsum += __shfl_xor(colsum, 32, 64);
    colsum += __shfl_xor(colsum, 16, 64);
    if (lane < 16) sum[r0 + lc] += colsum;
  }
}

__device__ __forceinline__ float cubic1(float x) { const float A = -0.75f; return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f; }
__device__ __forceinline__ float cubic2(float x) { const float A = -0.75f; return ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A; }

__device__ __forceinline__ void cubic_taps(float scale, int o, int size, int idx[4], float wgt[4]) {
  const float src = __fsub_rn(__fmul_rn(scale, (float)o + 0.5f), 0.5f);
  const float fl = floorf(src);
  const float t = src - fl;
  const int i0 = (int)fl;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int i = i0 - 1 + k;
    idx[k] = i < 0 ? 0 : (i > size - 1 ? size - 1 : i);
  }
  wgt[0] = cubic2(t + 1.f);
  wgt[1] = cubic1(t);
  wgt[2] = cubic1(1.f - t);
  wgt[3] = cubic2((1.f - t) + 1.f);
}

template <typename T>
__global__ __launch_bounds__(256) void resize_u8_kernel(const T* __restrict__ img, uint8_t* __restrict__ out, size_t total, int h, int w, int s) {
  constexpr bool BF = sizeof(T) == 2;
  const float sh = (float)h / (float)s, sw = (float)w / (float)s;
  const bool direct = h == s && w == s;
  for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < total; p += (size_t)gridDim.x * 256) {
    float v;
    if (direct) {
      v = (float)img[p];
    } else {
      const int ox = (int)(p % (size_t)s), oy = (int)((p / (size_t)s) % (size_t)s);
      const size_t plane = p / ((size_t)s * (size_t)s);
      const T* __restrict__ src = img + plane * (size_t)h * (size_t)w;
      int ix[4], iy[4];
      float wx[4], wy[4];
      cubic_taps(sw, ox, w, ix, wx);
      cubic_taps(sh, oy, h, iy, wy);
      float rows[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const T* __restrict__ r = src + (size_t)iy[k] * w;
        rows[k] = (float)r[ix[0]] * wx[0] + (float)r[ix[1]] * wx[1] + (float)r[ix[2]] * wx[2] + (float)r[ix[3]] * wx[3];
      }
      v = rows[0] * wy[0] + rows[1] * wy[1] + rows[2] * wy[2] + rows[3] * wy[3];
      if (BF) v = (float)(bf16)v;
    }
    float q = v * 255.f;
    if (BF) q = (float)(bf16)q;
    q = q < 0.f ? 0.f : (q > 255.f ? 255.f : q);              // NaN compares false twice and converts to 0 below, as in image_to_u8_kernel
    out[p] = (uint8_t)(int)(q == q ? q : 0.f);
  }
}

}  // namespace dmvae_fid

extern "C" int dmvae_fid_accumulate(const void* x, int x_dtype, size_t n, int f, size_t ld, void* sum, void* cov_sum, hipStream_t stream) {
  using namespace dmvae_fid;
  DMVAE_CHECK_ARG(x && sum && cov_sum, "fid_accumulate: NULL pointer");
  DMVAE_CHECK_ARG(x_dtype >= 0 && x_dtype <= 2, "fid_accumulate: x_dtype must be 0 (f32), 1 (bf16) or 2 (f64), got %d", x_dtype);
  DMVAE_CHECK_ARG(n > 0, "fid_accumulate: n > 0 required");
  DMVAE_CHECK_ARG(f >= 16 && f <= 4096 && f % 16 == 0, "fid_accumulate: f must be a multiple of 16 in [16, 4096], got %d", f);
  DMVAE_CHECK_ARG(ld >= (size_t)f, "fid_accumulate: leading dimension %zu < f %d", ld, f);
  const int nb = (f + BLK - 1) / BLK;
  const dim3 grid(nb * (nb + 1) / 2), block(256);             // F alone: never a function of n
  double* s = (double*)sum;
  double* c = (double*)cov_sum;
  if (x_dtype == 0) hipLaunchKernelGGL(accumulate_kernel<float>, grid, block, 0, stream, (const float*)x, n, f, ld, s, c, nb);
  else if (x_dtype == 1) hipLaunchKernelGGL(accumulate_kernel<bf16>, grid, block, 0, stream, (const bf16*)x, n, f, ld, s, c, nb);
  else hipLaunchKernelGGL(accumulate_kernel<double>, grid, block, 0, stream, (const double*)x, n, f, ld, s, c, nb);
  DMVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int dmvae_fid_resize_u8(const void* img, int is_bf16, size_t planes, int h, int w, int s, void* out, hipStream_t stream) {
  using namespace dmvae_fid;
  DMVAE_CHECK_ARG(img && out, "fid_resize_u8: NULL pointer");
  DMVAE_CHECK_ARG(planes > 0 && h >= 1 && w >= 1, "fid_resize_u8: planes > 0, h >= 1 and w >= 1 required, got h %d w %d", h, w);
  DMVAE_CHECK_ARG(s >= 1, "fid_resize_u8: s >= 1 required, got %d", s);
  const size_t total = planes * (size_t)s * (size_t)s;
  const int grid = grid_for(total, 256, 1 << 16);
  if (is_bf16) hipLaunchKernelGGL(resize_u8_kernel<bf16>, dim3(grid), dim3(256), 0, stream, (const bf16*)img, (uint8_t*)out, total, h, w, s);
  else hipLaunchKernelGGL(resize_u8_kernel<float>, dim3(grid), dim3(256), 0, stream, (const float*)img, (uint8_t*)out, total, h, w, s);
  DMVAE_CHECK_LAUNCH();
  return 0;
}
