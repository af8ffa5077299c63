// The all-pairs metrics of the evaluation tail (sample_50k.py:185-199, evaluation/fid.py:15-45: torch-fidelity's `prc` and `kid` over [N, 2048] feature sets):
// k-th nearest-neighbour radii, manifold membership and the polynomial-kernel MMD^2 of KID's subsets, all f64, nothing N x N in memory.  torch-fidelity is on
// none of the machines this was developed on: the definitions restate its published `calc_cdist_part(...).kthvalue(k + 1)`, `(dist <= radii).any(dim=1)` and
// `polynomial_mmd`; tests/manifold_spec.py restates them in numpy, and agreement with the library itself has not been run.
//
// gram_tile: G[i][j] = sum_f A[i][f] * B[j][f] for one 64 x 64 block on v_mfma_f64_16x16x4_f64.  Both operands are contiguous along the contraction (unlike
// fid.hip's X^T X), while the instruction wants one (row, k) element per lane -- A/B: row = lane & 15, k = lane >> 4; C/D: col = lane & 15, row = (lane >> 4) +
// 4 * reg, the f64 map, NOT the bf16 / f32 one -- so K-chunks of 16 go through LDS: thread t loads column t & 15 of rows (t >> 4) + 16 i of either operand (16
// lanes read one 64-B / 128-B run; scalar loads: no alignment is asked of the base or the pitch), widens to f64 (exact) and stores to a [64][18] f64 tile.  The
// pitch 18 (36 dwords): the 16 rows of a fragment read start at dword 36 r mod 64 = 0, 36, 8, 44, ... -- sixteen different multiples of 4 -- and the k-groups
// of a 32-lane pass sit 2 dwords apart: all 64 banks, no conflict.  Two LDS buffers, one barrier per chunk; the next chunk's global loads are issued before
// this chunk's 16 MFMAs per wave (past the end the last chunk is read again: no branch).  Wave w owns rows 16 w .. 16 w + 15 against the four 16-column tiles.
// A row past the operand's end is read as its last row (inside the buffer) and masked in every epilogue.  The pair (i, j) is accumulated over f in ascending
// k-steps of 4 from zero wherever it falls in a tile or in the grid: G[i][j] is a function of the two rows alone.
//
// norm_kernel runs the same instruction with a row as both operands and keeps the diagonal: |a_i|^2 has the bits the tile routine gives G[i][i], so two equal
// rows are at distance exactly 0.  d2(i, j) = max(0, (|a_i|^2 + |b_j|^2) - 2 G[i][j]).
//
// dmvae_knn_radius      workgroup (row block, column split) walks its column tiles; each lane keeps the 9 smallest d2 of each of its 4 rows (sorted insertion
//                       in registers; self distance set to 0), the 16 lanes of a row merge by an xor-shuffle butterfly, the splits' lists go through the
//                       workspace and a second kernel merges them and picks entry k.  Selection of exact values: independent of the split and of any order.
// dmvae_manifold_member the same walk with an OR of d2 <= radius2[j]; one byte per (split, query) in the workspace, OR-ed by a second kernel: one owner per byte.
// dmvae_kid_mmd2        workgroup (subset, xx / yy / xy, tile) gathers rows through the index tables, applies (gamma g + coef0)^degree by repeated
//                       multiplication (p = base; p = p * base, degree - 1 times; no contraction), sums its tile lane-first (tile column ascending, then
//                       register), lanes by an xor tree, waves 0..3 in order; one workgroup per subset adds the partials in a fixed order.  No atomics.
// The number of column splits is a function of the row and column counts alone (512 workgroups are aimed at), never of the device.
#include <math.h>

#include "common.h"
#include "dmvae_hip.h"

namespace dmvae_manifold {

typedef __attribute__((ext_vector_type(4))) double f64x4;

constexpr int BLK = 64;                   // rows of either operand per workgroup tile: 4 waves x 16 rows against 4 tiles of 16 columns
constexpr int KC = 16;                    // contraction elements staged per chunk: 4 MFMA k-steps
constexpr int PITCH = KC + 2;             // f64 row pitch of a staged tile (header comment)
constexpr int TILE_F64 = BLK * PITCH;     // one operand's staged chunk
constexpr int KEEP = 9;                   // smallest values kept per row: k + 1 at the largest k
constexpr size_t TARGET_WGS = 512;        // workgroups the column split aims at
constexpr size_t MAX_GRID = (1u << 24) - 1;   // workgroups of 256 threads one launch may have: the runtime refuses grid * block >= 2^32
constexpr size_t MAX_ROWS = BLK * MAX_GRID;   // 2^30 - 64 rows: their row blocks fit one launch, and the norm kernel's ceil(n / 16) waves of 64 stay below 2^32 threads

__host__ __device__ inline size_t tiles_of(size_t n) { return (n + BLK - 1) / BLK; }

// column splits of a (rows x cols) walk: a closed form of the two counts
inline size_t col_splits(size_t rows, size_t cols) {
  const size_t rb = tiles_of(rows), ct = tiles_of(cols);
  size_t s = (TARGET_WGS + rb - 1) / rb;
  s = s > ct ? ct : s;
  return s < 1 ? 1 : s;
}

template <typename T>
__device__ __forceinline__ void gram_tile(const T* __restrict__ a, const int64_t* __restrict__ atab, size_t a0, size_t na, size_t lda,
                                          const T* __restrict__ b, const int64_t* __restrict__ btab, size_t b0, size_t nb, size_t ldb, int f,
                                          double* __restrict__ lds, f64x4 (&acc)[4]) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, lk = lane >> 4;
  const int sc = tid & 15, sr = tid >> 4;                     // staging: column sc of rows sr + 16 i
  const T* pa[4];
  const T* pb[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    size_t p = a0 + sr + 16 * i;
    p = p < na ? p : na - 1;                                  // a row past the end is read as the last row and masked by the caller
    pa[i] = a + (atab ? (size_t)atab[p] : p) * lda + sc;
    size_t q = b0 + sr + 16 * i;
    q = q < nb ? q : nb - 1;
    pb[i] = b + (btab ? (size_t)btab[q] : q) * ldb + sc;
  }
  T ra[4], rb[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    ra[i] = pa[i][0];
    rb[i] = pb[i][0];
  }
#pragma unroll
  for (int j = 0; j < 4; j++) acc[j] = f64x4{0.0, 0.0, 0.0, 0.0};
  __syncthreads();                                            // the previous tile's last fragment reads
  int cur = 0;
  for (int k0 = 0; k0 < f; k0 += KC) {
    double* __restrict__ sa = lds + cur * 2 * TILE_F64;
    double* __restrict__ sb = sa + TILE_F64;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      sa[(sr + 16 * i) * PITCH + sc] = (double)ra[i];         // f32 -> f64 is exact
      sb[(sr + 16 * i) * PITCH + sc] = (double)rb[i];
    }
    __syncthreads();
    const int kn = k0 + KC < f ? k0 + KC : k0;                // the next chunk's loads fly under this chunk's MFMAs (past the end: this chunk again)
#pragma unroll
    for (int i = 0; i < 4; i++) {
      ra[i] = pa[i][kn];
      rb[i] = pb[i][kn];
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const double av = sa[(16 * w + lr) * PITCH + 4 * u + lk];
#pragma unroll
      for (int j = 0; j < 4; j++) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, sb[(16 * j + lr) * PITCH + 4 * u + lk], acc[j], 0, 0, 0);
    }
    cur ^= 1;
  }
}

// |x_i|^2 as the tile routine computes G[i][i]: one wave per 16 rows, the row as both operands, the diagonal kept
template <typename T>
__global__ __launch_bounds__(64) void norm_kernel(const T* __restrict__ x, size_t n, int f, size_t ld, double* __restrict__ out) {
  const int lane = threadIdx.x, lr = lane & 15, lk = lane >> 4;
  const size_t r0 = (size_t)blockIdx.x * 16;
  const size_t row = r0 + lr < n ? r0 + lr : n - 1;
  const T* __restrict__ p = x + row * ld + lk;
  f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < f; k0 += KC) {
    T v[4];
#pragma unroll
    for (int u = 0; u < 4; u++) v[u] = p[k0 + 4 * u];
#pragma unroll
    for (int u = 0; u < 4; u++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)v[u], (double)v[u], acc, 0, 0, 0);
  }
  // element (row lk + 4 reg, col lr) is on the diagonal where lr == lk + 4 reg
  if ((lr & 3) == lk && r0 + lr < n) {
    const int reg = lr >> 2;
    out[r0 + lr] = reg == 0 ? acc[0] : (reg == 1 ? acc[1] : (reg == 2 ? acc[2] : acc[3]));
  }
}

__device__ __forceinline__ double dist2(double na, double nb, double g) {
  const double d = (na + nb) - 2.0 * g;
  return d < 0.0 ? 0.0 : d;
}

// ascending list of the KEEP smallest values seen
__device__ __forceinline__ void keep_insert(double (&l)[KEEP], double v) {
  if (v < l[KEEP - 1]) {
#pragma unroll
    for (int t = 0; t < KEEP; t++) {
      const bool lt = v < l[t];
      const double lo = lt ? v : l[t], hi = lt ? l[t] : v;
      l[t] = lo;
      v = hi;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256, 2) void knn_kernel(const T* __restrict__ x, size_t n, int f, size_t ld, const double* __restrict__ norms,
                                                      double* __restrict__ lists, unsigned splits) {
  __shared__ double lds[4 * TILE_F64];
  const size_t rb = blockIdx.x / splits, sp = blockIdx.x % splits;
  const size_t row0 = rb * BLK, ct = tiles_of(n);
  const size_t t0 = sp * ct / splits, t1 = (sp + 1) * ct / splits;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, lc = lane & 15, lk = lane >> 4;
  size_t grow[4];
  double na[4], best[4][KEEP];
#pragma unroll
  for (int r = 0; r < 4; r++) {
    grow[r] = row0 + 16 * w + lk + 4 * r;
    na[r] = norms[grow[r] < n ? grow[r] : n - 1];
#pragma unroll
    for (int t = 0; t < KEEP; t++) best[r][t] = INFINITY;
  }
  for (size_t t = t0; t < t1; t++) {
    f64x4 acc[4];
    gram_tile<T>(x, nullptr, row0, n, ld, x, nullptr, t * BLK, n, ld, f, lds, acc);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const size_t gcol = t * BLK + 16 * j + lc;
      if (gcol < n) {                                         // a column past n never reaches a list
        const double nb = norms[gcol];
#pragma unroll
        for (int r = 0; r < 4; r++) keep_insert(best[r], gcol == grow[r] ? 0.0 : dist2(na[r], nb, acc[j][r]));      // the self distance is 0 by definition
      }
    }
  }
  // the 16 lanes that share lk hold the same rows: butterfly merge, after which each holds the KEEP smallest of the union
#pragma unroll
  for (int r = 0; r < 4; r++) {
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
      double other[KEEP];
#pragma unroll
      for (int t = 0; t < KEEP; t++) other[t] = __shfl_xor(best[r][t], off, 64);
#pragma unroll
      for (int t = 0; t < KEEP; t++) keep_insert(best[r], other[t]);
    }
    if (lc == 0 && grow[r] < n) {
#pragma unroll
      for (int t = 0; t < KEEP; t++) lists[(sp * n + grow[r]) * KEEP + t] = best[r][t];
    }
  }
}

__global__ __launch_bounds__(256) void knn_pick_kernel(const double* __restrict__ lists, size_t n, unsigned splits, int k, double* __restrict__ radius2) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double l[KEEP];
#pragma unroll
  for (int t = 0; t < KEEP; t++) l[t] = INFINITY;
  for (unsigned sp = 0; sp < splits; sp++) {
#pragma unroll
    for (int t = 0; t < KEEP; t++) keep_insert(l, lists[((size_t)sp * n + i) * KEEP + t]);
  }
  double v = l[0];
#pragma unroll
  for (int t = 1; t < KEEP; t++) v = t == k ? l[t] : v;
  radius2[i] = v;
}

template <typename T>
__global__ __launch_bounds__(256, 2) void member_kernel(const T* __restrict__ q, size_t nq, size_t ldq, const T* __restrict__ r, size_t nr, size_t ldr, int f,
                                                         const double* __restrict__ qn, const double* __restrict__ rn, const double* __restrict__ radius2,
                                                         uint8_t* __restrict__ part, unsigned splits) {
  __shared__ double lds[4 * TILE_F64];
  const size_t rb = blockIdx.x / splits, sp = blockIdx.x % splits;
  const size_t row0 = rb * BLK, ct = tiles_of(nr);
  const size_t t0 = sp * ct / splits, t1 = (sp + 1) * ct / splits;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, lc = lane & 15, lk = lane >> 4;
  size_t grow[4];
  double na[4];
  int in[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    grow[i] = row0 + 16 * w + lk + 4 * i;
    na[i] = qn[grow[i] < nq ? grow[i] : nq - 1];
    in[i] = 0;
  }
  for (size_t t = t0; t < t1; t++) {
    f64x4 acc[4];
    gram_tile<T>(q, nullptr, row0, nq, ldq, r, nullptr, t * BLK, nr, ldr, f, lds, acc);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const size_t gcol = t * BLK + 16 * j + lc;
      if (gcol < nr) {
        const double nb = rn[gcol], rad = radius2[gcol];
#pragma unroll
        for (int i = 0; i < 4; i++) in[i] |= dist2(na[i], nb, acc[j][i]) <= rad ? 1 : 0;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    int v = in[i];
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) v |= __shfl_xor(v, off, 64);
    if (lc == 0 && grow[i] < nq) part[sp * nq + grow[i]] = (uint8_t)v;
  }
}

__global__ __launch_bounds__(256) void member_or_kernel(const uint8_t* __restrict__ part, size_t nq, unsigned splits, uint8_t* __restrict__ member) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nq) return;
  uint8_t v = 0;
  for (unsigned sp = 0; sp < splits; sp++) v |= part[(size_t)sp * nq + i];
  member[i] = v;
}

// partials [subset][which][tile row][tile column], which = 0 xx, 1 yy, 2 xy
template <typename T>
__global__ __launch_bounds__(256, 2) void kid_kernel(const T* __restrict__ x, size_t ldx, const T* __restrict__ y, size_t ldy, int f,
                                                      const int64_t* __restrict__ idx1, const int64_t* __restrict__ idx2, size_t m, unsigned tiles, int degree,
                                                      double gamma, double coef0, double* __restrict__ partials) {
#pragma clang fp contract(off)
  __shared__ double lds[4 * TILE_F64];
  __shared__ double wsum[4];
  const unsigned flat = blockIdx.x, bj = flat % tiles, bi = (flat / tiles) % tiles, which = (flat / (tiles * tiles)) % 3;
  const size_t s = flat / (3 * tiles * tiles);
  const T* __restrict__ a = which == 1 ? y : x;
  const T* __restrict__ b = which == 0 ? x : y;
  const int64_t* __restrict__ atab = (which == 1 ? idx2 : idx1) + s * m;
  const int64_t* __restrict__ btab = (which == 0 ? idx1 : idx2) + s * m;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, lc = lane & 15, lk = lane >> 4;
  f64x4 acc[4];
  gram_tile<T>(a, atab, (size_t)bi * BLK, m, which == 1 ? ldy : ldx, b, btab, (size_t)bj * BLK, m, which == 0 ? ldx : ldy, f, lds, acc);
  double sum = 0.0;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const size_t pc = (size_t)bj * BLK + 16 * j + lc;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const size_t pr = (size_t)bi * BLK + 16 * w + lk + 4 * r;
      const double base = gamma * acc[j][r] + coef0;
      double p = base;
      for (int d = 1; d < degree; d++) p = p * base;
      sum += (pr < m && pc < m && (which == 2 || pr != pc)) ? p : 0.0;      // positions past m and the diagonal of xx / yy add nothing
    }
  }
  sum = block_sum_f64(sum, wsum);
  if (threadIdx.x == 0) partials[flat] = sum;
}

__global__ __launch_bounds__(256) void kid_finalize_kernel(const double* __restrict__ partials, size_t m, unsigned tiles, double* __restrict__ mmd2) {
#pragma clang fp contract(off)
  __shared__ double wsum[4];
  const size_t s = blockIdx.x, per = (size_t)tiles * tiles;
  double tot[3];
  for (int which = 0; which < 3; which++) {
    tot[which] = sum_partials_f64(partials + (s * 3 + which) * per, per, wsum);
    __syncthreads();                       // wsum is written again by the next sum
  }
  if (threadIdx.x == 0) {
    const double md = (double)m;
    mmd2[s] = (tot[0] + tot[1]) / (md * (md - 1.0)) - 2.0 * tot[2] / (md * md);
  }
}

inline bool is_f_ok(int f) { return f >= 16 && f <= 4096 && f % 16 == 0; }
inline size_t kid_tiles_total(size_t subsets, size_t m) { return subsets * 3 * tiles_of(m) * tiles_of(m); }
inline bool is_kid_size_ok(size_t subsets, size_t m) {
  return m >= 2 && m <= (1u << 20) && subsets >= 1 && subsets <= MAX_GRID && kid_tiles_total(subsets, m) <= MAX_GRID;
}

}  // namespace dmvae_manifold

extern "C" size_t dmvae_knn_radius_workspace(size_t n) {
  using namespace dmvae_manifold;
  if (n < 2 || n > MAX_ROWS) return 0;
  return (n + col_splits(n, n) * n * KEEP) * sizeof(double);
}

extern "C" int dmvae_knn_radius(const void* x, int dtype, size_t n, int f, size_t ld, int k, void* workspace, double* radius2, hipStream_t stream) {
  using namespace dmvae_manifold;
  DMVAE_CHECK_ARG(x && workspace && radius2, "knn_radius: NULL pointer");
  DMVAE_CHECK_ARG(dtype == 0 || dtype == 2, "knn_radius: dtype must be 0 (f32) or 2 (f64), got %d", dtype);
  DMVAE_CHECK_ARG(is_f_ok(f), "knn_radius: f must be a multiple of 16 in [16, 4096], got %d", f);
  DMVAE_CHECK_ARG(k >= 1 && k <= KEEP - 1, "knn_radius: k must lie in [1, %d], got %d", KEEP - 1, k);
  DMVAE_CHECK_ARG(n > (size_t)k && n <= MAX_ROWS, "knn_radius: n must lie in [k + 1 = %d, 2^30 - 64], got %zu", k + 1, n);
  DMVAE_CHECK_ARG(ld >= (size_t)f, "knn_radius: leading dimension %zu < f %d", ld, f);
  const size_t splits = col_splits(n, n);
  DMVAE_CHECK_ARG(tiles_of(n) * splits <= MAX_GRID, "knn_radius: %zu row blocks x %zu column splits exceed the grid", tiles_of(n), splits);
  double* norms = (double*)workspace;
  double* lists = norms + n;
  const dim3 ngrid((unsigned)((n + 15) / 16)), grid((unsigned)(tiles_of(n) * splits));
  if (dtype == 0) {
    hipLaunchKernelGGL(norm_kernel<float>, ngrid, dim3(64), 0, stream, (const float*)x, n, f, ld, norms);
    DMVAE_CHECK_LAUNCH();
    hipLaunchKernelGGL(knn_kernel<float>, grid, dim3(256), 0, stream, (const float*)x, n, f, ld, (const double*)norms, lists, (unsigned)splits);
  } else {
    hipLaunchKernelGGL(norm_kernel<double>, ngrid, dim3(64), 0, stream, (const double*)x, n, f, ld, norms);
    DMVAE_CHECK_LAUNCH();
    hipLaunchKernelGGL(knn_kernel<double>, grid, dim3(256), 0, stream, (const double*)x, n, f, ld, (const double*)norms, lists, (unsigned)splits);
  }
  DMVAE_CHECK_LAUNCH();
  hipLaunchKernelGGL(knn_pick_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (const double*)lists, n, (unsigned)splits, k, radius2);
  DMVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t dmvae_manifold_member_workspace(size_t nq, size_t nr) {
  using namespace dmvae_manifold;
  if (nq < 1 || nr < 1 || nq > MAX_ROWS || nr > MAX_ROWS) return 0;
  return (nq + nr) * sizeof(double) + (col_splits(nq, nr) * nq + 7) / 8 * 8;
}

extern "C" int dmvae_manifold_member(const void* q, size_t nq, size_t ldq, const void* r, size_t nr, size_t ldr, int dtype, int f, const double* radius2,
                                     void* workspace, uint8_t* member, hipStream_t stream) {
  using namespace dmvae_manifold;
  DMVAE_CHECK_ARG(q && r && radius2 && workspace && member, "manifold_member: NULL pointer");
  DMVAE_CHECK_ARG(dtype == 0 || dtype == 2, "manifold_member: dtype must be 0 (f32) or 2 (f64), got %d", dtype);
  DMVAE_CHECK_ARG(is_f_ok(f), "manifold_member: f must be a multiple of 16 in [16, 4096], got %d", f);
  DMVAE_CHECK_ARG(nq >= 1 && nq <= MAX_ROWS && nr >= 1 && nr <= MAX_ROWS, "manifold_member: nq and nr must lie in [1, 2^30 - 64], got %zu and %zu", nq, nr);
  DMVAE_CHECK_ARG(ldq >= (size_t)f && ldr >= (size_t)f, "manifold_member: leading dimensions %zu / %zu < f %d", ldq, ldr, f);
  const size_t splits = col_splits(nq, nr);
  DMVAE_CHECK_ARG(tiles_of(nq) * splits <= MAX_GRID, "manifold_member: %zu row blocks x %zu column splits exceed the grid", tiles_of(nq), splits);
  double* qn = (double*)workspace;
  double* rn = qn + nq;
  uint8_t* part = (uint8_t*)(rn + nr);
  const dim3 qgrid((unsigned)((nq + 15) / 16)), rgrid((unsigned)((nr + 15) / 16)), grid((unsigned)(tiles_of(nq) * splits));
#define DMVAE_MEMBER_LAUNCH(T)                                                                                                                          \
  do {                                                                                                                                                  \
    hipLaunchKernelGGL(norm_kernel<T>, qgrid, dim3(64), 0, stream, (const T*)q, nq, f, ldq, qn);                                                        \
    DMVAE_CHECK_LAUNCH();                                                                                                                               \
    hipLaunchKernelGGL(norm_kernel<T>, rgrid, dim3(64), 0, stream, (const T*)r, nr, f, ldr, rn);                                                        \
    DMVAE_CHECK_LAUNCH();                                                                                                                               \
    hipLaunchKernelGGL(member_kernel<T>, grid, dim3(256), 0, stream, (const T*)q, nq, ldq, (const T*)r, nr, ldr, f, (const double*)qn, (const double*)rn, \
                       radius2, part, (unsigned)splits);                                                                                                \
    DMVAE_CHECK_LAUNCH();                                                                                                                               \
  } while (0)
  if (dtype == 0) DMVAE_MEMBER_LAUNCH(float);
  else DMVAE_MEMBER_LAUNCH(double);
#undef DMVAE_MEMBER_LAUNCH
  hipLaunchKernelGGL(member_or_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, stream, (const uint8_t*)part, nq, (unsigned)splits, member);
  DMVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t dmvae_kid_mmd2_workspace(size_t subsets, size_t m) {
  using namespace dmvae_manifold;
  if (!is_kid_size_ok(subsets, m)) return 0;
  return kid_tiles_total(subsets, m) * sizeof(double);
}

extern "C" int dmvae_kid_mmd2(const void* x, size_t n1, size_t ldx, const void* y, size_t n2, size_t ldy, int dtype, int f, const int64_t* idx1,
                              const int64_t* idx2, size_t subsets, size_t m, int degree, double gamma, double coef0, void* workspace, double* mmd2,
                              hipStream_t stream) {
  using namespace dmvae_manifold;
  DMVAE_CHECK_ARG(x && y && idx1 && idx2 && workspace && mmd2, "kid_mmd2: NULL pointer");
  DMVAE_CHECK_ARG(dtype == 0 || dtype == 2, "kid_mmd2: dtype must be 0 (f32) or 2 (f64), got %d", dtype);
  DMVAE_CHECK_ARG(is_f_ok(f), "kid_mmd2: f must be a multiple of 16 in [16, 4096], got %d", f);
  DMVAE_CHECK_ARG(m >= 2 && m <= (1u << 20), "kid_mmd2: m must lie in [2, 2^20], got %zu", m);
  DMVAE_CHECK_ARG(n1 >= m && n2 >= m && n1 <= MAX_ROWS && n2 <= MAX_ROWS, "kid_mmd2: n1 and n2 must lie in [m = %zu, 2^30 - 64], got %zu and %zu", m, n1, n2);
  DMVAE_CHECK_ARG(is_kid_size_ok(subsets, m), "kid_mmd2: subsets >= 1 and at most 2^24 - 1 tiles (one launch) required, got %zu subsets of %zu", subsets, m);
  DMVAE_CHECK_ARG(degree >= 1 && degree <= 8, "kid_mmd2: degree must lie in [1, 8], got %d", degree);
  DMVAE_CHECK_ARG(ldx >= (size_t)f && ldy >= (size_t)f, "kid_mmd2: leading dimensions %zu / %zu < f %d", ldx, ldy, f);
  double* partials = (double*)workspace;
  const unsigned tiles = (unsigned)tiles_of(m);
  const dim3 grid((unsigned)kid_tiles_total(subsets, m));
  if (dtype == 0)
    hipLaunchKernelGGL(kid_kernel<float>, grid, dim3(256), 0, stream, (const float*)x, ldx, (const float*)y, ldy, f, idx1, idx2, m, tiles, degree, gamma, coef0,
                       partials);
  else
    hipLaunchKernelGGL(kid_kernel<double>, grid, dim3(256), 0, stream, (const double*)x, ldx, (const double*)y, ldy, f, idx1, idx2, m, tiles, degree, gamma, coef0,
                       partials);
  DMVAE_CHECK_LAUNCH();
  hipLaunchKernelGGL(kid_finalize_kernel, dim3((unsigned)subsets), dim3(256), 0, stream, (const double*)partials, m, tiles, mmd2);
  DMVAE_CHECK_LAUNCH();
  return 0;
}
