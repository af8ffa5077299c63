// Multi-tensor optimiser tail: the arithmetic of optim.hip over a device TABLE of ordinary, separately allocated tensors instead of one flat buffer -- what
// torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW.step + update_ema's per-tensor loop do in the reference's own training loop
// (train_tokenizer.py:140-150,382,415-419,437; train_dmd.py:473-475,540-574; train_diffusion.py:209,293-297), whose parameters cannot be re-homed into flat
// buffers (zero_grad(set_to_none=True), stock DDP, deepcopy).  One record per tensor, a chunk list {tensor, first element} of fixed chunk length next to it; a
// workgroup claims chunks in a grid-stride loop, so ONE launch covers any number of tensors.  HBM-bound streaming kernels: every lane moves 16 B per stream where
// the record's pointers are 16-byte aligned (chunks start at multiples of the chunk length, so a tensor's alignment is its base pointers'), 4 B otherwise
// (views, odd storage offsets: tensors are only guaranteed 4-byte aligned); consecutive lanes touch consecutive addresses in both forms.
#include "common.h"
#include "optim_common.h"
#include "dmvae_hip.h"

namespace dmvae_optim {

constexpr int MT_BLOCK = 256;
constexpr size_t MT_CHUNK = 4096;      // elements per chunk: four 16-B vectors per lane; 16 KiB per stream and workgroup visit
constexpr int MT_GRID_CAP = 2048;      // 8 workgroups per CU; the per-chunk partial sums are laid out by chunk, not by grid, so the cap does not enter the norm's bits

// the chunk's record, its first element and its length; false for an entry that does not lie inside the table (a corrupt list is skipped, never followed)
__device__ __forceinline__ bool mt_chunk(const dmvae_mt_tensor* __restrict__ table, size_t n_tensors, const dmvae_mt_chunk* __restrict__ chunks, size_t ci,
                                         dmvae_mt_tensor& rec, size_t& first, int& n) {
  const dmvae_mt_chunk c = chunks[ci];
  if (c.tensor >= n_tensors) return false;
  rec = table[c.tensor];
  if (c.first >= rec.numel) return false;
  first = c.first;
  const size_t left = rec.numel - c.first;
  n = (int)(left < MT_CHUNK ? left : MT_CHUNK);
  return true;
}
__device__ __forceinline__ bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr, const void* e = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d | (uintptr_t)e) & 15) == 0;
}

// part[chunk] = sum of g^2 over the chunk: per lane in element order, then the wave, then the four waves -- a fixed order, so two calls give the same bits.
__global__ __launch_bounds__(MT_BLOCK) void mt_sumsq_kernel(const dmvae_mt_tensor* __restrict__ table, size_t n_tensors, const dmvae_mt_chunk* __restrict__ chunks,
                                                            size_t n_chunks, float* __restrict__ part) {
  __shared__ float sh[4];
  for (size_t ci = blockIdx.x; ci < n_chunks; ci += gridDim.x) {
    dmvae_mt_tensor rec; size_t first; int n;
    float s = 0.f;
    if (mt_chunk(table, n_tensors, chunks, ci, rec, first, n) && rec.g) {
      const float* g = (const float*)rec.g + first;
      if (aligned16(g)) {
        const int n4 = n / 4;
        for (int i = threadIdx.x; i < n4; i += MT_BLOCK) {
          const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g) + i);
          s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
        }
        if ((int)threadIdx.x < (n & 3)) { const float v = g[n4 * 4 + threadIdx.x]; s += v * v; }
      } else {
        for (int i = threadIdx.x; i < n; i += MT_BLOCK) { const float v = g[i]; s += v * v; }
      }
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[ci] = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
  }
}

// g *= clip[1] in place: what clip_grad_norm_ does to the gradients themselves
__global__ __launch_bounds__(MT_BLOCK) void mt_scale_kernel(const dmvae_mt_tensor* __restrict__ table, size_t n_tensors, const dmvae_mt_chunk* __restrict__ chunks,
                                                            size_t n_chunks, const float* __restrict__ clip) {
  const float coef = clip[1];
  for (size_t ci = blockIdx.x; ci < n_chunks; ci += gridDim.x) {
    dmvae_mt_tensor rec; size_t first; int n;
    if (!mt_chunk(table, n_tensors, chunks, ci, rec, first, n) || !rec.g) continue;
    float* g = (float*)rec.g + first;
    if (aligned16(g)) {
      const int n4 = n / 4;
      for (int i = threadIdx.x; i < n4; i += MT_BLOCK) {
        f32x4 v = reinterpret_cast<const f32x4*>(g)[i];
        v[0] *= coef; v[1] *= coef; v[2] *= coef; v[3] *= coef;
        reinterpret_cast<f32x4*>(g)[i] = v;
      }
      if ((int)threadIdx.x < (n & 3)) g[n4 * 4 + threadIdx.x] *= coef;
    } else {
      for (int i = threadIdx.x; i < n; i += MT_BLOCK) g[i] *= coef;
    }
  }
}

// adamw_ema_kernel's body (optim.hip) per chunk; the gradient is read once (non-temporal), p, m, v and ema are read and written once
__global__ __launch_bounds__(MT_BLOCK) void mt_adamw_ema_kernel(const dmvae_mt_tensor* __restrict__ table, size_t n_tensors, const dmvae_mt_chunk* __restrict__ chunks,
                                                                size_t n_chunks, const float* __restrict__ clip, float lr, float b1, float b2, float eps, float wd,
                                                                float bc1, float bc2_sqrt, float decay) {
  const float coef = clip ? clip[1] : 1.f;
  const float step = lr / bc1;
  for (size_t ci = blockIdx.x; ci < n_chunks; ci += gridDim.x) {
    dmvae_mt_tensor rec; size_t first; int n;
    if (!mt_chunk(table, n_tensors, chunks, ci, rec, first, n) || !rec.p || !rec.g || !rec.m || !rec.v) continue;
    float* p = (float*)rec.p + first;
    const float* g = (const float*)rec.g + first;
    float* m = (float*)rec.m + first;
    float* v = (float*)rec.v + first;
    float* ema = rec.ema ? (float*)rec.ema + first : nullptr;
    if (aligned16(p, g, m, v, ema)) {
      const int n4 = n / 4;
      for (int i = threadIdx.x; i < n4; i += MT_BLOCK) {
        f32x4 pv = reinterpret_cast<const f32x4*>(p)[i], mv = reinterpret_cast<const f32x4*>(m)[i], vv = reinterpret_cast<const f32x4*>(v)[i];
        const f32x4 gv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g) + i);
        f32x4 ev = {0.f, 0.f, 0.f, 0.f};
        if (ema) ev = reinterpret_cast<const f32x4*>(ema)[i];
#pragma unroll
        for (int e = 0; e < 4; e++) {
          float pe = pv[e], me = mv[e], ve = vv[e], ee = ev[e];
          adamw_one(pe, gv[e], me, ve, ema ? &ee : nullptr, coef, lr, b1, b2, eps, wd, step, bc2_sqrt, decay);
          pv[e] = pe; mv[e] = me; vv[e] = ve; ev[e] = ee;
        }
        reinterpret_cast<f32x4*>(p)[i] = pv;
        reinterpret_cast<f32x4*>(m)[i] = mv;
        reinterpret_cast<f32x4*>(v)[i] = vv;
        if (ema) reinterpret_cast<f32x4*>(ema)[i] = ev;
      }
      if ((int)threadIdx.x < (n & 3)) {
        const int i = n4 * 4 + threadIdx.x;
        float pe = p[i], me = m[i], ve = v[i], ee = ema ? ema[i] : 0.f;
        adamw_one(pe, g[i], me, ve, ema ? &ee : nullptr, coef, lr, b1, b2, eps, wd, step, bc2_sqrt, decay);
        p[i] = pe; m[i] = me; v[i] = ve;
        if (ema) ema[i] = ee;
      }
    } else {
      for (int i = threadIdx.x; i < n; i += MT_BLOCK) {
        float pe = p[i], me = m[i], ve = v[i], ee = ema ? ema[i] : 0.f;
        adamw_one(pe, __builtin_nontemporal_load(g + i), me, ve, ema ? &ee : nullptr, coef, lr, b1, b2, eps, wd, step, bc2_sqrt, decay);
        p[i] = pe; m[i] = me; v[i] = ve;
        if (ema) ema[i] = ee;
      }
    }
  }
}

// the last line of adamw_one alone (ema_one, optim_common.h), over (ema, p) pairs
__global__ __launch_bounds__(MT_BLOCK) void mt_ema_kernel(const dmvae_mt_tensor* __restrict__ table, size_t n_tensors, const dmvae_mt_chunk* __restrict__ chunks,
                                                          size_t n_chunks, float decay) {
  for (size_t ci = blockIdx.x; ci < n_chunks; ci += gridDim.x) {
    dmvae_mt_tensor rec; size_t first; int n;
    if (!mt_chunk(table, n_tensors, chunks, ci, rec, first, n) || !rec.p || !rec.ema) continue;
    const float* p = (const float*)rec.p + first;
    float* ema = (float*)rec.ema + first;
    if (aligned16(p, ema)) {
      const int n4 = n / 4;
      for (int i = threadIdx.x; i < n4; i += MT_BLOCK) {
        const f32x4 pv = reinterpret_cast<const f32x4*>(p)[i];
        f32x4 ev = reinterpret_cast<const f32x4*>(ema)[i];
#pragma unroll
        for (int e = 0; e < 4; e++) ev[e] = ema_one(ev[e], pv[e], decay);
        reinterpret_cast<f32x4*>(ema)[i] = ev;
      }
      if ((int)threadIdx.x < (n & 3)) { const int i = n4 * 4 + threadIdx.x; ema[i] = ema_one(ema[i], p[i], decay); }
    } else {
      for (int i = threadIdx.x; i < n; i += MT_BLOCK) ema[i] = ema_one(ema[i], p[i], decay);
    }
  }
}

}  // namespace dmvae_optim
using namespace dmvae_optim;

#define MT_CHECK_TABLE(name) \
  do { \
    if (n_tensors == 0) return 0; \
    DMVAE_CHECK_ARG(table, name ": null table"); \
    DMVAE_CHECK_ARG(chunks, name ": null chunk list"); \
    DMVAE_CHECK_ARG(n_chunks <= 0x7fffffffu, name ": more than 2^31 - 1 chunks"); \
  } while (0)

extern "C" size_t dmvae_mt_chunk_elems(void) { return MT_CHUNK; }

extern "C" size_t dmvae_mt_grad_norm_workspace(size_t n_chunks) { return (n_chunks < 1 ? 1 : n_chunks) * sizeof(float); }

extern "C" int dmvae_mt_grad_norm(const dmvae_mt_tensor* table, size_t n_tensors, const dmvae_mt_chunk* chunks, size_t n_chunks, void* norm_out3, void* workspace,
                                  size_t workspace_bytes, float max_norm, hipStream_t stream) {
  MT_CHECK_TABLE("mt_grad_norm");
  DMVAE_CHECK_ARG(norm_out3 && workspace, "mt_grad_norm: null pointer");
  DMVAE_CHECK_ARG(workspace_bytes >= dmvae_mt_grad_norm_workspace(n_chunks), "mt_grad_norm: workspace too small");
  if (n_chunks) {
    hipLaunchKernelGGL(mt_sumsq_kernel, dim3(grid_for(n_chunks, 1, MT_GRID_CAP)), dim3(MT_BLOCK), 0, stream, table, n_tensors, chunks, n_chunks, (float*)workspace);
    DMVAE_CHECK_LAUNCH();
  }
  return norm_final_launch((const float*)workspace, (float*)norm_out3, (int)n_chunks, max_norm, 0, stream);
}

extern "C" int dmvae_mt_scale_grads(const dmvae_mt_tensor* table, size_t n_tensors, const dmvae_mt_chunk* chunks, size_t n_chunks, const void* norm_out3,
                                    hipStream_t stream) {
  MT_CHECK_TABLE("mt_scale_grads");
  DMVAE_CHECK_ARG(norm_out3, "mt_scale_grads: null pointer");
  if (n_chunks == 0) return 0;
  hipLaunchKernelGGL(mt_scale_kernel, dim3(grid_for(n_chunks, 1, MT_GRID_CAP)), dim3(MT_BLOCK), 0, stream, table, n_tensors, chunks, n_chunks, (const float*)norm_out3);
  DMVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int dmvae_mt_adamw_ema_step(const dmvae_mt_tensor* table, size_t n_tensors, const dmvae_mt_chunk* chunks, size_t n_chunks, const void* norm_out3, float lr,
                                       float beta1, float beta2, float eps, float weight_decay, int step, float ema_decay, hipStream_t stream) {
  DMVAE_CHECK_ARG(step >= 1, "mt_adamw_ema_step: step counts from 1");
  MT_CHECK_TABLE("mt_adamw_ema_step");
  if (n_chunks == 0) return 0;
  const float bc1 = 1.f - powf(beta1, (float)step);       // as adamw_launch (optim.hip) forms them
  const float bc2 = 1.f - powf(beta2, (float)step);
  hipLaunchKernelGGL(mt_adamw_ema_kernel, dim3(grid_for(n_chunks, 1, MT_GRID_CAP)), dim3(MT_BLOCK), 0, stream, table, n_tensors, chunks, n_chunks,
                     (const float*)norm_out3, lr, beta1, beta2, eps, weight_decay, bc1, sqrtf(bc2), ema_decay);
  DMVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int dmvae_mt_ema(const dmvae_mt_tensor* table, size_t n_tensors, const dmvae_mt_chunk* chunks, size_t n_chunks, float decay, hipStream_t stream) {
  MT_CHECK_TABLE("mt_ema");
  if (n_chunks == 0) return 0;
  hipLaunchKernelGGL(mt_ema_kernel, dim3(grid_for(n_chunks, 1, MT_GRID_CAP)), dim3(MT_BLOCK), 0, stream, table, n_tensors, chunks, n_chunks, decay);
  DMVAE_CHECK_LAUNCH();
  return 0;
}
