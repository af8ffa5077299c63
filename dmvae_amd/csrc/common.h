// Shared device/host helpers for the DMVAE gfx950 kernels (MI355X / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef __bf16 bf16;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;

#define GPTR(p) ((const __attribute__((address_space(1))) void*)(p))
#define LPTR(p) ((__attribute__((address_space(3))) void*)(p))

// 64 B of zeros in device memory: source for padded / out-of-range rows of LDS-DMA tiles.
static __device__ uint4 dmvae_zero_page[4];  // one copy per translation unit (no -fgpu-rdc)

// error plumbing for the C ABI (thread-local last error string)
void dmvae_set_error(const char* fmt, ...);
#define DMVAE_CHECK_ARG(cond, ...) do { if (!(cond)) { dmvae_set_error(__VA_ARGS__); return -22; } } while (0)
#define DMVAE_CHECK_LAUNCH() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) { dmvae_set_error("%s:%d launch failed: %s", __FILE__, __LINE__, hipGetErrorString(e_)); return -5; } } while (0)

// Grid of a grid-stride kernel: ceil(n / block) blocks, at least 1, at most `cap`.  No default cap: some kernels lay their partial sums out by grid size, so
// every caller names the cap it was tuned and tested with.
static inline int grid_for(size_t n, int block, int cap) {
  size_t g = (n + block - 1) / block;
  return (int)(g > (size_t)cap ? cap : (g < 1 ? 1 : g));
}

// Opt-in to more than the default 64 KB of dynamic LDS, which a kernel needs set once on every device it is launched on (the attribute is kept per device, so
// a process-wide "done" flag would leave a second device without it and its launches failing).  `seen` is the call site's static: bit d = set on device d
// (devices past 63 share bit 63's "set it every time").  After the first call on a device this is one hipGetDevice and one relaxed load; no lock, no
// allocation -- two threads racing through the first call both set the same value.  Returns 0, or -5 with the site in dmvae_last_error().  (api.hip)
struct dmvae_lds_seen { unsigned long long devs; };
int dmvae_lds_optin(dmvae_lds_seen* seen, const void* kernel, int bytes, const char* file, int line);
// DMVAE_LDS_OPTIN(bytes, kernel<template, arguments>): in front of the launch, in a function that returns the C ABI's int
#define DMVAE_LDS_OPTIN(bytes, ...) do { static dmvae_lds_seen seen_; if (dmvae_lds_optin(&seen_, reinterpret_cast<const void*>(__VA_ARGS__), (int)(bytes), __FILE__, __LINE__)) return -5; } while (0)

// ---- primitives of the LDS-DMA pipelined kernels (conv_pp, gemm_pp, conv_wgrad_pp, wgrad_thin) ---------------------------------------------------------

// Raw buffer descriptor over `bytes` bytes at p (stride 0: voffset + soffset is a byte offset, range-checked against `bytes`; a load past it returns zeros, an
// LDS-DMA writes zeros, a store is dropped).  The last word is dword 3 of the gfx9 / CDNA descriptor: DATA_FORMAT (bits 18:15) = 4, BUF_DATA_FORMAT_32 (0 is
// BUF_DATA_FORMAT_INVALID), and everything else zero: no swizzle, no add-tid; dst_sel and num_format are not used by the untyped accesses of these kernels.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t dmvae_buffer_rsrc(const void* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, 0x00020000);
}
// A voffset beyond any descriptor's num_records: loads return zeros, the LDS-DMA writes zeros, stores are dropped.
constexpr unsigned SENT = 0x80000000u;

// Chunk key of 64-B LDS rows, 4 rows per 256-B bank row.  Fragments are read for v_mfma_f32_16x16x32_bf16: lane l takes the 16-B chunk l >> 4 of row (l & 15), and
// ds_read_b128 serves the lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31}, ... in one pass each; with the chunk XOR-ed by (-(row >> 2)) & 3 the four lanes of
// a group that share row % 4 land in four different 16-B slots of the bank row (derivation in DESIGN_HISTORY.md 3.1).
__device__ __forceinline__ int swz64(int row) { return (0 - (row >> 2)) & 3; }

// s_waitcnt vmcnt(N) through the builtin, not inline asm: the compiler's own wait-count pass then SEES the wait.  With the asm form it kept a VMEM event from
// before the K loop pending on a fragment register for ever (the loop's own LDS-DMA instructions make its count imprecise) and put an s_waitcnt vmcnt(0) in
// front of the second ds_read of every K tile.  Removing that drain changed nothing measurable in conv_pp (342 vs 340 us per launch in the step): by then the
// pieces of the next tiles have landed anyway -- the loop is not waiting on the DMA queue.
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit field on gfx9");
  __builtin_amdgcn_s_waitcnt((N & 15) | 0x0F70 | ((N >> 4) << 14));   // gfx9 encoding: vmcnt[3:0] | expcnt 7 | lgkmcnt 15 | vmcnt[5:4] << 14
  asm volatile("" ::: "memory");
}

// The transpose read (ds_read_b64_tr_b16) in two forms.  Which one a kernel takes depends on who orders it behind the writes of the tile it reads:
//
// tr_read_uncounted<OFF>(lds byte address): inline asm, for kernels whose LDS is filled by LDS-DMA into a ring.  The compiler's wait-count pass orders every
// LDS read it can see behind every earlier LDS-DMA (it cannot prove the ring slots disjoint) and put an s_waitcnt vmcnt(0) at the head of the K loop -- the
// three-tile prefetch queue was drained once per K tile and the loop ran at the latency of the newest piece (tools/loop_waits.py shows the skeleton;
// conv_wgrad_pp 128->128 @256^2: DESIGN_HISTORY.md 8.12).  The asm form carries no memory operand: the CALLER's counted wait_vmcnt + barrier protocol is what
// orders the read behind the pieces it needs, and the caller's lgkmcnt(0) ahead of the barrier covers the result.
template <int OFF>
__device__ __forceinline__ s16x4 tr_read_uncounted(unsigned lds_addr) {
  s16x4 r;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(r) : "v"(lds_addr), "n"(OFF));
  return r;
}
// tr_read_ordered(pointer into LDS): the builtin, for kernels that fill LDS with ordinary ds_write / global loads + __syncthreads(): the compiler sees the
// memory operand and places every wait itself.  Never inside an LDS-DMA ring (above).
__device__ __forceinline__ s16x4 tr_read_ordered(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(p));
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// ---- the f64 sums of the evaluation kernels (ssim, lpips_eval, fidelity, manifold; the butterfly also parity_dit, diffaug) ------------------------------
// These kernels promise the same bits on every run, alone or in any batch; that promise IS the order of the additions below.  Change none of it.
//
// One wave (all 64 lanes active): the xor butterfly at distances 32, 16, 8, 4, 2, 1 -- step o replaces every lane's v by v + (the v of lane ^ o).  The two
// lanes of a pair add the same two values (a + b and b + a: the same bits), so after the last step every lane holds the sum of one fixed binary tree.
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// One workgroup of exactly 256 threads, every thread calls: the butterfly per wave, lane 0 of wave w stores to wsum[w], ONE barrier, then
// ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3] in every thread: every thread gets the sum.  (Not (w0 + w1) + (w2 + w3): parity_dit.hip::block_sum_d_waves and
// diffaug.hip add the waves that way, parity.hip and sampler.hip through LDS trees; those are other bits and other functions.)  There is no barrier after
// the reads: a caller that writes wsum[4] again -- a second call on the same array -- puts a __syncthreads() between the two.
__device__ __forceinline__ double block_sum_f64(double v, double* wsum) {
  v = wave_sum_f64(v);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}
// One owner's n partial sums, 256 threads: thread t adds src[t], src[t + 256], ... in ascending order onto 0.0, then block_sum_f64 (and its rule for wsum).
__device__ __forceinline__ double sum_partials_f64(const double* __restrict__ src, size_t n, double* wsum) {
  double s = 0.0;
  for (size_t i = threadIdx.x; i < n; i += 256) s += src[i];
  return block_sum_f64(s, wsum);
}

__device__ __forceinline__ float bf2f(bf16 v) { return (float)v; }
// v_rcp_f32 (1 ulp), not an IEEE division: `1.0f / y` compiles to v_div_scale x2 + v_rcp + four FMAs + v_div_fmas + v_div_fixup -- ten instructions per element in
// kernels (GroupNorm backward: 23 of ~37 VALU instructions per element were the two divisions' sequences) whose results are rounded to bf16 anyway.
__device__ __forceinline__ float sigmoidf_(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float sigmoid_exact(float x) { return 1.0f / (1.0f + expf(-x)); }   // the f32 parity kernels' (parity.hip, parity_dit.hip): IEEE division, libm expf

// Exact-form GELU 0.5 x (1 + erf(x / sqrt 2)) (nn.GELU() of timm's Mlp, reached through models/vae.py:47-53) with erf from Abramowitz & Stegun 7.1.26
// (|error| <= 1.5e-7): E = (a1 t + ... + a5 t^5) exp(-z^2), t = 1 / (1 + p z), z = |x| / sqrt 2, and 1 + erf(x / sqrt 2) = E for x < 0, 2 - E for x >= 0 --
// the negative tail is computed without the 1 - erf cancellation.  ~15 VALU instructions, two of them transcendental, no branches; libm's erff is ~45 with two
// exec-masked branches, which as the epilogue of the fc1 GEMM (33.7 M values per call on ViT-L at batch 32) cost more than the HBM-bound stand-alone kernel
// it was fused to replace (29 vs 24 us).  Every result is rounded to bf16 (2^-9 relative) by its users, 1000 x coarser than the approximation.  Explicit
// fmaf: the stand-alone kernel (vit_bwd.hip) and the GEMM epilogue (gemm_pp.hip) give the same bits.
__device__ __forceinline__ float dmvae_gelu_f(float x) {
  const float z = fabsf(x) * 0.70710678118654752f;
  const float t = __builtin_amdgcn_rcpf(__builtin_fmaf(0.3275911f, z, 1.0f));
  float p = __builtin_fmaf(1.061405429f, t, -1.453152027f);
  p = __builtin_fmaf(p, t, 1.421413741f);
  p = __builtin_fmaf(p, t, -0.284496736f);
  p = __builtin_fmaf(p, t, 0.254829592f);
  const float e = p * t * __expf(-z * z);
  return 0.5f * x * (x < 0.f ? e : 2.0f - e);
}

// XCD-aware block order (MI355X: 8 XCDs with private L2s; the dispatcher places flat block b on XCD b % 8).
// Maps the flat dispatch index to a logical work index such that each XCD walks ONE contiguous range of logical
// indices in dispatch order, so blocks that are neighbours in logical order share an L2.  Bijective for any total.
// Placement is a speed assumption only; results do not depend on it.
__device__ __forceinline__ unsigned xcd_remap(unsigned flat, unsigned total) {
  const unsigned q = total >> 3, r = total & 7u, x = flat & 7u;
  const unsigned start = x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q;
  return start + (flat >> 3);
}

// 16-B load of a tensor this kernel reads ONCE: non-temporal, so that a streaming pass does not push the conv kernels' re-read operands out of L2 / the Infinity
// Cache (csrc/groupnorm.hip: -0.46 ms per step and 7-10 % on the passes themselves).
__device__ __forceinline__ bf16x8 dmvae_ldnt8(const bf16* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(p));
}
__device__ __forceinline__ unsigned dmvae_pack_bf16x2(float a, float b) {
  bf16x2 t = {(bf16)a, (bf16)b};
  return *reinterpret_cast<unsigned*>(&t);
}
// RMSNorm + RoPE of 8 consecutive channels d0..d0+7 of token `tok` (csrc/dit.hip::qknorm_rope_kernel's arithmetic: the normalised value is rounded to
// bf16 before the f32 weight multiplies; pairs (2i, 2i+1) rotate with their own table entries)
__device__ __forceinline__ uint4 dmvae_norm_rope8(const uint4 raw, float r, const float* __restrict__ w, const float* __restrict__ cosb,
                                            const float* __restrict__ sinb, int tok, int D, int d0) {
  const bf16x8 x = *reinterpret_cast<const bf16x8*>(&raw);
  const float4 w0 = *reinterpret_cast<const float4*>(w + d0), w1 = *reinterpret_cast<const float4*>(w + d0 + 4);
  const float4 c0 = *reinterpret_cast<const float4*>(cosb + (size_t)tok * D + d0), c1 = *reinterpret_cast<const float4*>(cosb + (size_t)tok * D + d0 + 4);
  const float4 s0 = *reinterpret_cast<const float4*>(sinb + (size_t)tok * D + d0), s1 = *reinterpret_cast<const float4*>(sinb + (size_t)tok * D + d0 + 4);
  const float wv[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
  const float cv[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
  const float sv[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
  float n[8];
#pragma unroll
  for (int e = 0; e < 8; e++) n[e] = (float)(bf16)((float)x[e] * r) * wv[e];
  uint4 o;
  o.x = dmvae_pack_bf16x2(n[0] * cv[0] - n[1] * sv[0], n[1] * cv[1] + n[0] * sv[1]);
  o.y = dmvae_pack_bf16x2(n[2] * cv[2] - n[3] * sv[2], n[3] * cv[3] + n[2] * sv[3]);
  o.z = dmvae_pack_bf16x2(n[4] * cv[4] - n[5] * sv[4], n[5] * cv[5] + n[4] * sv[5]);
  o.w = dmvae_pack_bf16x2(n[6] * cv[6] - n[7] * sv[6], n[7] * cv[7] + n[6] * sv[7]);
  return o;
}
__device__ __forceinline__ float dmvae_sumsq8(const uint4 raw) {
  const bf16x8 x = *reinterpret_cast<const bf16x8*>(&raw);
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 8; e++) s += (float)x[e] * (float)x[e];
  return s;
}

