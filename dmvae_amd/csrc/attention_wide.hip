// Streaming-softmax single-head self-attention forward at head dim 512 for gfx950 (MI355X): the decoder AttnBlock's attention at ANY token count (reference:
// models/flux_ae.py:37-49 -- one head, d = C = 512, over the h * w tokens of the mid block, twice the latent grid each way: 288 px is 36 x 36 = 1296, 512 px 64 x 64 = 4096).
// functional.AttnBlockFn composes the attention from GEMMs (gemm_nt -> softmax_rows -> gemm_nt) with an f32 and a bf16 [n, S, S] tensor in HBM; this kernel walks 32-key
// tiles with an online softmax instead.  Nothing of size S x S reaches HBM.  attention_stream.hip's template stops at a staged head dim of 96 (Q and O of a wave's 32
// queries in registers beside 64-key tiles); at 512 channels the same structure needs the whole unified register file of a SIMD for one wave, hence a file of its own.
//
// Operands: q, k, v [B][S][512] bf16, three pointers, token rows 512 elements apart (the three 1x1 conv outputs of AttnBlockFn viewed [n, s, c]); out [B][S][512] bf16;
// optional lse [B][S] f32 = scale * max + log(sum) of a query's scaled scores (natural log, the definition of attention_stream.hip): what the streaming backward,
// attention_wide_bwd.hip, rebuilds P from -- functional.AttnBlockFn asks for it whenever that backward will run; the out bits are the same with and without it.
//
// Structure: a workgroup = 4 waves, ONE PER SIMD (launch bound 256: a wave may take the unified 512-register file), owns 64 consecutive queries of one sample and walks
// the ceil(S / 32) key tiles.  Two waves share 32 queries: both compute the same scores and the same softmax (the same instructions on the same data, so the same bits),
// and each accumulates ONE HALF of the 512 output channels.  Per wave, in registers for the whole walk: the Q fragments (32 sixteen-channel steps x bf16x8 = 128
// registers), the f32 accumulators of its 256 channels (8 thirty-two-channel blocks x f32x16 = 128 registers), the running maximum m of the RAW scores and the running
// sum l.  Why not 32 queries x 512 channels per wave: with more than 256 registers a kernel's MFMA results live in the 256 accumulation registers, the sixteen blocks of a
// whole row would fill them, and the score block needs sixteen more -- that form compiled to 298 ... 544 spilled registers; this one to none.  Its price is that q k^T is
// computed twice (48 MFMAs per wave and tile instead of 32 + 32 for twice the channels: 1.5 x the matrix work and LDS reads per query).
// A K tile (32 keys x 1024 B, 16-B chunks XOR-swizzled by key & 15: att_kslot<1024>) and a V tile (32 x 1024 B in the image the transpose read ds_read_b64_tr_b16 wants:
// the sixteen 64-B segments of a row swizzled by key & 3 -- wide_vslot, read by attention_common.h's tr_off0<1024> / tr_frag<1024>) are double-buffered in LDS:
// 2 x 2 x 32 KiB = 128 KiB dynamic (opt-in attribute).  Conflict rules of attention_common.h: the rows are 0 mod 256 B, so the sixteen lanes of a ds_read_b128 group
// (keys whose low four bits are all different) land in sixteen distinct 16-B slots, and the four key rows of a transpose-read pass in four distinct 64-B slots.
// Register staging in two sweeps so that K and V share the staging registers (8 x 16 B per thread; wave w carries rows w, w + 4, ... of a tile, a lane one chunk): the
// next K tile's loads are issued at the head of the iteration, land under q k^T and are written to the OTHER buffer behind the softmax; the next V tile's loads are issued
// there, land under the PV products and are written at the end.  Both writes are behind the barrier at the head of the iteration, which says that every wave has left that
// buffer.  One barrier per tile.
//
// Products (as attention_stream.hip): S^T = K Q^T, so a lane owns ONE query -- (lane & 31) of the wave's 32 -- and 16 of the tile's 32 scores (the other 16 sit in
// lane ^ 32); O^T = V^T P^T keeps the query in the lane: rescale and 1 / l are in-lane, a lane stores 4 consecutive channels.  One MFMA opcode throughout
// (v_mfma_f32_32x32x16_bf16): per wave and tile 32 for q k^T and 16 for its half of PV.
// Rounding sites (those of attention_stream.hip): bf16 operands; scores accumulated in f32 on the matrix cores; p = 2^(s * ec - m * ec), ec = scale * log2(e), in f32;
// the row sum l from the f32 p in a fixed order; p rounded to bf16 ONCE as the PV operand; O accumulated in f32, multiplied by 1 / l at the end and rounded once.
// Always rescale: no deferred-max threshold.
// Ragged S: keys >= S exist only in the last tile, are staged as zero rows and score -inf (p = 0 exactly); with ceil(S / 32) tiles every tile holds a live key, so every
// tile's maximum is finite.  Queries >= S compute on zero fragments and are not stored.  A wave whose 32 queries are all >= S only stages and synchronises (its own loop: the
// same sweeps and the same one barrier per tile; the wave index is read into a scalar register, so the choice is a scalar branch).
// Determinism: every reduction has a fixed order and everything is per sample: reruns are bit-identical, a 2B-sample call equals two B-sample calls.
// Grid: one flat dimension of B * ceil(S / 64) workgroups through xcd_remap: the query blocks of one sample run on one XCD and share its L2 for K / V.
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): 256 VGPRs, 249 AGPRs, 72 SGPRs, no scratch, no spill, 128 KiB dynamic LDS,
// 1 wave per SIMD, one workgroup per CU.
#include "attention_common.h"

namespace dmvae_attn_wide {

constexpr int NT = 256;          // 4 waves, one per SIMD
constexpr int QW = 32;           // queries per wave
constexpr int QB = QW * NT / 128; // queries per workgroup: 64 (two waves share 32 queries, each owns half the output channels)
constexpr int KT = 32;           // keys per tile
constexpr int C = 512;           // channels = head dim
constexpr int ROW = C * 2;       // bytes per row in LDS
constexpr int TILE = KT * ROW;   // 32 KiB
constexpr int KS = C / 16;       // 16-channel steps of q k^T
constexpr int DB = C / 64;       // 32-channel blocks of a wave's accumulators: its half of the channels
constexpr int SW = KT * (ROW / 16) / NT;      // staging sweeps per tile: 8 (a wave writes one whole row per sweep)
constexpr int KG = 4;           // K fragments read ahead of their products
constexpr int LDS_BYTES = 2 * 2 * TILE;       // [buffer][K | V]
static_assert(ROW / 16 == 64 && SW * (NT / 64) == KT, "a wave stages one row per sweep");

struct WideArgs {
  const bf16 *q, *k, *v;      // [B][S][512]
  bf16* out;
  float* lse;      // optional [B][S]
  int S;
  int nqb;         // query blocks per sample: ceil(S / 64)
  float scale;
};

// V image, byte offset of 16-B chunk c (0 .. 63) of row `key`: 64-B segment c >> 2 swizzled by key & 3, slot c & 3 inside it (att_vslot's 256-B rule on a 1024-B row)
__device__ __forceinline__ int wide_vslot(int key, int c) { return key * ROW + (((c >> 2) ^ (key & 3)) << 6) + ((c & 3) << 4); }

__global__ __launch_bounds__(NT) void attention_wide_kernel(WideArgs a) {
#if __HIP_DEVICE_COMPILE__
  extern __shared__ __attribute__((aligned(256))) char smem[];      // LDS_BYTES
  const int S = a.S;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // the wave index in a scalar register: `live` is a scalar branch
  const unsigned item = xcd_remap(blockIdx.x, gridDim.x);
  const int b = (int)(item / (unsigned)a.nqb), qblk = (int)(item % (unsigned)a.nqb);
  const size_t sample = (size_t)b * S * C;
  const bf16* qp = a.q + sample;
  const bf16* kp = a.k + sample;
  const bf16* vp = a.v + sample;
  const int kg = lane >> 5, ql = lane & 31;
  const int ch = wave & 1;                   // the wave's half of the output channels: 32-channel blocks ch * 8 .. ch * 8 + 7
  const int q0 = qblk * QB + (wave >> 1) * QW;      // the wave's first query
  const int q = q0 + ql;
  const bool live = q0 < S;                  // wave-uniform

  // staging: sweep `it` of wave w is row w + 4 it of the tile, lane = its 16-B chunk; rows >= S are zeros (the load takes row S - 1 instead: no branch, in bounds)
  uint4 sreg[SW];
  auto load_rows = [&](const bf16* p, int t) {
#pragma unroll
    for (int it = 0; it < SW; it++) {
      const int key = t * KT + wave + it * (NT / 64);
      const uint4 x = *reinterpret_cast<const uint4*>(p + (size_t)min(key, S - 1) * C + lane * 8);
      sreg[it] = key < S ? x : uint4{0, 0, 0, 0};
    }
  };
  auto store_k = [&](int buf) {
#pragma unroll
    for (int it = 0; it < SW; it++) *reinterpret_cast<uint4*>(smem + buf * 2 * TILE + att_kslot<ROW>(wave + it * (NT / 64), lane)) = sreg[it];
  };
  auto store_v = [&](int buf) {
#pragma unroll
    for (int it = 0; it < SW; it++) *reinterpret_cast<uint4*>(smem + buf * 2 * TILE + TILE + wide_vslot(wave + it * (NT / 64), lane)) = sreg[it];
  };
  load_rows(kp, 0);
  store_k(0);
  load_rows(vp, 0);

  // Q fragments (column operand of the swapped product): 8 channels per lane per 16-channel step
  bf16x8 qf[KS];
#pragma unroll
  for (int kk = 0; kk < KS; kk++) {
    uint4 t = *reinterpret_cast<const uint4*>(qp + (size_t)min(q, S - 1) * C + kk * 16 + kg * 8);
    if (q >= S) t = uint4{0, 0, 0, 0};
    qf[kk] = *reinterpret_cast<bf16x8*>(&t);
  }
  const int voff0 = tr_off0<ROW>(lane);
  store_v(0);
  const int nt = (S + KT - 1) / KT;
  if (!live) {      // stage and synchronise only: the same sweeps and the same barrier per tile as the live waves below
    for (int t = 0; t < nt; t++) {
      __syncthreads();
      if (t + 1 < nt) { load_rows(kp, t + 1); store_k((t + 1) & 1); load_rows(vp, t + 1); store_v((t + 1) & 1); }
    }
    return;
  }

  const float ec = a.scale * 1.4426950408889634f;     // scale > 0 (checked on the host): the maximum of the raw scores is the maximum of the scaled ones
  float m = -INFINITY, l = 0.f;
  f32x16 o[DB];
#pragma unroll
  for (int db = 0; db < DB; db++)
#pragma unroll
    for (int r = 0; r < 16; r++) o[db][r] = 0.f;

  for (int t = 0; t < nt; t++) {
    __syncthreads();          // tile t's image is complete, and every wave has left tile t - 1's buffer (the one this iteration refills)
    const char* ks = smem + (t & 1) * 2 * TILE;
    const char* vs = ks + TILE;
    const bool more = t + 1 < nt;
    if (more) load_rows(kp, t + 1);      // in flight under q k^T
    f32x16 st;                           // st[r] = score(key = t*32 + (r&3) + 8*(r>>2) + 4*kg, query q), then its p
#pragma unroll
    for (int r = 0; r < 16; r++) st[r] = 0.f;
#pragma unroll
    for (int g = 0; g < KS / KG; g++) {   // KG fragment reads ahead of their KG products
      bf16x8 kf[KG];
#pragma unroll
      for (int j = 0; j < KG; j++) kf[j] = *reinterpret_cast<const bf16x8*>(ks + att_kslot<ROW>(ql, (g * KG + j) * 2 + kg));
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < KG; j++) st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[j], qf[g * KG + j], st, 0, 0, 0);
    }
    if (t * KT + KT > S) {             // the last tile of a ragged S
      const int lim = S - t * KT - 4 * kg;
#pragma unroll
      for (int r = 0; r < 16; r++) st[r] = (r & 3) + 8 * (r >> 2) < lim ? st[r] : -INFINITY;
    }
    // ---- online softmax: the tile's maximum (finite: a tile holds a live key), the factor for what is accumulated at the old maximum ------------------------
    float tm = st[0];
#pragma unroll
    for (int r = 1; r < 16; r++) tm = fmaxf(tm, st[r]);
    const float mn = fmaxf(m, xhalf_max(tm));
    const float alpha = __builtin_amdgcn_exp2f((m - mn) * ec);      // first tile: 2^(-inf) = 0
    const float emc = mn * ec;
    m = mn;
    l *= alpha;
#pragma unroll
    for (int db = 0; db < DB; db++)
#pragma unroll
      for (int r = 0; r < 16; r++) o[db][r] *= alpha;
#pragma unroll
    for (int r = 0; r < 16; r++) { st[r] = __builtin_amdgcn_exp2f(fmaf(st[r], ec, -emc)); l += st[r]; }
    if (more) { store_k((t + 1) & 1); load_rows(vp, t + 1); }      // the V loads land under the PV products
    bf16x8 pa[2];                               // p rounded to bf16: the column operands of the tile's two 16-key steps
    to_afrag(st, pa);
#pragma unroll
    for (int half = 0; half < 2; half++) {
#pragma unroll
      for (int g = 0; g < DB / 4; g++) {        // four V^T fragments ahead of their four products
        bf16x8 vf[4];
#pragma unroll
        for (int j = 0; j < 4; j++) vf[j] = tr_frag<ROW>(vs, half, voff0, ch * DB + g * 4 + j);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 4; j++) o[g * 4 + j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[j], pa[half], o[g * 4 + j], 0, 0, 0);
      }
    }
    if (more) store_v((t + 1) & 1);      // behind this iteration's barrier: nobody reads that buffer any more; visible behind the next one
  }
  l = xhalf_sum(l);                      // the two halves of the query's keys: the same bits in both lanes
  const float inv = 1.f / l;
  if (q < S) {
    if (a.lse && kg == 0 && ch == 0) a.lse[(size_t)b * S + q] = m * a.scale + __logf(l);
    // lane = query q; registers r = 4 r4 .. 4 r4 + 3 are channels db*32 + 8 r4 + 4 kg + 0..3: 8-byte stores
    bf16* orow = a.out + sample + (size_t)q * C + ch * (C / 2);
#pragma unroll
    for (int db = 0; db < DB; db++)
#pragma unroll
      for (int r4 = 0; r4 < 4; r4++) {
        uint2 pk;
        pk.x = dmvae_pack_bf16x2(o[db][4 * r4 + 0] * inv, o[db][4 * r4 + 1] * inv);
        pk.y = dmvae_pack_bf16x2(o[db][4 * r4 + 2] * inv, o[db][4 * r4 + 3] * inv);
        *reinterpret_cast<uint2*>(orow + db * 32 + 8 * r4 + 4 * kg) = pk;
      }
  }
#endif
}

}  // namespace dmvae_attn_wide

extern "C" int dmvae_attention_wide_stream_bf16(const void* q, const void* k, const void* v, void* out, void* lse, int batch, int seq, int channels, float scale,
                                                hipStream_t stream) {
  using namespace dmvae_attn_wide;
  static const char* name = "attention_wide_stream_bf16";
  DMVAE_CHECK_ARG(q && k && v && out, "%s: null q, k, v or out", name);
  DMVAE_CHECK_ARG(batch >= 1 && seq >= 1, "%s: needs batch, seq >= 1 (got %d, %d)", name, batch, seq);
  DMVAE_CHECK_ARG(channels == C, "%s: needs channels %d (got %d)", name, C, channels);
  DMVAE_CHECK_ARG(scale > 0.f && isfinite(scale), "%s: needs a finite scale > 0 (got %g)", name, (double)scale);
  const int nqb = attn_row_blocks(seq, QB);
  DMVAE_CHECK_ARG((long long)batch * nqb <= 0x7fffffffLL, "%s: %d x %d tokens does not fit the grid", name, batch, seq);
  WideArgs a = {};
  a.q = (const bf16*)q; a.k = (const bf16*)k; a.v = (const bf16*)v; a.out = (bf16*)out; a.lse = (float*)lse;
  a.S = seq; a.nqb = nqb; a.scale = scale;
  DMVAE_LDS_OPTIN(LDS_BYTES, attention_wide_kernel);
  hipLaunchKernelGGL(attention_wide_kernel, dim3((unsigned)(batch * nqb)), dim3(NT), LDS_BYTES, stream, a);
  DMVAE_CHECK_LAUNCH();
  return 0;
}
