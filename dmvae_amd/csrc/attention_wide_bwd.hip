// Streaming backward of the decoder AttnBlock's single-head attention at head dim 512 for gfx950 (MI355X): dq, dk, dv at ANY token count, the backward half of
// attention_wide.hip (reference: autograd of models/flux_ae.py:37-49 -- one head, d = C = 512, over the h * w tokens of the mid block).  functional.AttnBlockFn's
// composed backward rebuilds P with GEMMs and holds an f32 and a bf16 [n, S, S] score tensor, an f32 dP and a bf16 dS in HBM while it runs (12 S^2 bytes per sample);
// these two kernels walk 32-row tiles instead.  Nothing of size S x S reaches HBM; the only scratch is delta [B][S] f32.
//
//   P = exp(scale s - L)      dV = P^T dO      dP = dO V^T      dS = P o (dP - delta),  delta_q = sum_k P dP      dQ = scale dS K      dK = scale dS^T Q
//
// Operands: q, k, v, dout [B][S][512] bf16, token rows 512 elements apart (o, the forward's result, is part of the entry's signature and is not read: see delta
// below); lse [B][S] f32 = scale * max + log(sum) of a query's scaled scores (what attention_wide.hip writes); dq, dk, dv [B][S][512] bf16.
//
// Two passes on one stream, the two-orientation form of attention_bwd_stream.hip (S and dP are formed with the queries on the lanes AND with the keys on the lanes):
// every sum has a fixed order and everything is per sample -- no float atomics, no waiting between workgroups; reruns are bit-identical and a 2B-sample call equals
// two B-sample calls.
// Partition: attention_bwd_stream.hip's wave owns 32 rows x all channels; at 512 channels that is 128 registers of Q fragments, 128 of dO fragments and 256 of dQ
// accumulators before a single score.  Here a workgroup = 4 waves, ONE PER SIMD (launch bound 256), owns 32 rows, and wave w owns the channels 128 w .. 128 w + 127:
//   1. every wave forms the PARTIAL scores of its quarter -- S and dP of the tile's 32 x 32 block summed over its 128 channels, 8 + 8 MFMAs;
//   2. the four waves' partial blocks are exchanged through LDS (2 x 4 KiB per wave, written and read as 16-B pieces a lane apart: no bank conflict), one barrier;
//   3. every wave sums the four quarters in the order ((0 + 1) + 2) + 3 -- all four hold the same bits -- and forms p and scale * dS in registers;
//   4. every wave accumulates its own 128 channels of the gradient (v_mfma_f32_32x32x16_bf16 throughout).
// No product is computed by two waves.  Per wave and 32 x 32 block: query pass 16 (first walk) + 16 + 16 (dQ from hi and lo), key pass 16 + 8 (dV) + 16 (dK).
//   query pass (attention_wide_bwd_dq_kernel): 32 queries per workgroup, walks the ceil(S / 32) key tiles.  In registers for the whole walk: the wave's quarter of
//     the Q and dO fragments (2 x 32), L and delta of the lane's query, the dQ accumulators (4 x 16).  S^T = K Q^T and dP^T = V dO^T with the query on the lane.
//     TWO walks: the first forms delta_q = sum_k P dP in f32 (steps 1 - 3 only, no image; every wave the same sum in the same order: the same bits; written by
//     wave 0 for the key pass), the second dS^T -> bf16 A fragments (to_afrag) and dQ += dS K through the transpose read of K.
//   key pass (attention_wide_bwd_dkdv_kernel): 32 keys per workgroup (the wave's quarter of the K and V fragments, 2 x 32, and of the dK and dV accumulators,
//     2 x 4 x 16, in registers), walks the Q / dO tiles: S = Q K^T and dP = dO V^T with the KEY on the lane, so P^T and dS^T are the next products' A fragments by
//     the same swaps; dV += P^T dO and dK += dS^T Q through transpose reads of dO / Q.  L and delta of a tile's 32 queries travel with it.
// LDS (160 KiB per CU; a 32-row image at 512 channels is 32 KiB).  With this partition each byte of a row-read operand is read by exactly one wave, so the row
// fragments (K and V in the query pass, Q and dO in the key pass: the A operands of the partial products) are loaded from global memory STRAIGHT INTO REGISTERS,
// one tile ahead (16 x 16 B per lane, issued behind the partial products that consumed the previous ones; the four 32-B pieces of a 128-B line are asked for by four
// consecutive loads and come out of the vector L1).  Only the transposed reads need LDS: ds_read_b64_tr_b16 through attention_common.h's tr_off0<1024> / tr_frag<1024>
// on attention_wide.hip's wide_vslot layout.  Images are SINGLE-buffered: the walk has two barriers per tile anyway (A: everyone has left the previous tile's image and
// partials; B: the partials are complete), the next tile's image is carried in registers (wave w rows w, w + 4, ..., a lane one 16-B chunk: coalesced 1-KiB row
// loads) and written behind barrier A, read behind barrier B.
//   query pass: K transposed 32 KiB | exchange 32 KiB = 64 KiB dynamic.
//   key pass:   Q transposed 32 KiB | dO transposed 32 KiB | exchange 32 KiB | L [32], delta [32] 256 B = 96.25 KiB dynamic (opt-in).
// Rounding sites: q, k, v, dO are bf16 operands; scores and dP are accumulated in f32 on the matrix cores (per quarter, the quarters added in f32); p = exp(scale s - L)
// in f32; P is rounded to bf16 ONCE as the dV operand; dQ, dK, dV are accumulated in f32 and rounded to bf16 once at the store.  Two sites are FINER than
// attention_bwd_stream.hip's, because its two are not good enough at this width on ill-conditioned inputs (one head over every token: rows whose keys are nearly
// parallel, or one key with all the weight, leave dQ and dK as the small remainder of a cancelling sum, sum_k dS = 0):
//   delta is sum_k P dP in f32 from the kernel's own p and dP -- not dO . O on the saved bf16 O, whose rounding (2^-9 of |O| per channel) is an error in delta that
//     every dS of the row carries with weight P; with the kernel's own p the identity sum_k dS = 0 holds to f32 rounding.  Price: the query pass walks the keys twice.
//   scale * dS enters the matrix cores as hi + lo, hi = bf16(x), lo = bf16(x - hi) (2^-17 relative instead of 2^-9): two MFMAs per K^T / Q^T fragment.
// Measured on tests/test_gpu_attention_wide.py's rank-one directed inputs at S = 1025 / 1156 (rel-L2 of dq against float64): with the sibling's two sites 5.2e-2 /
// 5.7e-2 ('ascending') and 0.86 / 0.73 ('last'; dk 25 at S = 1025) -- the GEMM-composed backward, which has the same two sites, 3.2e-2 ... 0.58 --
// with these rel-L2 1.6e-03 ... 2.5e-03 over dq, dk and dv of all four cases (max-error / max <= 9.5e-03).
// Ragged S: rows >= S exist only in the last tile and are staged as zeros (the load takes row S - 1 instead: no branch, in bounds).  Query pass: a key >= S gets
// p = 0 by a select (its zero K row scores 0, not -inf).  Key pass: a query >= S travels with L = +inf and delta = 0, so p = exp(-inf) = 0 and dS = 0 exactly.
// Rows >= S of a workgroup's own block compute on zero fragments and are not stored.  All four waves of a workgroup own the SAME 32 rows, and with ceil(S / 32)
// workgroups per sample the first of them is live: no wave is ever idle, every wave passes the same two barriers per tile.
// Grid: one flat dimension of B * ceil(S / 32) workgroups through xcd_remap, both passes: the row blocks of one sample run on one XCD and share its L2.
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; no scratch and no spill in either):
//   query pass: 250 VGPRs,  96 AGPRs, 59 SGPRs, 64 KiB dynamic LDS; 1 wave per SIMD, one workgroup per CU.
//   key pass:   256 VGPRs, 184 AGPRs, 48 SGPRs, 96.25 KiB dynamic LDS; 1 wave per SIMD, one workgroup per CU.
#include "attention_common.h"
#include "dmvae_hip.h"

namespace dmvae_attn_wide_bwd {

constexpr int NT = 256;          // 4 waves, one per SIMD
constexpr int BR = 32;           // rows (queries / keys) a workgroup owns
constexpr int TR = 32;           // rows per streamed tile
constexpr int C = 512;           // channels = head dim
constexpr int ROW = C * 2;       // bytes per row in LDS
constexpr int TILE = TR * ROW;   // 32 KiB
constexpr int CW = C / (NT / 64);             // channels a wave owns: 128
constexpr int KS = CW / 16;      // 16-channel steps of a wave's partial products: 8
constexpr int DB = CW / 32;      // 32-channel blocks of a wave's accumulators: 4
constexpr int SW = TR * (ROW / 16) / NT;      // staging sweeps per image: 8 (a wave writes one whole row per sweep)
constexpr int XBLK = 64 * 16 * (int)sizeof(float);      // one wave's partial 32 x 32 block: 4 KiB
constexpr int XCH = (NT / 64) * 2 * XBLK;     // [wave][S | dP]: 32 KiB
constexpr int DQ_LDS = TILE + XCH;                                  // K transposed | exchange
constexpr int DKDV_LDS = 2 * TILE + XCH + 2 * TR * (int)sizeof(float);      // Q transposed | dO transposed | exchange | L [32] | delta [32]
static_assert(ROW / 16 == 64 && SW * (NT / 64) == TR, "a wave stages one row per sweep");

struct Args {
  const bf16 *q, *k, *v, *dout;          // [B][S][512]
  const float* lse;          // [B][S]
  bf16 *dq, *dk, *dv;        // [B][S][512]
  float* delta;              // [B][S]: written by the query pass, read by the key pass
  int S;
  int nb;                    // row blocks per sample: ceil(S / 32)
  float scale;
};

// attention_wide.hip's V image: byte offset of 16-B chunk c (0 .. 63) of row `key`, 64-B segment c >> 2 swizzled by key & 3 (what tr_off0<1024> / tr_frag<1024> read)
__device__ __forceinline__ int wide_vslot(int key, int c) { return key * ROW + (((c >> 2) ^ (key & 3)) << 6) + ((c & 3) << 4); }

// The exchange of the partial blocks: wave w's block `which` (0: S, 1: dP) as four 1-KiB planes, plane r4 = registers 4 r4 .. 4 r4 + 3 of every lane, 16 B a lane.
// All four waves hold the same 32 x 32 block position in the same register layout, so a lane reads its own element of every wave's block.
__device__ __forceinline__ void xch_put(char* x, int wave, int which, int lane, const f32x16& c) {
#pragma unroll
  for (int r4 = 0; r4 < 4; r4++)
    *reinterpret_cast<f32x4*>(x + (wave * 2 + which) * XBLK + r4 * 1024 + lane * 16) = f32x4{c[4 * r4], c[4 * r4 + 1], c[4 * r4 + 2], c[4 * r4 + 3]};
}
// the four quarters in the order ((0 + 1) + 2) + 3: the same bits in every wave
__device__ __forceinline__ f32x16 xch_sum(const char* x, int which, int lane) {
  f32x16 s;
#pragma unroll
  for (int r4 = 0; r4 < 4; r4++) {
    f32x4 t = *reinterpret_cast<const f32x4*>(x + which * XBLK + r4 * 1024 + lane * 16);
#pragma unroll
    for (int w = 1; w < NT / 64; w++) t = t + *reinterpret_cast<const f32x4*>(x + (w * 2 + which) * XBLK + r4 * 1024 + lane * 16);
    s[4 * r4] = t[0]; s[4 * r4 + 1] = t[1]; s[4 * r4 + 2] = t[2]; s[4 * r4 + 3] = t[3];
  }
  return s;
}
// 16 B of row min(row, S - 1) at element offset `col`, zeros for a row >= S
__device__ __forceinline__ uint4 load_row16(const bf16* p, int row, int S, int col) {
  const uint4 x = *reinterpret_cast<const uint4*>(p + (size_t)min(row, S - 1) * C + col);
  return row < S ? x : uint4{0, 0, 0, 0};
}

__global__ __launch_bounds__(NT) void attention_wide_bwd_dq_kernel(Args a) {
#if __HIP_DEVICE_COMPILE__
  extern __shared__ __attribute__((aligned(256))) char smem[];      // DQ_LDS
  char* kt = smem;
  char* xch = smem + TILE;
  const int S = a.S;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned item = xcd_remap(blockIdx.x, gridDim.x);
  const int b = (int)(item / (unsigned)a.nb), blk = (int)(item % (unsigned)a.nb);
  const size_t sample = (size_t)b * S * C;
  const bf16 *qp = a.q + sample, *kp = a.k + sample, *vp = a.v + sample, *dop = a.dout + sample;
  const int kg = lane >> 5, ql = lane & 31;
  const int q0 = blk * BR;                   // the workgroup's first query (< S)
  const int q = q0 + ql;
  const int cw = wave * CW;                  // the wave's first channel
  const int nt = (S + TR - 1) / TR;

  // the K^T image of the next tile: sweep `it` of wave w is row w + 4 it, lane = its 16-B chunk
  uint4 sreg[SW];
  auto load_image = [&](int t) {
#pragma unroll
    for (int it = 0; it < SW; it++) sreg[it] = load_row16(kp, t * TR + wave + it * (NT / 64), S, lane * 8);
  };
  auto store_image = [&]() {
#pragma unroll
    for (int it = 0; it < SW; it++) *reinterpret_cast<uint4*>(kt + wide_vslot(wave + it * (NT / 64), lane)) = sreg[it];
  };
  // the row fragments of the next tile's partial products: key ql of the tile, 8 channels per lane per 16-channel step of the wave's quarter
  uint4 kf[KS], vf[KS];
  auto load_rows = [&](int t) {
#pragma unroll
    for (int kk = 0; kk < KS; kk++) {
      kf[kk] = load_row16(kp, t * TR + ql, S, cw + kk * 16 + kg * 8);
      vf[kk] = load_row16(vp, t * TR + ql, S, cw + kk * 16 + kg * 8);
    }
  };
  load_rows(0);

  // the wave's quarter of the Q / dO fragments (column operands: query on the lane, 8 channels per lane per 16-channel step)
  uint4 qf[KS], dof[KS];
#pragma unroll
  for (int kk = 0; kk < KS; kk++) {
    qf[kk] = load_row16(qp, q, S, cw + kk * 16 + kg * 8);
    dof[kk] = load_row16(dop, q, S, cw + kk * 16 + kg * 8);
  }
  const float Lq = q < S ? a.lse[(size_t)b * S + q] : INFINITY;      // a padded query: every P of its column is 0
  const int toff = tr_off0<ROW>(lane);
  const float scale = a.scale;

  // st[r] = this quarter's part of score(key t*32 + (r&3) + 8 (r>>2) + 4 kg, query q), dpt likewise: the partial products of the tile whose row fragments are in
  // registers, into the exchange
  f32x16 st, dpt;
  auto partials = [&]() {
#pragma unroll
    for (int r = 0; r < 16; r++) { st[r] = 0.f; dpt[r] = 0.f; }
#pragma unroll
    for (int kk = 0; kk < KS; kk++) {
      st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<bf16x8*>(&kf[kk]), *reinterpret_cast<bf16x8*>(&qf[kk]), st, 0, 0, 0);
      dpt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<bf16x8*>(&vf[kk]), *reinterpret_cast<bf16x8*>(&dof[kk]), dpt, 0, 0, 0);
    }
    xch_put(xch, wave, 0, lane, st);
    xch_put(xch, wave, 1, lane, dpt);
  };
  // the four quarters summed, st -> p = exp(scale s - L), 0 for a key >= S (only the last tile has such keys)
  auto probabilities = [&](int t) {
    st = xch_sum(xch, 0, lane);
    dpt = xch_sum(xch, 1, lane);
    const int lim = S - t * TR - 4 * kg;      // keys of this lane's registers below lim are live
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const float p = __expf(st[r] * scale - Lq);
      st[r] = (r & 3) + 8 * (r >> 2) < lim ? p : 0.f;
    }
  };

  // ---- first walk: delta_q = sum_k P dP, in f32 and in a fixed order (the lane's 16 keys of every tile in turn, then the two halves of a query's keys) ----------
  float delta = 0.f;
  for (int t = 0; t < nt; t++) {
    __syncthreads();          // A: every wave has left tile t - 1's partial blocks
    partials();
    if (t + 1 < nt) load_rows(t + 1); else { load_image(0); load_rows(0); }      // in flight under the rest of the iteration; the last one fetches the second walk's tile 0
    __syncthreads();          // B: the four partial blocks are complete
    probabilities(t);
#pragma unroll
    for (int r = 0; r < 16; r++) delta = fmaf(st[r], dpt[r], delta);
  }
  delta = xhalf_sum(delta);   // the same bits in all four waves: the same instructions on the same exchanged blocks
  if (q < S && wave == 0 && kg == 0) a.delta[(size_t)b * S + q] = delta;

  // ---- second walk: dQ ----------------------------------------------------------------------------------------------------------------------------------
  f32x16 dq[DB];
#pragma unroll
  for (int db = 0; db < DB; db++)
#pragma unroll
    for (int r = 0; r < 16; r++) dq[db][r] = 0.f;

  for (int t = 0; t < nt; t++) {
    __syncthreads();          // A: every wave has left tile t - 1's image and partial blocks
    store_image();
    partials();
    if (t + 1 < nt) { load_image(t + 1); load_rows(t + 1); }      // in flight under the rest of the iteration
    __syncthreads();          // B: tile t's image and the four partial blocks are complete
    probabilities(t);
    // scale * dS as the sum of TWO bf16 values, hi = bf16(x) and lo = bf16(x - hi): two products on the same K^T fragments
    f32x16 lo;
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const float x = st[r] * (dpt[r] - delta) * scale;
      dpt[r] = x;
      lo[r] = x - (float)(bf16)x;
    }
    bf16x8 ah[2], al[2];
    to_afrag(dpt, ah);
    to_afrag(lo, al);
#pragma unroll
    for (int half = 0; half < 2; half++)
#pragma unroll
      for (int db = 0; db < DB; db++) {
        const bf16x8 ktr = tr_frag<ROW>(kt, half, toff, wave * DB + db);
        dq[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[half], ktr, dq[db], 0, 0, 0);
        dq[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[half], ktr, dq[db], 0, 0, 0);
      }
  }
  // registers r are queries q0 + (r&3) + 8 (r>>2) + 4 kg, the lane is channel cw + db*32 + ql: 32 lanes write 64 consecutive bytes of a row
  bf16* dqg = a.dq + sample + cw;
#pragma unroll
  for (int db = 0; db < DB; db++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int qo = q0 + (r & 3) + 8 * (r >> 2) + 4 * kg;
      if (qo < S) dqg[(size_t)qo * C + db * 32 + ql] = (bf16)dq[db][r];
    }
#endif
}

__global__ __launch_bounds__(NT) void attention_wide_bwd_dkdv_kernel(Args a) {
#if __HIP_DEVICE_COMPILE__
  extern __shared__ __attribute__((aligned(256))) char smem[];      // DKDV_LDS
  char* qt = smem;
  char* dt = smem + TILE;
  char* xch = smem + 2 * TILE;
  float* Ls = reinterpret_cast<float*>(smem + 2 * TILE + XCH);
  float* Ds = Ls + TR;
  const int S = a.S;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned item = xcd_remap(blockIdx.x, gridDim.x);
  const int b = (int)(item / (unsigned)a.nb), blk = (int)(item % (unsigned)a.nb);
  const size_t sample = (size_t)b * S * C;
  const bf16 *qp = a.q + sample, *kp = a.k + sample, *vp = a.v + sample, *dop = a.dout + sample;
  const float* lse = a.lse + (size_t)b * S;
  const float* dlt = a.delta + (size_t)b * S;
  const int kg = lane >> 5, ql = lane & 31;
  const int key0 = blk * BR;                 // the workgroup's first key (< S)
  const int key = key0 + ql;
  const int cw = wave * CW;                  // the wave's first channel
  const int nt = (S + TR - 1) / TR;

  // the Q^T and dO^T images of the next tile (sweep `it` of wave w is row w + 4 it, lane = its 16-B chunk); threads 0-31 its L, threads 32-63 its delta
  uint4 qreg[SW], dreg[SW];
  float sreg = 0.f;
  auto load_image = [&](int t) {
#pragma unroll
    for (int it = 0; it < SW; it++) {
      qreg[it] = load_row16(qp, t * TR + wave + it * (NT / 64), S, lane * 8);
      dreg[it] = load_row16(dop, t * TR + wave + it * (NT / 64), S, lane * 8);
    }
    if (tid < 2 * TR) {
      const int sq = t * TR + (tid & (TR - 1));
      const float x = tid < TR ? lse[min(sq, S - 1)] : dlt[min(sq, S - 1)];
      sreg = sq < S ? x : (tid < TR ? INFINITY : 0.f);      // a padded query: L = +inf, delta = 0 -> p = 0, dS = 0
    }
  };
  auto store_image = [&]() {
#pragma unroll
    for (int it = 0; it < SW; it++) {
      *reinterpret_cast<uint4*>(qt + wide_vslot(wave + it * (NT / 64), lane)) = qreg[it];
      *reinterpret_cast<uint4*>(dt + wide_vslot(wave + it * (NT / 64), lane)) = dreg[it];
    }
    if (tid < 2 * TR) Ls[tid] = sreg;      // Ds = Ls + 32
  };
  // the row fragments of the next tile's partial products: query ql of the tile, 8 channels per lane per 16-channel step of the wave's quarter
  uint4 qfr[KS], dor[KS];
  auto load_rows = [&](int t) {
#pragma unroll
    for (int kk = 0; kk < KS; kk++) {
      qfr[kk] = load_row16(qp, t * TR + ql, S, cw + kk * 16 + kg * 8);
      dor[kk] = load_row16(dop, t * TR + ql, S, cw + kk * 16 + kg * 8);
    }
  };
  load_image(0);
  load_rows(0);

  // the wave's quarter of the K / V fragments (column operands: key on the lane)
  uint4 kfb[KS], vfb[KS];
#pragma unroll
  for (int kk = 0; kk < KS; kk++) {
    kfb[kk] = load_row16(kp, key, S, cw + kk * 16 + kg * 8);
    vfb[kk] = load_row16(vp, key, S, cw + kk * 16 + kg * 8);
  }
  const int toff = tr_off0<ROW>(lane);
  const float scale = a.scale;

  f32x16 dk[DB], dv[DB];
#pragma unroll
  for (int db = 0; db < DB; db++)
#pragma unroll
    for (int r = 0; r < 16; r++) { dk[db][r] = 0.f; dv[db][r] = 0.f; }

  for (int t = 0; t < nt; t++) {
    __syncthreads();          // A: every wave has left tile t - 1's images, statistics and partial blocks
    store_image();
    // s[r] = this quarter's part of score(query t*32 + (r&3) + 8 (r>>2) + 4 kg, this lane's key), dp likewise
    f32x16 s, dp;
#pragma unroll
    for (int r = 0; r < 16; r++) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
    for (int kk = 0; kk < KS; kk++) {
      s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<bf16x8*>(&qfr[kk]), *reinterpret_cast<bf16x8*>(&kfb[kk]), s, 0, 0, 0);
      dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<bf16x8*>(&dor[kk]), *reinterpret_cast<bf16x8*>(&vfb[kk]), dp, 0, 0, 0);
    }
    xch_put(xch, wave, 0, lane, s);
    xch_put(xch, wave, 1, lane, dp);
    if (t + 1 < nt) { load_image(t + 1); load_rows(t + 1); }      // in flight under the rest of the iteration
    __syncthreads();          // B: tile t's images, statistics and the four partial blocks are complete
    s = xch_sum(xch, 0, lane);
    dp = xch_sum(xch, 1, lane);
    f32x16 lo;
#pragma unroll
    for (int r4 = 0; r4 < 4; r4++) {
      const f32x4 Lv = *reinterpret_cast<const f32x4*>(Ls + 8 * r4 + 4 * kg), Dv = *reinterpret_cast<const f32x4*>(Ds + 8 * r4 + 4 * kg);
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const float p = __expf(s[r4 * 4 + r] * scale - Lv[r]);
        const float x = p * (dp[r4 * 4 + r] - Dv[r]) * scale;
        s[r4 * 4 + r] = p;
        dp[r4 * 4 + r] = x;
        lo[r4 * 4 + r] = x - (float)(bf16)x;      // scale * dS = hi + lo, two bf16 values (as the query pass)
      }
    }
    bf16x8 pf[2], dsh[2], dsl[2];
    to_afrag(s, pf);
    to_afrag(dp, dsh);
    to_afrag(lo, dsl);
#pragma unroll
    for (int half = 0; half < 2; half++)
#pragma unroll
      for (int db = 0; db < DB; db++) {
        dv[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pf[half], tr_frag<ROW>(dt, half, toff, wave * DB + db), dv[db], 0, 0, 0);
        const bf16x8 qtr = tr_frag<ROW>(qt, half, toff, wave * DB + db);
        dk[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dsh[half], qtr, dk[db], 0, 0, 0);
        dk[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dsl[half], qtr, dk[db], 0, 0, 0);
      }
  }
  // registers r are keys key0 + (r&3) + 8 (r>>2) + 4 kg, the lane is channel cw + db*32 + ql
  bf16* dkg = a.dk + sample + cw;
  bf16* dvg = a.dv + sample + cw;
#pragma unroll
  for (int db = 0; db < DB; db++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int ko = key0 + (r & 3) + 8 * (r >> 2) + 4 * kg;
      if (ko < S) {
        dkg[(size_t)ko * C + db * 32 + ql] = (bf16)dk[db][r];
        dvg[(size_t)ko * C + db * 32 + ql] = (bf16)dv[db][r];
      }
    }
#endif
}

}  // namespace dmvae_attn_wide_bwd

extern "C" int dmvae_attention_wide_bwd_stream_bf16(const void* q, const void* k, const void* v, const void* o, const void* dout, const void* lse, void* dq, void* dk,
                                                    void* dv, void* delta, int batch, int seq, int channels, float scale, hipStream_t stream) {
  using namespace dmvae_attn_wide_bwd;
  static const char* name = "attention_wide_bwd_stream_bf16";
  DMVAE_CHECK_ARG(q && k && v && o && dout && dq && dk && dv, "%s: null q, k, v, o, dout, dq, dk or dv", name);
  DMVAE_CHECK_ARG(lse, "%s: null lse (the forward's row statistics are required)", name);
  DMVAE_CHECK_ARG(delta, "%s: null delta scratch (batch * seq floats)", name);
  DMVAE_CHECK_ARG(batch >= 1 && seq >= 1, "%s: needs batch, seq >= 1 (got %d, %d)", name, batch, seq);
  DMVAE_CHECK_ARG(channels == C, "%s: needs channels %d (got %d)", name, C, channels);
  DMVAE_CHECK_ARG(scale > 0.f && isfinite(scale), "%s: needs a finite scale > 0 (got %g)", name, (double)scale);
  const int nb = attn_row_blocks(seq, BR);      // both passes: 32 rows per workgroup
  DMVAE_CHECK_ARG((long long)batch * nb <= 0x7fffffffLL, "%s: %d x %d tokens does not fit the grid", name, batch, seq);
  Args a = {};
  a.q = (const bf16*)q; a.k = (const bf16*)k; a.v = (const bf16*)v; a.dout = (const bf16*)dout; a.lse = (const float*)lse;
  a.dq = (bf16*)dq; a.dk = (bf16*)dk; a.dv = (bf16*)dv; a.delta = (float*)delta;
  a.S = seq; a.nb = nb; a.scale = scale;
  const dim3 grid((unsigned)(batch * nb));
  DMVAE_LDS_OPTIN(DQ_LDS, attention_wide_bwd_dq_kernel);
  DMVAE_LDS_OPTIN(DKDV_LDS, attention_wide_bwd_dkdv_kernel);
  hipLaunchKernelGGL(attention_wide_bwd_dq_kernel, grid, dim3(NT), DQ_LDS, stream, a);
  DMVAE_CHECK_LAUNCH();
  hipLaunchKernelGGL(attention_wide_bwd_dkdv_kernel, grid, dim3(NT), DKDV_LDS, stream, a);
  DMVAE_CHECK_LAUNCH();
  return 0;
}
