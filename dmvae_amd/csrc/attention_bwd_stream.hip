// Streaming backward of the encoder's multi-head self-attention for gfx950 (MI355X): d(qkv) at ANY token count, the backward half of attention_stream.hip (reference:
// autograd of models/dino_layers/attention.py:56-69 where the encoder trains, train_dmd.py:349,519, at the token counts models/vae.py:38-50 reaches: 577, 1025).
// csrc/attention_bwd.hip keeps a whole head's operands resident in LDS and stops at 288 tokens; these two kernels walk 64-row tiles instead.  Nothing of size S x S
// reaches HBM; the only scratch is delta [B*H][S] f32.
//
//   P = exp(scale s - L)      dV = P^T dO      dP = dO V^T      dS = P o (dP - delta),  delta_q = dO_q . O_q      dQ = scale dS K      dK = scale dS^T Q
//
// Operands: qkv [B][S][3][H][64] bf16 (the qkv Linear's output), out / dout [B][S][H*64] bf16, lse [B*H][S] f32 = scale * max + log(sum) of a query's scaled scores
// (what attention_stream.hip and vit.hip write), dqkv in qkv's layout.
//
// Two passes on one stream, the two-orientation form of attention_bwd.hip (seven S x S x 64 contractions instead of five: S and dP are formed with the queries on the
// lanes AND with the keys on the lanes).  The alternatives sum dQ across workgroups -- float atomics (no fixed order) or an ordered hand-off between resident workgroups
// (inter-workgroup waiting) -- and are not taken: every sum here has a fixed order and every operation is per (sample, head), so reruns are bit-identical and a
// 2B-sample call equals two B-sample calls.
//   query pass (attention_bwd_stream_dq_kernel): a workgroup = 8 waves owns 256 consecutive queries of one (sample, head), 32 per wave, and walks the ceil(S / 64) key
//     tiles.  In registers for the whole walk: the wave's Q and dO fragments, L and delta of the lane's query, the dQ accumulators (2 x 16).  Per 32-key block:
//     S^T = K Q^T and dP^T = V dO^T with the query on the lane, dS^T -> bf16 A fragments by two v_permlane32_swap per 16 keys (to_afrag), dQ += dS K through the
//     transpose read of K.  Writes delta for the second pass.
//   key pass (attention_bwd_stream_dkdv_kernel): a workgroup owns 256 keys, 32 per wave (K / V fragments and the dK / dV accumulators, 4 x 16, in registers), and walks
//     the Q / dO tiles: S = Q K^T and dP = dO V^T with the KEY on the lane, so P^T and dS^T are the next products' A fragments by the same swaps -- no LDS transpose;
//     dV += P^T dO and dK += dS^T Q through transpose reads of dO / Q.  L and delta of a tile's 64 queries travel with it.
// Tile walk as attention_stream.hip: tiles double-buffered in LDS through register staging (every thread carries one 16-B piece of each of the next tile's two operands,
// loaded behind the first block's products, written to the OTHER buffer at the end of the iteration), one barrier per tile, one flat grid through xcd_remap so that
// the blocks of one head share an XCD's L2.  An operand that is read by rows AND transposed is staged twice, once per layout of common.h (att_kslot: conflict-free
// ds_read_b128 rows; att_vslot: ds_read_b64_tr_b16): query pass K rows | K transposed | V rows = 24 KiB per buffer, 48 KiB static; key pass Q rows | Q transposed |
// dO rows | dO transposed | L, delta = 32.5 KiB per buffer, 65 KiB dynamic (opt-in).
//
// Rounding sites (attention_bwd.hip's lse kernels): q, k, v, dO, O are bf16 operands; delta is an f32 sum of products of the bf16 dO and the saved bf16 O; scores and dP
// are accumulated in f32 on the matrix cores; p = exp(scale s - L) in f32; P and scale * dS are rounded to bf16 ONCE as MFMA operands; dQ, dK, dV are accumulated in f32
// and rounded to bf16 once at the store.
// Ragged S: rows >= S exist only in the last tile and are staged as zeros.  Query pass: a key >= S gets p = 0 by a select (its zero K row scores 0, not -inf).  Key
// pass: a query >= S is staged with L = +inf and delta = 0, so p = exp(-inf) = 0 and dS = 0 exactly: it contributes nothing to dK / dV.  Queries / keys >= S of a
// workgroup's own block compute on zero fragments and are not stored; a wave whose 32 rows are all >= S only stages and synchronises; a 32-row block of the last tile
// that lies wholly past S is skipped.
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): query pass 159 VGPRs, 0 AGPRs, 44 SGPRs, no scratch, no spill,
// 48 KiB LDS; key pass 238 VGPRs, 0 AGPRs, 48 SGPRs, no scratch, no spill, 65 KiB LDS.  Both run two waves per SIMD (one 8-wave workgroup of the key pass, LDS-bound;
// the query pass fits three workgroups' LDS but two workgroups' registers).
#include "common.h"
#include "dmvae_hip.h"
#include <math.h>

namespace dmvae_attn_bwd_stream {

constexpr int D = 64;            // head dim
constexpr int NT = 512;          // 8 waves
constexpr int BW = 32;           // rows (queries / keys) a wave owns
constexpr int BB = BW * NT / 64; // rows a workgroup owns: 256
constexpr int TT = 64;           // rows per streamed tile
constexpr int ROW = 128;         // bytes per row in LDS
constexpr int TILE = TT * ROW;   // 8 KiB
constexpr int DQ_BUF = 3 * TILE;                                    // K rows | K transposed | V rows
constexpr int DKDV_BUF = 4 * TILE + 2 * TT * (int)sizeof(float);    // Q rows | Q transposed | dO rows | dO transposed | L [64] | delta [64]

struct Args {
  const bf16 *q, *k, *v;     // qkv, qkv + C, qkv + 2 C: per (sample, head) base + b * bs + h * 64, token rows rs elements apart
  const bf16 *o, *dout;      // [B][S][C]
  bf16 *dq, *dk, *dv;        // dqkv in the same geometry
  const float* lse;          // [B * H][S]
  float* delta;              // [B * H][S]: written by the query pass, read by the key pass
  long long bs;              // elements between samples: S * 3 C
  int rs;                    // 3 C
  int S, H;
  int nb;                    // 256-row blocks per (sample, head)
  float scale;
};

// transpose-read addressing in an att_vslot image (as attention_stream.hip): the lane supplies 4 channels of row 8 kg + rr (and + 4) of a 16-row step; channel block
// db is the 64-B segment db ^ swizzle: offset ^ (db << 6)
__device__ __forceinline__ int tr_off0(int lane) {
  const int kg = lane >> 5, g16 = (lane >> 4) & 1, rr = (lane & 15) >> 2, qq = lane & 3;
  return (kg * 8 + rr) * ROW + (((rr >> 1) & 1) << 6) + (16 * g16 + 4 * qq) * 2;
}
__device__ __forceinline__ bf16x8 tr_frag(const char* img, int step16, int off0, int db) {
  union { bf16x8 v; s16x4 hlf[2]; } f;
  f.hlf[0] = tr_read_ordered(img + step16 * (16 * ROW) + (off0 ^ (db << 6)));
  f.hlf[1] = tr_read_ordered(img + step16 * (16 * ROW) + (off0 ^ (db << 6)) + 4 * ROW);
  return f.v;
}

__global__ __launch_bounds__(NT) void attention_bwd_stream_dq_kernel(Args a) {
#if __HIP_DEVICE_COMPILE__
  __shared__ __attribute__((aligned(256))) char smem[2 * DQ_BUF];
  const int S = a.S, C = a.H * D;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned item = xcd_remap(blockIdx.x, gridDim.x);
  const int bh = (int)(item / (unsigned)a.nb), blk = (int)(item % (unsigned)a.nb);
  const int b = bh / a.H, h = bh % a.H;
  const size_t base = (size_t)b * a.bs + h * D;
  const bf16 *qp = a.q + base, *kp = a.k + base, *vp = a.v + base;
  const bf16* og = a.o + (size_t)b * S * C + h * D;
  const bf16* dog = a.dout + (size_t)b * S * C + h * D;
  const int kg = lane >> 5, ql = lane & 31;
  const int q0 = blk * BB + wave * BW;       // the wave's first query
  const int q = q0 + ql;
  const bool live = q0 < S;                  // wave-uniform
  const int nt = (S + TT - 1) / TT;

  // staging: thread -> key row tid >> 3 of the tile, 16-B chunk tid & 7 of its K row and of its V row
  const int skey = tid >> 3, sc = tid & 7;
  const int rsl = att_kslot<ROW>(skey, sc), tsl = att_vslot<ROW>(skey, sc);
  uint4 kreg, vreg;
  auto load_tile = [&](int t) {
    const int key = t * TT + skey;
    kreg = uint4{0, 0, 0, 0}; vreg = uint4{0, 0, 0, 0};
    if (key < S) {
      kreg = *reinterpret_cast<const uint4*>(kp + (size_t)key * a.rs + sc * 8);
      vreg = *reinterpret_cast<const uint4*>(vp + (size_t)key * a.rs + sc * 8);
    }
  };
  auto store_tile = [&](int buf) {
    char* img = smem + buf * DQ_BUF;
    *reinterpret_cast<uint4*>(img + rsl) = kreg;
    *reinterpret_cast<uint4*>(img + TILE + tsl) = kreg;
    *reinterpret_cast<uint4*>(img + 2 * TILE + rsl) = vreg;
  };
  load_tile(0);

  // the wave's Q / dO fragments (column operands: query on the lane, 8 channels per lane per 16-channel step) and delta
  bf16x8 qf[4], dof[4];
  float delta = 0.f;
#pragma unroll
  for (int kk = 0; kk < 4; kk++) {
    uint4 tq = {0, 0, 0, 0}, td = {0, 0, 0, 0}, to = {0, 0, 0, 0};
    const int d0 = kk * 16 + kg * 8;
    if (q < S) {
      tq = *reinterpret_cast<const uint4*>(qp + (size_t)q * a.rs + d0);
      td = *reinterpret_cast<const uint4*>(dog + (size_t)q * C + d0);
      to = *reinterpret_cast<const uint4*>(og + (size_t)q * C + d0);
    }
    qf[kk] = *reinterpret_cast<bf16x8*>(&tq);
    dof[kk] = *reinterpret_cast<bf16x8*>(&td);
    delta += dot8(td, to);
  }
  delta += __shfl_xor(delta, 32, 64);
  float Lq = INFINITY;                      // a padded query: every P of its column is 0
  if (q < S) {
    Lq = a.lse[(size_t)bh * S + q];
    if (kg == 0) a.delta[(size_t)bh * S + q] = delta;
  }
  const int toff = tr_off0(lane);
  const float scale = a.scale;
  store_tile(0);

  f32x16 dq[2];
#pragma unroll
  for (int db = 0; db < 2; db++)
#pragma unroll
    for (int r = 0; r < 16; r++) dq[db][r] = 0.f;

  for (int t = 0; t < nt; t++) {
    __syncthreads();          // tile t's images are complete, and every wave has left tile t - 1's buffer (the one this iteration refills)
    const char* ks = smem + (t & 1) * DQ_BUF;
    const char* kt = ks + TILE;
    const char* vs = ks + 2 * TILE;
    const bool more = t + 1 < nt;
    if (live) {
#pragma unroll
      for (int kb = 0; kb < 2; kb++) {
        const int key0 = t * TT + kb * 32;
        if (kb == 1 && key0 >= S) break;      // the last tile's second block wholly past S (wave-uniform)
        // st[r] = score(key key0 + (r&3) + 8 (r>>2) + 4 kg, query q), dpt likewise: every row fragment of the block ahead of its products
        bf16x8 kf[4], vf[4];
#pragma unroll
        for (int kk = 0; kk < 4; kk++) {
          const int off = att_kslot<ROW>(kb * 32 + ql, kk * 2 + kg);
          kf[kk] = *reinterpret_cast<const bf16x8*>(ks + off);
          vf[kk] = *reinterpret_cast<const bf16x8*>(vs + off);
        }
        __builtin_amdgcn_sched_barrier(0);
        f32x16 st, dpt;
#pragma unroll
        for (int r = 0; r < 16; r++) { st[r] = 0.f; dpt[r] = 0.f; }
#pragma unroll
        for (int kk = 0; kk < 4; kk++) {
          st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[kk], qf[kk], st, 0, 0, 0);
          dpt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[kk], dof[kk], dpt, 0, 0, 0);
        }
        // behind the products: the K^T fragments of the dQ product (they land under the exponentials), and the next tile's global loads
        bf16x8 ktr[2][2];
#pragma unroll
        for (int half = 0; half < 2; half++)
#pragma unroll
          for (int db = 0; db < 2; db++) ktr[half][db] = tr_frag(kt, kb * 2 + half, toff, db);
        if (kb == 0 && more) load_tile(t + 1);
        __builtin_amdgcn_sched_barrier(0);
        if (key0 + 32 > S) {      // only the last live block can hold keys past S: a wave-uniform branch
#pragma unroll
          for (int r = 0; r < 16; r++) {
            float p = __expf(st[r] * scale - Lq);
            if (key0 + (r & 3) + 8 * (r >> 2) + 4 * kg >= S) p = 0.f;
            dpt[r] = p * (dpt[r] - delta) * scale;
          }
        } else {
#pragma unroll
          for (int r = 0; r < 16; r++) {
            const float p = __expf(st[r] * scale - Lq);
            dpt[r] = p * (dpt[r] - delta) * scale;
          }
        }
        bf16x8 af[2];
        to_afrag(dpt, af);
#pragma unroll
        for (int half = 0; half < 2; half++)
#pragma unroll
          for (int db = 0; db < 2; db++) dq[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[half], ktr[half][db], dq[db], 0, 0, 0);
      }
    } else if (more) {
      load_tile(t + 1);
    }
    if (more) store_tile((t + 1) & 1);   // behind this iteration's barrier: nobody reads that buffer any more; visible behind the next one
  }
  if (!live) return;
  // registers r are queries q0 + (r&3) + 8 (r>>2) + 4 kg, the lane is channel db*32 + ql: 32 lanes write 64 consecutive bytes of a row
  bf16* dqg = a.dq + base;
#pragma unroll
  for (int db = 0; db < 2; db++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int qo = q0 + (r & 3) + 8 * (r >> 2) + 4 * kg;
      if (qo < S) dqg[(size_t)qo * a.rs + db * 32 + ql] = (bf16)dq[db][r];
    }
#endif
}

__global__ __launch_bounds__(NT) void attention_bwd_stream_dkdv_kernel(Args a) {
#if __HIP_DEVICE_COMPILE__
  extern __shared__ __attribute__((aligned(256))) char smem[];      // 2 x DKDV_BUF
  const int S = a.S, C = a.H * D;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned item = xcd_remap(blockIdx.x, gridDim.x);
  const int bh = (int)(item / (unsigned)a.nb), blk = (int)(item % (unsigned)a.nb);
  const int b = bh / a.H, h = bh % a.H;
  const size_t base = (size_t)b * a.bs + h * D;
  const bf16 *qp = a.q + base, *kp = a.k + base, *vp = a.v + base;
  const bf16* dog = a.dout + (size_t)b * S * C + h * D;
  const float* lse = a.lse + (size_t)bh * S;
  const float* dlt = a.delta + (size_t)bh * S;
  const int kg = lane >> 5, ql = lane & 31;
  const int key0 = blk * BB + wave * BW;     // the wave's first key
  const int key = key0 + ql;
  const bool live = key0 < S;                // wave-uniform
  const int nt = (S + TT - 1) / TT;

  // staging: thread -> query row tid >> 3 of the tile, 16-B chunk tid & 7 of its Q row and of its dO row; threads 0-63 its L, threads 64-127 its delta
  const int srow = tid >> 3, sc = tid & 7;
  const int rsl = att_kslot<ROW>(srow, sc), tsl = att_vslot<ROW>(srow, sc);
  uint4 qreg, dreg;
  float sreg = 0.f;
  auto load_tile = [&](int t) {
    const int row = t * TT + srow;
    qreg = uint4{0, 0, 0, 0}; dreg = uint4{0, 0, 0, 0};
    if (row < S) {
      qreg = *reinterpret_cast<const uint4*>(qp + (size_t)row * a.rs + sc * 8);
      dreg = *reinterpret_cast<const uint4*>(dog + (size_t)row * C + sc * 8);
    }
    if (tid < 2 * TT) {
      const int sq = t * TT + (tid & (TT - 1));
      sreg = tid < TT ? INFINITY : 0.f;      // a padded query: L = +inf, delta = 0 -> p = 0, dS = 0
      if (sq < S) sreg = tid < TT ? lse[sq] : dlt[sq];
    }
  };
  auto store_tile = [&](int buf) {
    char* img = smem + buf * DKDV_BUF;
    *reinterpret_cast<uint4*>(img + rsl) = qreg;
    *reinterpret_cast<uint4*>(img + TILE + tsl) = qreg;
    *reinterpret_cast<uint4*>(img + 2 * TILE + rsl) = dreg;
    *reinterpret_cast<uint4*>(img + 3 * TILE + tsl) = dreg;
    if (tid < 2 * TT) reinterpret_cast<float*>(img + 4 * TILE)[tid] = sreg;
  };
  load_tile(0);

  // the wave's K / V fragments (column operands: key on the lane)
  bf16x8 kfb[4], vfb[4];
#pragma unroll
  for (int kk = 0; kk < 4; kk++) {
    uint4 tk = {0, 0, 0, 0}, tv = {0, 0, 0, 0};
    const int d0 = kk * 16 + kg * 8;
    if (key < S) {
      tk = *reinterpret_cast<const uint4*>(kp + (size_t)key * a.rs + d0);
      tv = *reinterpret_cast<const uint4*>(vp + (size_t)key * a.rs + d0);
    }
    kfb[kk] = *reinterpret_cast<bf16x8*>(&tk);
    vfb[kk] = *reinterpret_cast<bf16x8*>(&tv);
  }
  const int toff = tr_off0(lane);
  const float scale = a.scale;
  store_tile(0);

  f32x16 dk[2], dv[2];
#pragma unroll
  for (int db = 0; db < 2; db++)
#pragma unroll
    for (int r = 0; r < 16; r++) { dk[db][r] = 0.f; dv[db][r] = 0.f; }

  for (int t = 0; t < nt; t++) {
    __syncthreads();          // tile t's images are complete, and every wave has left tile t - 1's buffer (the one this iteration refills)
    const char* qs = smem + (t & 1) * DKDV_BUF;
    const char* qt = qs + TILE;
    const char* ds = qs + 2 * TILE;
    const char* dt = qs + 3 * TILE;
    const float* Ls = reinterpret_cast<const float*>(qs + 4 * TILE);
    const float* Ds = Ls + TT;
    const bool more = t + 1 < nt;
    if (live) {
#pragma unroll
      for (int qb = 0; qb < 2; qb++) {
        if (qb == 1 && t * TT + 32 >= S) break;      // the last tile's second block wholly past S (wave-uniform): all its P and dS are zero
        // s[r] = score(query qb*32 + (r&3) + 8 (r>>2) + 4 kg of the tile, this lane's key), dp likewise
        bf16x8 qfr[4], dor[4];
#pragma unroll
        for (int kk = 0; kk < 4; kk++) {
          const int off = att_kslot<ROW>(qb * 32 + ql, kk * 2 + kg);
          qfr[kk] = *reinterpret_cast<const bf16x8*>(qs + off);
          dor[kk] = *reinterpret_cast<const bf16x8*>(ds + off);
        }
        __builtin_amdgcn_sched_barrier(0);
        f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; r++) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
        for (int kk = 0; kk < 4; kk++) {
          s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qfr[kk], kfb[kk], s, 0, 0, 0);
          dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dor[kk], vfb[kk], dp, 0, 0, 0);
        }
        // behind the products: the row statistics of the block's 32 queries and the transposed dO / Q fragments (they land under the exponentials), and the next
        // tile's global loads
        f32x4 Lv[4], Dv[4];
#pragma unroll
        for (int r4 = 0; r4 < 4; r4++) {
          Lv[r4] = *reinterpret_cast<const f32x4*>(Ls + qb * 32 + 8 * r4 + 4 * kg);
          Dv[r4] = *reinterpret_cast<const f32x4*>(Ds + qb * 32 + 8 * r4 + 4 * kg);
        }
        bf16x8 dft[2][2], qft[2][2];
#pragma unroll
        for (int half = 0; half < 2; half++)
#pragma unroll
          for (int db = 0; db < 2; db++) {
            dft[half][db] = tr_frag(dt, qb * 2 + half, toff, db);
            qft[half][db] = tr_frag(qt, qb * 2 + half, toff, db);
          }
        if (qb == 0 && more) load_tile(t + 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r4 = 0; r4 < 4; r4++)
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const float p = __expf(s[r4 * 4 + r] * scale - Lv[r4][r]);
            s[r4 * 4 + r] = p;
            dp[r4 * 4 + r] = p * (dp[r4 * 4 + r] - Dv[r4][r]) * scale;
          }
        bf16x8 pf[2], dsf[2];
        to_afrag(s, pf);
        to_afrag(dp, dsf);
#pragma unroll
        for (int half = 0; half < 2; half++)
#pragma unroll
          for (int db = 0; db < 2; db++) {
            dv[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pf[half], dft[half][db], dv[db], 0, 0, 0);
            dk[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dsf[half], qft[half][db], dk[db], 0, 0, 0);
          }
      }
    } else if (more) {
      load_tile(t + 1);
    }
    if (more) store_tile((t + 1) & 1);   // behind this iteration's barrier: nobody reads that buffer any more; visible behind the next one
  }
  if (!live) return;
  // registers r are keys key0 + (r&3) + 8 (r>>2) + 4 kg, the lane is channel db*32 + ql
  bf16* dkg = a.dk + base;
  bf16* dvg = a.dv + base;
#pragma unroll
  for (int db = 0; db < 2; db++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int ko = key0 + (r & 3) + 8 * (r >> 2) + 4 * kg;
      if (ko < S) {
        dkg[(size_t)ko * a.rs + db * 32 + ql] = (bf16)dk[db][r];
        dvg[(size_t)ko * a.rs + db * 32 + ql] = (bf16)dv[db][r];
      }
    }
#endif
}

}  // namespace dmvae_attn_bwd_stream

extern "C" int dmvae_attention_bwd_qkv_stream_bf16(const void* qkv, const void* out, const void* dout, const void* lse, void* dqkv, void* delta, int batch, int seq,
                                                   int heads, int head_dim, float scale, hipStream_t stream) {
  using namespace dmvae_attn_bwd_stream;
  DMVAE_CHECK_ARG(qkv && out && dout && dqkv, "attention_bwd_qkv_stream_bf16: null qkv, out, dout or dqkv");
  DMVAE_CHECK_ARG(lse, "attention_bwd_qkv_stream_bf16: null lse (the forward's row statistics are required)");
  DMVAE_CHECK_ARG(delta, "attention_bwd_qkv_stream_bf16: null delta scratch (batch * heads * seq floats)");
  DMVAE_CHECK_ARG(batch > 0 && heads > 0 && seq >= 1, "attention_bwd_qkv_stream_bf16: needs batch, heads, seq >= 1 (got %d, %d, %d)", batch, heads, seq);
  DMVAE_CHECK_ARG(head_dim == D, "attention_bwd_qkv_stream_bf16: needs head_dim 64 (got %d)", head_dim);
  DMVAE_CHECK_ARG(scale > 0.f && isfinite(scale), "attention_bwd_qkv_stream_bf16: needs a finite scale > 0 (got %g)", (double)scale);
  const long long C = (long long)heads * head_dim;
  const long long nb = ((long long)seq + BB - 1) / BB, blocks = (long long)batch * heads * nb;
  // the row stride and the (sample, head) count are ints in the kernels; the flat grid is one dimension
  DMVAE_CHECK_ARG(3 * C <= 0x7fffffffLL && (long long)batch * heads <= 0x7fffffffLL && blocks <= 0x7fffffffLL,
                  "attention_bwd_qkv_stream_bf16: %d x %d heads x %d tokens does not fit the grid", batch, heads, seq);
  Args a = {};
  a.q = (const bf16*)qkv; a.k = a.q + C; a.v = a.q + 2 * C;
  a.dq = (bf16*)dqkv; a.dk = a.dq + C; a.dv = a.dq + 2 * C;
  a.o = (const bf16*)out; a.dout = (const bf16*)dout; a.lse = (const float*)lse; a.delta = (float*)delta;
  a.bs = (long long)seq * 3 * C; a.rs = (int)(3 * C);
  a.S = seq; a.H = heads; a.nb = (int)nb; a.scale = scale;
  DMVAE_LDS_OPTIN(2 * DKDV_BUF, attention_bwd_stream_dkdv_kernel);
  hipLaunchKernelGGL(attention_bwd_stream_dq_kernel, dim3((unsigned)blocks), dim3(NT), 0, stream, a);
  DMVAE_CHECK_LAUNCH();
  hipLaunchKernelGGL(attention_bwd_stream_dkdv_kernel, dim3((unsigned)blocks), dim3(NT), 2 * DKDV_BUF, stream, a);
  DMVAE_CHECK_LAUNCH();
  return 0;
}
