// Streaming backward of the encoder's multi-head self-attention for gfx950 (MI355X): d(qkv) at ANY token count, the backward half of attention_stream.hip (reference:
// autograd of models/dino_layers/attention.py:56-69 where the encoder trains, train_dmd.py:349,519, at the token counts models/vae.py:38-50 reaches: 577, 1025).
// csrc/attention_bwd.hip keeps a whole head's operands resident in LDS and stops at 288 tokens; these two kernels walk 64-row tiles instead.  Nothing of size S x S
// reaches HBM; the only scratch is delta [B*H][S] f32.
//
//   P = exp(scale s - L)      dV = P^T dO      dP = dO V^T      dS = P o (dP - delta),  delta_q = dO_q . O_q      dQ = scale dS K      dK = scale dS^T Q
//
// Operands: qkv [B][S][3][H][64] bf16 (the qkv Linear's output), out / dout [B][S][H*64] bf16, lse [B*H][S] f32 = scale * max + log(sum) of a query's scaled scores
// (what attention_stream.hip and attention.hip write), dqkv in qkv's layout.
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
// the blocks of one head share an XCD's L2.  An operand that is read by rows AND transposed is staged twice, once per layout of attention_common.h (att_kslot: conflict-free
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
// Resources: one table for all four instantiations at the end of this header.
//
// Both kernels are templates on DP, the staged head dim.  DP = 64 is everything above: the encoder's entry dmvae_attention_bwd_qkv_stream_bf16, and head-major
// operands of head dim 64.  DP = 96 is LightningDiT's head dim 72 on the head-major operands of dmvae_qknorm_rope_bf16 (q, k, dq, dk [B*H][N][72 or 96], v, dv
// [B*H][N][72]; entry dmvae_attention_bwd_heads_stream_bf16): 256-B rows in the layouts of the 96-wide resident kernel (attention_common.h att_kslot<256> / att_vslot<256>),
// 16-KiB images.  The channels 72 .. 95 are zeros in LDS and never loaded, the products over channels take five 16-channel steps (upper half of the fifth zero, the
// sixth skipped), the accumulators are three 32-channel blocks; dV columns >= 72 are not stored and the padded columns of dq / dk (rows of 96) are written as the
// exact zeros the zero K / Q channels produce.  The operands are described by strides, q / k and v separately (head-major v rows are 72 wide, q / k rows 72 or 96).
// The 96-wide KEY pass does not fit eight waves: two more 32-channel accumulator blocks (dK, dV: + 32 registers) and the wider fragments put it past 256 registers.
// Choice: a FOUR-wave workgroup (one wave per SIMD, 512 registers: the accumulators go to AGPRs), 128 keys per workgroup, four staging sweeps per tile; fewer keys per
// wave or 16-wide accumulator blocks would have kept eight waves at half the matrix work per fragment read.  Its LDS, 2 x (4 x 16 KiB + 512 B) = 129 KiB dynamic,
// admits one workgroup per CU either way.
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; no scratch and no spill in any of the four).  "Waves per SIMD" is the
// compiler's register-limited figure; a workgroup of 8 waves puts two on each SIMD, so what is resident is whole workgroups within that figure and within LDS.
//   DP = 64 query pass (8 waves): 161 VGPRs, 0 AGPRs, 48 SGPRs, 48 KiB static LDS; 3 waves per SIMD by registers = ONE resident workgroup per CU (a second would need
//     4 per SIMD; LDS would admit three).  Before the operands were described by separate q / k and v strides: 159 VGPRs, 44 SGPRs, the same residency.
//   DP = 64 key pass (8 waves): 238 VGPRs, 0 AGPRs, 54 SGPRs (before: 48), 65 KiB dynamic LDS; 2 waves per SIMD = one workgroup per CU (registers and LDS agree).
//   DP = 96 query pass (8 waves): 216 VGPRs, 0 AGPRs, 54 SGPRs, 96 KiB dynamic LDS; 2 waves per SIMD = one workgroup per CU.
//   DP = 96 key pass (4 waves): 234 VGPRs, 128 AGPRs, 59 SGPRs, 129 KiB dynamic LDS; 1 wave per SIMD = one workgroup per CU.
#include "attention_common.h"
#include "dmvae_hip.h"

namespace dmvae_attn_bwd_stream {

constexpr int NTQ = 512;         // query pass: 8 waves
constexpr int BW = 32;           // rows (queries / keys) a wave owns
constexpr int TT = ATT_STREAM_TILE;       // rows per streamed tile
// attention_common.h's tile geometry (dV columns >= 72 and dQ / dK columns past the row width are not stored) plus the two passes' LDS images.  NT: threads of the
// workgroup (the key pass at 96 runs four waves: file header).
template <int DP, int NT = NTQ> struct Geo : AttnStreamGeo<DP, NT> {
  static constexpr int DQ_BUF = 3 * Geo::TILE;                                    // K rows | K transposed | V rows
  static constexpr int DKDV_BUF = 4 * Geo::TILE + 2 * TT * (int)sizeof(float);    // Q rows | Q transposed | dO rows | dO transposed | L [64] | delta [64]
};

// The operand fields, named as attention_common.h says.  Both passes address q AND k (and dq, dk) through q's geometry (q_*): the two always share one (packed qkv: the
// same strides; head-major: the same row width).  v and dv have their own (v_*).  At DP = 96 q_rs is also the width of a q / k / dq / dk row (72 or 96).
struct Args {
  const bf16 *q, *k, *v;
  const bf16 *o, *dout;      // [B][S][H * D]
  bf16 *dq, *dk, *dv;        // dq, dk in q's geometry, dv in v's
  const float* lse;          // [B * H][S]
  float* delta;              // [B * H][S]: written by the query pass, read by the key pass
  long long q_bs, q_hs, v_bs, v_hs;      // elements
  int q_rs, v_rs;            // elements between token rows
  int S, H;
  int nb;                    // row blocks per (sample, head) of the kernel being launched
  float scale;
  long long k_bs, k_hs;      // k's geometry as the shared recipes fill it: equal to q's, and read by neither kernel (behind everything they load, so the loads keep their places)
  int k_rs;
};

// the query pass' images: static up to 64 KiB (the 64-wide form, as before), the launch's dynamic LDS beyond
template <int BYTES>
__device__ __forceinline__ char* dq_image() {
  if constexpr (BYTES <= 65536) {
    __shared__ __attribute__((aligned(256))) char img[BYTES];
    return img;
  } else {
    extern __shared__ __attribute__((aligned(256))) char dyn[];
    return dyn;
  }
}

template <int DP>
__global__ __launch_bounds__(NTQ) void attention_bwd_stream_dq_kernel(Args a) {
#if __HIP_DEVICE_COMPILE__
  using G = Geo<DP>;
  constexpr int NT = NTQ, D = G::D, ROW = G::ROW, TILE = G::TILE, KS = G::KS, DB = G::DB, CPR = G::CPR, SW = G::SW, BB = G::BB, DQ_BUF = G::DQ_BUF;
  char* smem = dq_image<2 * DQ_BUF>();
  const int S = a.S, C = a.H * D;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned item = xcd_remap(blockIdx.x, gridDim.x);
  const int bh = (int)(item / (unsigned)a.nb), blk = (int)(item % (unsigned)a.nb);
  const int b = bh / a.H, h = bh % a.H;
  const size_t base = (size_t)b * a.q_bs + h * a.q_hs, vbase = (size_t)b * a.v_bs + h * a.v_hs;
  const bf16 *qp = a.q + base, *kp = a.k + base, *vp = a.v + vbase;
  const bf16* og = a.o + (size_t)b * S * C + h * D;
  const bf16* dog = a.dout + (size_t)b * S * C + h * D;
  const int kg = lane >> 5, ql = lane & 31;
  const int q0 = blk * BB + wave * BW;       // the wave's first query
  const int q = q0 + ql;
  const bool live = q0 < S;                  // wave-uniform
  const int nt = (S + TT - 1) / TT;

  // staging: thread -> key row tid / CPR (+ NT / CPR per sweep) of the tile, 16-B chunk tid % CPR of its K row and of its V row; a chunk past the D real channels
  // is not loaded (zeros in LDS)
  const int skey = tid / CPR, sc = tid % CPR;
  int rsl[SW], tsl[SW];
#pragma unroll
  for (int it = 0; it < SW; it++) { rsl[it] = att_kslot<ROW>(skey + it * (NT / CPR), sc); tsl[it] = att_vslot<ROW>(skey + it * (NT / CPR), sc); }
  uint4 kreg[SW], vreg[SW];
  auto load_tile = [&](int t) {
#pragma unroll
    for (int it = 0; it < SW; it++) {
      const int key = t * TT + skey + it * (NT / CPR);
      kreg[it] = uint4{0, 0, 0, 0}; vreg[it] = uint4{0, 0, 0, 0};
      if (key < S && (DP == 64 || sc < D / 8)) {
        kreg[it] = *reinterpret_cast<const uint4*>(kp + (size_t)key * a.q_rs + sc * 8);
        vreg[it] = *reinterpret_cast<const uint4*>(vp + (size_t)key * a.v_rs + sc * 8);
      }
    }
  };
  auto store_tile = [&](int buf) {
    char* img = smem + buf * DQ_BUF;
#pragma unroll
    for (int it = 0; it < SW; it++) {
      *reinterpret_cast<uint4*>(img + rsl[it]) = kreg[it];
      *reinterpret_cast<uint4*>(img + TILE + tsl[it]) = kreg[it];
      *reinterpret_cast<uint4*>(img + 2 * TILE + rsl[it]) = vreg[it];
    }
  };
  load_tile(0);

  // the wave's Q / dO fragments (column operands: query on the lane, 8 channels per lane per 16-channel step) and delta
  bf16x8 qf[KS], dof[KS];
  float delta = 0.f;
#pragma unroll
  for (int kk = 0; kk < KS; kk++) {
    uint4 tq = {0, 0, 0, 0}, td = {0, 0, 0, 0}, to = {0, 0, 0, 0};
    const int d0 = kk * 16 + kg * 8;
    if (q < S && (DP == 64 || d0 < D)) {
      tq = *reinterpret_cast<const uint4*>(qp + (size_t)q * a.q_rs + d0);
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
  const int toff = tr_off0<ROW>(lane);
  const float scale = a.scale;
  store_tile(0);

  f32x16 dq[DB];
#pragma unroll
  for (int db = 0; db < DB; db++)
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
        bf16x8 kf[KS], vf[KS];
#pragma unroll
        for (int kk = 0; kk < KS; kk++) {
          const int off = att_kslot<ROW>(kb * 32 + ql, kk * 2 + kg);
          kf[kk] = *reinterpret_cast<const bf16x8*>(ks + off);
          vf[kk] = *reinterpret_cast<const bf16x8*>(vs + off);
        }
        __builtin_amdgcn_sched_barrier(0);
        f32x16 st, dpt;
#pragma unroll
        for (int r = 0; r < 16; r++) { st[r] = 0.f; dpt[r] = 0.f; }
#pragma unroll
        for (int kk = 0; kk < KS; kk++) {
          st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[kk], qf[kk], st, 0, 0, 0);
          dpt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[kk], dof[kk], dpt, 0, 0, 0);
        }
        // behind the products: the K^T fragments of the dQ product (they land under the exponentials), and the next tile's global loads
        bf16x8 ktr[2][DB];
#pragma unroll
        for (int half = 0; half < 2; half++)
#pragma unroll
          for (int db = 0; db < DB; db++) ktr[half][db] = tr_frag<ROW>(kt, kb * 2 + half, toff, db);
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
          for (int db = 0; db < DB; db++) dq[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[half], ktr[half][db], dq[db], 0, 0, 0);
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
  for (int db = 0; db < DB; db++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int qo = q0 + (r & 3) + 8 * (r >> 2) + 4 * kg;
      if (qo < S && (DP == 64 || db * 32 + ql < a.q_rs)) dqg[(size_t)qo * a.q_rs + db * 32 + ql] = (bf16)dq[db][r];
    }
#endif
}

template <int DP, int NT>
__global__ __launch_bounds__(NT) void attention_bwd_stream_dkdv_kernel(Args a) {
#if __HIP_DEVICE_COMPILE__
  using G = Geo<DP, NT>;
  constexpr int D = G::D, ROW = G::ROW, TILE = G::TILE, KS = G::KS, DB = G::DB, CPR = G::CPR, SW = G::SW, BB = G::BB, DKDV_BUF = G::DKDV_BUF;
  extern __shared__ __attribute__((aligned(256))) char smem[];      // 2 x DKDV_BUF
  const int S = a.S, C = a.H * D;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned item = xcd_remap(blockIdx.x, gridDim.x);
  const int bh = (int)(item / (unsigned)a.nb), blk = (int)(item % (unsigned)a.nb);
  const int b = bh / a.H, h = bh % a.H;
  const size_t base = (size_t)b * a.q_bs + h * a.q_hs, vbase = (size_t)b * a.v_bs + h * a.v_hs;
  const bf16 *qp = a.q + base, *kp = a.k + base, *vp = a.v + vbase;
  const bf16* dog = a.dout + (size_t)b * S * C + h * D;
  const float* lse = a.lse + (size_t)bh * S;
  const float* dlt = a.delta + (size_t)bh * S;
  const int kg = lane >> 5, ql = lane & 31;
  const int key0 = blk * BB + wave * BW;     // the wave's first key
  const int key = key0 + ql;
  const bool live = key0 < S;                // wave-uniform
  const int nt = (S + TT - 1) / TT;

  // staging: thread -> query row tid / CPR (+ NT / CPR per sweep) of the tile, 16-B chunk tid % CPR of its Q row and of its dO row (a chunk past the D real channels
  // is not loaded: zeros in LDS); threads 0-63 its L, threads 64-127 its delta
  const int srow = tid / CPR, sc = tid % CPR;
  int rsl[SW], tsl[SW];
#pragma unroll
  for (int it = 0; it < SW; it++) { rsl[it] = att_kslot<ROW>(srow + it * (NT / CPR), sc); tsl[it] = att_vslot<ROW>(srow + it * (NT / CPR), sc); }
  uint4 qreg[SW], dreg[SW];
  float sreg = 0.f;
  auto load_tile = [&](int t) {
#pragma unroll
    for (int it = 0; it < SW; it++) {
      const int row = t * TT + srow + it * (NT / CPR);
      qreg[it] = uint4{0, 0, 0, 0}; dreg[it] = uint4{0, 0, 0, 0};
      if (row < S && (DP == 64 || sc < D / 8)) {
        qreg[it] = *reinterpret_cast<const uint4*>(qp + (size_t)row * a.q_rs + sc * 8);
        dreg[it] = *reinterpret_cast<const uint4*>(dog + (size_t)row * C + sc * 8);
      }
    }
    if (tid < 2 * TT) {
      const int sq = t * TT + (tid & (TT - 1));
      sreg = tid < TT ? INFINITY : 0.f;      // a padded query: L = +inf, delta = 0 -> p = 0, dS = 0
      if (sq < S) sreg = tid < TT ? lse[sq] : dlt[sq];
    }
  };
  auto store_tile = [&](int buf) {
    char* img = smem + buf * DKDV_BUF;
#pragma unroll
    for (int it = 0; it < SW; it++) {
      *reinterpret_cast<uint4*>(img + rsl[it]) = qreg[it];
      *reinterpret_cast<uint4*>(img + TILE + tsl[it]) = qreg[it];
      *reinterpret_cast<uint4*>(img + 2 * TILE + rsl[it]) = dreg[it];
      *reinterpret_cast<uint4*>(img + 3 * TILE + tsl[it]) = dreg[it];
    }
    if (tid < 2 * TT) reinterpret_cast<float*>(img + 4 * TILE)[tid] = sreg;
  };
  load_tile(0);

  // the wave's K / V fragments (column operands: key on the lane)
  bf16x8 kfb[KS], vfb[KS];
#pragma unroll
  for (int kk = 0; kk < KS; kk++) {
    uint4 tk = {0, 0, 0, 0}, tv = {0, 0, 0, 0};
    const int d0 = kk * 16 + kg * 8;
    if (key < S && (DP == 64 || d0 < D)) {
      tk = *reinterpret_cast<const uint4*>(kp + (size_t)key * a.q_rs + d0);
      tv = *reinterpret_cast<const uint4*>(vp + (size_t)key * a.v_rs + d0);
    }
    kfb[kk] = *reinterpret_cast<bf16x8*>(&tk);
    vfb[kk] = *reinterpret_cast<bf16x8*>(&tv);
  }
  const int toff = tr_off0<ROW>(lane);
  const float scale = a.scale;
  store_tile(0);

  f32x16 dk[DB], dv[DB];
#pragma unroll
  for (int db = 0; db < DB; db++)
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
        bf16x8 qfr[KS], dor[KS];
#pragma unroll
        for (int kk = 0; kk < KS; kk++) {
          const int off = att_kslot<ROW>(qb * 32 + ql, kk * 2 + kg);
          qfr[kk] = *reinterpret_cast<const bf16x8*>(qs + off);
          dor[kk] = *reinterpret_cast<const bf16x8*>(ds + off);
        }
        __builtin_amdgcn_sched_barrier(0);
        f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; r++) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
        for (int kk = 0; kk < KS; kk++) {
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
        bf16x8 dft[2][DB], qft[2][DB];
#pragma unroll
        for (int half = 0; half < 2; half++)
#pragma unroll
          for (int db = 0; db < DB; db++) {
            dft[half][db] = tr_frag<ROW>(dt, qb * 2 + half, toff, db);
            qft[half][db] = tr_frag<ROW>(qt, qb * 2 + half, toff, db);
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
          for (int db = 0; db < DB; db++) {
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
  bf16* dvg = a.dv + vbase;
#pragma unroll
  for (int db = 0; db < DB; db++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int ko = key0 + (r & 3) + 8 * (r >> 2) + 4 * kg;
      if (ko < S) {
        if (DP == 64 || db * 32 + ql < a.q_rs) dkg[(size_t)ko * a.q_rs + db * 32 + ql] = (bf16)dk[db][r];
        if (DP == 64 || db * 32 + ql < D) dvg[(size_t)ko * a.v_rs + db * 32 + ql] = (bf16)dv[db][r];
      }
    }
#endif
}

}  // namespace dmvae_attn_bwd_stream

extern "C" int dmvae_attention_bwd_qkv_stream_bf16(const void* qkv, const void* out, const void* dout, const void* lse, void* dqkv, void* delta, int batch, int seq,
                                                   int heads, int head_dim, float scale, hipStream_t stream) {
  using namespace dmvae_attn_bwd_stream;
  using G = Geo<64>;
  if (int e = attn_stream_check("attention_bwd_qkv_stream_bf16", "qkv, out, dout or dqkv", qkv && out && dout && dqkv, ATTN_PACKED, ATTN_BWD, lse, delta, batch, seq, heads, head_dim, 0,
                                scale, G::BB)) return e;
  Args a = {};
  attn_operands_qkv(a, qkv, seq, heads, head_dim);
  attn_grads_qkv(a, dqkv, heads, head_dim);
  a.o = (const bf16*)out; a.dout = (const bf16*)dout; a.lse = (const float*)lse; a.delta = (float*)delta;
  a.nb = attn_row_blocks(seq, G::BB); a.scale = scale;
  const dim3 grid((unsigned)(batch * heads * a.nb));
  DMVAE_LDS_OPTIN(2 * G::DKDV_BUF, attention_bwd_stream_dkdv_kernel<64, NTQ>);
  hipLaunchKernelGGL(attention_bwd_stream_dq_kernel<64>, grid, dim3(NTQ), 0, stream, a);
  DMVAE_CHECK_LAUNCH();
  hipLaunchKernelGGL((attention_bwd_stream_dkdv_kernel<64, NTQ>), grid, dim3(NTQ), 2 * G::DKDV_BUF, stream, a);
  DMVAE_CHECK_LAUNCH();
  return 0;
}

// The same two passes on head-major operands (q, k, dq, dk: [B*H][N][QD], v, dv: [B*H][N][D]: what dmvae_attention_bwd_heads_lse_bf16 takes) at any token count.
// head_dim 64 or 72; QD = head_dim (unpadded rows) or its round-up to 32 (rows zero-padded by the producer; the padded columns of dq / dk are written as zeros).
extern "C" int dmvae_attention_bwd_heads_stream_bf16(const void* q, const void* k, const void* v, const void* out, const void* dout, const void* lse, void* dq, void* dk,
                                                     void* dv, void* delta, int batch, int seq, int heads, int head_dim, int head_dim_padded, float scale,
                                                     hipStream_t stream) {
  using namespace dmvae_attn_bwd_stream;
  constexpr int NTK96 = 256;      // the 96-wide key pass: four waves, 128 keys per workgroup (file header)
  constexpr int lds_dq96 = 2 * Geo<96>::DQ_BUF, lds_dkdv64 = 2 * Geo<64>::DKDV_BUF, lds_dkdv96 = 2 * Geo<96, NTK96>::DKDV_BUF;
  if (int e = attn_stream_check("attention_bwd_heads_stream_bf16", "q, k, v, out, dout, dq, dk or dv", q && k && v && out && dout && dq && dk && dv, ATTN_HEADS, ATTN_BWD, lse, delta,
                                batch, seq, heads, head_dim, head_dim_padded, scale, head_dim == 64 ? Geo<64>::BB : Geo<96, NTK96>::BB)) return e;
  const int nbq = attn_row_blocks(seq, Geo<64>::BB);
  const int nbk = head_dim == 64 ? nbq : attn_row_blocks(seq, Geo<96, NTK96>::BB);
  Args a = {};
  attn_operands_heads(a, q, k, v, seq, heads, head_dim, head_dim_padded);
  attn_grads_heads(a, dq, dk, dv);
  a.o = (const bf16*)out; a.dout = (const bf16*)dout; a.lse = (const float*)lse; a.delta = (float*)delta;
  a.scale = scale;
  const unsigned bh = (unsigned)(batch * heads);
  if (head_dim == 64) {
    DMVAE_LDS_OPTIN(lds_dkdv64, attention_bwd_stream_dkdv_kernel<64, NTQ>);
    a.nb = nbq;
    hipLaunchKernelGGL(attention_bwd_stream_dq_kernel<64>, dim3(bh * (unsigned)nbq), dim3(NTQ), 0, stream, a);
    DMVAE_CHECK_LAUNCH();
    hipLaunchKernelGGL((attention_bwd_stream_dkdv_kernel<64, NTQ>), dim3(bh * (unsigned)nbq), dim3(NTQ), lds_dkdv64, stream, a);
  } else {
    DMVAE_LDS_OPTIN(lds_dq96, attention_bwd_stream_dq_kernel<96>);
    DMVAE_LDS_OPTIN(lds_dkdv96, attention_bwd_stream_dkdv_kernel<96, NTK96>);
    a.nb = nbq;
    hipLaunchKernelGGL(attention_bwd_stream_dq_kernel<96>, dim3(bh * (unsigned)nbq), dim3(NTQ), lds_dq96, stream, a);
    DMVAE_CHECK_LAUNCH();
    a.nb = nbk;
    hipLaunchKernelGGL((attention_bwd_stream_dkdv_kernel<96, NTK96>), dim3(bh * (unsigned)nbk), dim3(NTK96), lds_dkdv96, stream, a);
  }
  DMVAE_CHECK_LAUNCH();
  return 0;
}
