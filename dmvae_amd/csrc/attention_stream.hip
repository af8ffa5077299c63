// Streaming-softmax multi-head self-attention forward for gfx950 (MI355X): the encoder's attention at ANY token count -- patch 8 at 256 px is 1025 tokens, 384 px at
// patch 16 is 577 (reference: models/dino_layers/attention.py:56-69, reached with patch_size / img_size through models/vae.py:38-50 and train_diffusion.py:54,224).
// csrc/attention.hip's attention_kernel keeps a whole head's K and V resident in LDS and therefore stops at 288 tokens; this kernel walks 64-key tiles with an online
// softmax instead.  Nothing of size S x S reaches HBM.
//
// Operands: the qkv Linear's output [B][S][3][H][64] bf16 described by strides (attention_common.h's operand fields: per-(sample, head) base = ptr + b * bs + h * hs, token rows rs elements
// apart -- head-major operands fit the same struct), out [B][S][H*64] bf16, optional lse [B*H][S] f32 = scale * max + log(sum) of a query's scaled scores (natural
// log: the definition of dmvae_attention_*_lse_bf16, what the LSE-consuming backward kernels rebuild P from).
//
// Structure (cdna_hip_programming "Fused attention prefill"): a workgroup = 8 waves owns 256 consecutive queries of one (sample, head), 32 per wave, and walks the
// ceil(S / 64) key tiles.  Per wave, in registers for the whole walk: the Q fragments (4 x bf16x8), the running maximum m of the RAW scores, the running sum l, and the
// f32 output accumulators (2 x 16).  A K tile (64 keys x 128 B, 16-B chunks XOR-swizzled per key: att_kslot) and a V tile (64 x 128 B in the image the transpose read
// ds_read_b64_tr_b16 wants: att_vslot) are double-buffered in LDS: 2 x 16 KiB = 32 KiB static.  Register staging: every thread carries one 16-B piece of the next K tile
// and one of the next V tile; their global loads are issued right after this tile's QK^T, land under the softmax and the PV products, and are written to the OTHER buffer
// at the end of the iteration -- behind the barrier at the head of this iteration, which is what says that every wave has left that buffer.  One barrier per tile.
//
// Products: S^T = K Q^T (swapped), so a lane owns ONE query -- (lane & 31) of the wave's 32 -- and 16 of a 32-key block's scores (the other 16 sit in lane ^ 32): the row
// maximum and the row sum are in-lane chains plus ONE exchange with lane ^ 32 (v_permlane32_swap).
// Rescale factor: exp(m_old - m_new) lives in the query's lane.  The output accumulator keeps the query in the lane as well, O^T = V^T P^T (V fragments as the row
// operand, P as the column operand): the rescale is then 32 in-lane multiplies per tile with no broadcast, 1 / l at the end is the lane's own value, and a lane stores 4
// consecutive channels of its query's row.  P reaches the column-operand layout with the same two v_permlane32_swap per 16 keys that the resident kernel uses; the
// alternative (O = P V, queries along the registers) would need the factor of 16 different queries in every lane -- a cross-lane broadcast per tile.
//
// Rounding sites: q, k, v are bf16 operands; scores are accumulated in f32 on the matrix cores; p = exp(scale * s - scale * m) = 2^(s * ec - m * ec), ec = scale *
// log2(e), is one fma + v_exp_f32 in f32; the row sum l is taken from the f32 p (in a fixed order); p is rounded to bf16 ONCE as the PV operand; O is accumulated in f32,
// multiplied by 1 / l at the end and rounded to bf16 once.  The O rescale and l rescale use the same f32 factor.
// Always rescale: no deferred-max threshold (a data-dependent branch with a correctness hazard for about 5 %).
// Ragged S: keys >= S exist only in the last tile, are staged as zero rows and score -inf (p = 0 exactly); with ceil(S / 64) tiles every tile holds at least one live key, so
// every tile's maximum is finite: the first tile's factor is 2^(-inf) = 0 on zero accumulators, never exp(-inf - (-inf)).  Queries >= S compute on zero fragments and are
// not stored.  A wave whose 32 queries are all >= S skips the matrix work and only stages and synchronises.
// Determinism: every reduction has a fixed order and every operation is per (sample, head): reruns are bit-identical and a 2B-sample call equals two B-sample calls.
// Grid: one flat dimension of B * H * ceil(S / 256) workgroups through xcd_remap, so that the query blocks of one head run on one XCD and share its L2 for K / V.
//
// Two instantiations of the one kernel (template parameter DP, the staged head dim).  DP = 64: everything above -- the encoder's entry dmvae_attention_qkv_stream_bf16
// and head-major operands of head dim 64.  DP = 96: LightningDiT's head dim 72 on the head-major operands of dmvae_qknorm_rope_bf16 (q, k [B*H][N][72 or 96],
// v [B*H][N][72]; entry dmvae_attention_heads_stream_bf16): K / V tiles of 256-B rows in the layouts the 96-wide resident kernel uses (attention_common.h att_kslot<256> /
// att_vslot<256>), 2 x 2 x 16 KiB = 64 KiB static, two staging sweeps per tile (sixteen lanes per key row, nine of them load).  As in the resident kernels the channels
// 72 .. 95 are zeros in LDS and never loaded -- rows padded to 96 by the producer and rows of 72 channels give the same bits --, q k^T takes five 16-channel steps (the
// upper half of the fifth is zero, the sixth is skipped), the output accumulators are three 32-channel blocks and channels >= 72 are not stored.
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): DP = 64: 137 VGPRs, 0 AGPRs, 50 SGPRs, no scratch, no spill, 32 KiB LDS, 3 waves per
// SIMD -- the numbers of the kernel before it was a template.  DP = 96: 186 VGPRs, 0 AGPRs, 56 SGPRs, no scratch, no spill, 64 KiB LDS, 2 waves per SIMD.
#include "attention_common.h"

namespace dmvae_attn_stream {

constexpr int NT = 512;          // 8 waves
constexpr int QW = 32;           // queries per wave
constexpr int KT = ATT_STREAM_TILE;       // keys per tile
template <int DP> using Geo = AttnStreamGeo<DP, NT>;      // attention_common.h; staging sweeps per tile (SW): 1 / 2
constexpr int QB = Geo<64>::BB;  // queries per workgroup: 256

struct StreamArgs {
  const bf16 *q, *k, *v;      // the operand fields, named as attention_common.h says
  bf16* out;
  long long q_bs, q_hs, k_bs, k_hs, v_bs, v_hs;   // elements
  int q_rs, k_rs, v_rs;                           // elements between token rows
  int S, H;
  int nqb;         // query blocks per (sample, head): ceil(S / 256)
  float scale;
  float* lse;      // optional [B * H][S]
};

template <int DP>
__global__ __launch_bounds__(NT) void attention_stream_kernel(StreamArgs a) {
#if __HIP_DEVICE_COMPILE__
  using G = Geo<DP>;
  constexpr int D = G::D, ROW = G::ROW, TILE = G::TILE, KS = G::KS, DB = G::DB, CPR = G::CPR, SW = G::SW;
  __shared__ __attribute__((aligned(256))) char smem[2 * 2 * TILE];     // [buffer][K | V][64 keys][ROW B]
  const int S = a.S;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned item = xcd_remap(blockIdx.x, gridDim.x);
  const int bh = (int)(item / (unsigned)a.nqb), qblk = (int)(item % (unsigned)a.nqb);
  const int b = bh / a.H, h = bh % a.H;
  const bf16* qp = a.q + b * a.q_bs + h * a.q_hs;
  const bf16* kp = a.k + b * a.k_bs + h * a.k_hs;
  const bf16* vp = a.v + b * a.v_bs + h * a.v_hs;
  const int kg = lane >> 5, ql = lane & 31;
  const int q0 = qblk * QB + wave * QW;      // the wave's first query
  const int q = q0 + ql;
  const bool live = q0 < S;                  // wave-uniform
  const int nt = (S + KT - 1) / KT;

  // staging: thread -> key row tid / CPR (+ NT / CPR per sweep) of the tile, 16-B chunk tid % CPR of its K row and of its V row; a chunk past the D real channels
  // is not loaded (zeros in LDS)
  const int skey = tid / CPR, sc = tid % CPR;
  int ksl[SW], vsl[SW];
#pragma unroll
  for (int it = 0; it < SW; it++) { ksl[it] = att_kslot<ROW>(skey + it * (NT / CPR), sc); vsl[it] = att_vslot<ROW>(skey + it * (NT / CPR), sc); }
  uint4 kreg[SW], vreg[SW];
  auto load_tile = [&](int t) {
#pragma unroll
    for (int it = 0; it < SW; it++) {
      const int key = t * KT + skey + it * (NT / CPR);
      kreg[it] = uint4{0, 0, 0, 0}; vreg[it] = uint4{0, 0, 0, 0};
      if (key < S && (DP == 64 || sc < D / 8)) {
        kreg[it] = *reinterpret_cast<const uint4*>(kp + (size_t)key * a.k_rs + sc * 8);
        vreg[it] = *reinterpret_cast<const uint4*>(vp + (size_t)key * a.v_rs + sc * 8);
      }
    }
  };
  auto store_tile = [&](int buf) {
    char* base = smem + buf * 2 * TILE;
#pragma unroll
    for (int it = 0; it < SW; it++) {
      *reinterpret_cast<uint4*>(base + ksl[it]) = kreg[it];
      *reinterpret_cast<uint4*>(base + TILE + vsl[it]) = vreg[it];
    }
  };
  load_tile(0);

  // Q fragments (column operand of the swapped product): 8 channels per lane per 16-channel step
  bf16x8 qf[KS];
#pragma unroll
  for (int kk = 0; kk < KS; kk++) {
    uint4 t = {0, 0, 0, 0};
    if (q < S && (DP == 64 || kk * 16 + kg * 8 < D)) t = *reinterpret_cast<const uint4*>(qp + (size_t)q * a.q_rs + kk * 16 + kg * 8);
    qf[kk] = *reinterpret_cast<bf16x8*>(&t);
  }
  // V transpose-read addressing: attention_common.h's tr_off0 / tr_frag, spelled out (calling them here changes this kernel's instruction stream)
  const int g16 = (lane >> 4) & 1, rr = (lane & 15) >> 2, qq = lane & 3;
  const int voff0 = (kg * 8 + rr) * ROW + ((ROW == 128 ? (rr >> 1) & 1 : rr) << 6) + (16 * g16 + 4 * qq) * 2;
  store_tile(0);

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
    if (live) {
      // ---- S^T = K Q^T for the tile's two 32-key blocks: st[kb][r] = score(key = t*64 + kb*32 + (r&3) + 8*(r>>2) + 4*kg, query q) ----------------------------
      f32x16 st[2];
#pragma unroll
      for (int kb = 0; kb < 2; kb++) {
        bf16x8 kf[KS];     // every fragment read of the block ahead of its products
#pragma unroll
        for (int kk = 0; kk < KS; kk++) kf[kk] = *reinterpret_cast<const bf16x8*>(ks + att_kslot<ROW>(kb * 32 + ql, kk * 2 + kg));
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < 16; r++) st[kb][r] = 0.f;
#pragma unroll
        for (int kk = 0; kk < KS; kk++) st[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[kk], qf[kk], st[kb], 0, 0, 0);
      }
      if (more) load_tile(t + 1);      // in flight under the softmax and the PV products
      if (t * KT + KT > S) {           // the last tile of a ragged S: register r of block kb is key t*64 + kb*32 + (r&3) + 8*(r>>2) + 4*kg
        const int lim = S - t * KT - 4 * kg;
#pragma unroll
        for (int kb = 0; kb < 2; kb++)
#pragma unroll
          for (int r = 0; r < 16; r++) st[kb][r] = kb * 32 + (r & 3) + 8 * (r >> 2) < lim ? st[kb][r] : -INFINITY;
      }
      // ---- online softmax: the tile's maximum (finite: a tile holds a live key), the factor for what is accumulated at the old maximum ------------------------
      float tm = st[0][0];
#pragma unroll
      for (int r = 1; r < 16; r++) tm = fmaxf(tm, st[0][r]);
#pragma unroll
      for (int r = 0; r < 16; r++) tm = fmaxf(tm, st[1][r]);
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
      for (int kb = 0; kb < 2; kb++) {
        // the block's V^T fragments (two 16-key steps x DB 32-channel blocks) are on their way while its exponentials run
        union { bf16x8 v; s16x4 hlf[2]; } vf[2][DB];
#pragma unroll
        for (int half = 0; half < 2; half++)
#pragma unroll
          for (int db = 0; db < DB; db++) {
            vf[half][db].hlf[0] = tr_read_ordered(vs + (kb * 2 + half) * (16 * ROW) + (voff0 ^ (db << 6)));
            vf[half][db].hlf[1] = tr_read_ordered(vs + (kb * 2 + half) * (16 * ROW) + (voff0 ^ (db << 6)) + 4 * ROW);
          }
#pragma unroll
        for (int r = 0; r < 16; r++) { st[kb][r] = __builtin_amdgcn_exp2f(fmaf(st[kb][r], ec, -emc)); l += st[kb][r]; }
#pragma unroll
        for (int half = 0; half < 2; half++) {      // 16-key step kb*2 + half: registers r = half*8 .. half*8+7 of the block
          const unsigned p0 = dmvae_pack_bf16x2(st[kb][half * 8 + 0], st[kb][half * 8 + 1]);
          const unsigned p1 = dmvae_pack_bf16x2(st[kb][half * 8 + 2], st[kb][half * 8 + 3]);
          const unsigned p2 = dmvae_pack_bf16x2(st[kb][half * 8 + 4], st[kb][half * 8 + 5]);
          const unsigned p3 = dmvae_pack_bf16x2(st[kb][half * 8 + 6], st[kb][half * 8 + 7]);
          // lanes < 32 hold keys {0-3, 8-11} of the step, lanes >= 32 {4-7, 12-15}: the fragment wants {0-7} / {8-15} (to_afrag's swaps, spelled out: see there)
          const auto s0 = __builtin_amdgcn_permlane32_swap(p0, p2, false, false);
          const auto s1 = __builtin_amdgcn_permlane32_swap(p1, p3, false, false);
          union { unsigned u[4]; bf16x8 v; } pa;
          pa.u[0] = s0[0]; pa.u[1] = s1[0]; pa.u[2] = s0[1]; pa.u[3] = s1[1];
#pragma unroll
          for (int db = 0; db < DB; db++) o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[half][db].v, pa.v, o[db], 0, 0, 0);
        }
      }
    } else if (more) {
      load_tile(t + 1);
    }
    if (more) store_tile((t + 1) & 1);   // behind this iteration's barrier: nobody reads that buffer any more; visible behind the next one
  }
  if (!live) return;
  l = xhalf_sum(l);                      // the two halves of the query's keys: the same bits in both lanes
  const float inv = 1.f / l;
  if (q < S) {
    if (a.lse && kg == 0) a.lse[(size_t)bh * S + q] = m * a.scale + __logf(l);
    // lane = query q; registers r = 4 r4 .. 4 r4 + 3 are channels db*32 + 8 r4 + 4 kg + 0..3: 8-byte stores
    bf16* orow = a.out + ((size_t)b * S + q) * ((size_t)a.H * D) + h * D;
#pragma unroll
    for (int db = 0; db < DB; db++)
#pragma unroll
      for (int r4 = 0; r4 < 4; r4++) {
        if (DP != 64 && db * 32 + 8 * r4 + 4 * kg >= D) continue;      // D % 8 == 0: the four channels are inside together
        uint2 pk;
        pk.x = dmvae_pack_bf16x2(o[db][4 * r4 + 0] * inv, o[db][4 * r4 + 1] * inv);
        pk.y = dmvae_pack_bf16x2(o[db][4 * r4 + 2] * inv, o[db][4 * r4 + 3] * inv);
        *reinterpret_cast<uint2*>(orow + db * 32 + 8 * r4 + 4 * kg) = pk;
      }
  }
#endif
}

}  // namespace dmvae_attn_stream

extern "C" int dmvae_attention_qkv_stream_bf16(const void* qkv, void* out, void* lse, int batch, int seq, int heads, int head_dim, float scale, hipStream_t stream) {
  using namespace dmvae_attn_stream;
  if (int e = attn_stream_check("attention_qkv_stream_bf16", "qkv or out", qkv && out, ATTN_PACKED, ATTN_FWD, nullptr, nullptr, batch, seq, heads, head_dim, 0, scale, QB)) return e;
  StreamArgs a = {};
  attn_operands_qkv(a, qkv, seq, heads, head_dim);
  a.out = (bf16*)out; a.nqb = attn_row_blocks(seq, QB); a.scale = scale; a.lse = (float*)lse;
  hipLaunchKernelGGL(attention_stream_kernel<64>, dim3((unsigned)(batch * heads * a.nqb)), dim3(NT), 0, stream, a);
  DMVAE_CHECK_LAUNCH();
  return 0;
}

// The same kernel on head-major operands (q, k: [B*H][N][QD], v: [B*H][N][D]; LightningDiT after QK-norm + RoPE: what dmvae_attention_heads_lse_bf16 takes) at any
// token count.  head_dim 64 or 72; QD = head_dim (unpadded rows) or its round-up to 32 (rows zero-padded by the producer): the kernel reads the head_dim real channels
// of a row either way, so both forms give the same bits.
extern "C" int dmvae_attention_heads_stream_bf16(const void* q, const void* k, const void* v, void* out, void* lse, int batch, int seq, int heads, int head_dim,
                                                 int head_dim_padded, float scale, hipStream_t stream) {
  using namespace dmvae_attn_stream;
  if (int e = attn_stream_check("attention_heads_stream_bf16", "q, k, v or out", q && k && v && out, ATTN_HEADS, ATTN_FWD, nullptr, nullptr, batch, seq, heads, head_dim,
                                head_dim_padded, scale, QB)) return e;
  StreamArgs a = {};
  attn_operands_heads(a, q, k, v, seq, heads, head_dim, head_dim_padded);
  a.out = (bf16*)out; a.nqb = attn_row_blocks(seq, QB); a.scale = scale; a.lse = (float*)lse;
  const dim3 grid((unsigned)(batch * heads * a.nqb));
  if (head_dim == 64) hipLaunchKernelGGL(attention_stream_kernel<64>, grid, dim3(NT), 0, stream, a);
  else hipLaunchKernelGGL(attention_stream_kernel<96>, grid, dim3(NT), 0, stream, a);
  DMVAE_CHECK_LAUNCH();
  return 0;
}
