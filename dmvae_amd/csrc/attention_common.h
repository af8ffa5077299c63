// What the four attention sources share (attention.hip, attention_bwd.hip: a head resident in LDS; attention_stream.hip, attention_bwd_stream.hip: 64-row tiles):
// the operand geometry and its two host recipes, the entries' shared argument checks, and the device helpers that only attention uses.
#pragma once
#include "common.h"
#include <math.h>

constexpr int ATT_RESIDENT_KEYS = 288;      // tokens the resident kernels hold in LDS (nine 32-key blocks); beyond it ops.py (ATTENTION_RESIDENT_MAX) takes the streaming kernels
constexpr int ATT_STREAM_TILE = 64;         // rows per streamed tile

// The operand fields, spelled alike in every attention kernel's argument struct (A below):
//   const bf16 *q, *k, *v;  long long q_bs, q_hs, k_bs, k_hs, v_bs, v_hs;  int q_rs, k_rs, v_rs;  int S, H;          and, backward,  bf16 *dq, *dk, *dv;
// per-(sample, head) base = ptr + b * bs + h * hs (elements), token rows `rs` elements apart; dq / dk / dv in the geometry of q / k / v.  NOT one base struct the four
// inherit from: that moves each kernel's extras behind the base in its argument segment, the argument loads merge differently and all eighteen kernels' instruction
// streams change (profiles/r14_attention_refactor_isa.txt).  Each struct keeps its layout; the recipes below are the one place that knows what the fields hold.
// ---- the two operand recipes -----------------------------------------------------------------------------------------------------------------------------
// packed: the qkv Linear's output [B][S][3][H][D]
template <class A> static inline void attn_operands_qkv(A& a, const void* qkv, int seq, int heads, int head_dim) {
  const long long C = (long long)heads * head_dim;
  a.q = (const bf16*)qkv; a.k = a.q + C; a.v = a.q + 2 * C;
  a.q_bs = a.k_bs = a.v_bs = (long long)seq * 3 * C; a.q_hs = a.k_hs = a.v_hs = head_dim;
  a.q_rs = a.k_rs = a.v_rs = (int)(3 * C);
  a.S = seq; a.H = heads;
}
template <class A> static inline void attn_grads_qkv(A& g, void* dqkv, int heads, int head_dim) {
  g.dq = (bf16*)dqkv; g.dk = g.dq + (long long)heads * head_dim; g.dv = g.dk + (long long)heads * head_dim;
}
// head-major: q, k [B*H][S][head_dim_padded], v [B*H][S][head_dim] (what dmvae_qknorm_rope_bf16 writes)
template <class A> static inline void attn_operands_heads(A& a, const void* q, const void* k, const void* v, int seq, int heads, int head_dim, int head_dim_padded) {
  a.q = (const bf16*)q; a.k = (const bf16*)k; a.v = (const bf16*)v;
  a.q_hs = a.k_hs = (long long)seq * head_dim_padded; a.q_bs = a.k_bs = a.q_hs * heads;
  a.v_hs = (long long)seq * head_dim; a.v_bs = a.v_hs * heads;
  a.q_rs = a.k_rs = head_dim_padded; a.v_rs = head_dim;
  a.S = seq; a.H = heads;
}
template <class A> static inline void attn_grads_heads(A& g, void* dq, void* dk, void* dv) { g.dq = (bf16*)dq; g.dk = (bf16*)dk; g.dv = (bf16*)dv; }

// ---- argument checks: `name` is the entry's short name, the prefix of its messages; 0 (or a width), or -22 with dmvae_last_error() set --------------------------
// The resident head-major entries' shape condition.  q / k rows: head_dim_padded channels -- 64 / 96 (zero-padded by the producer), or head_dim itself (no padding in
// memory; the kernels' 96-wide products see zeros).  Returns the staged width, 64 or 96.
static inline int attn_resident_heads_check(const char* name, int seq, int head_dim, int head_dim_padded) {
  const int dpc = (head_dim_padded + 31) / 32 * 32;
  DMVAE_CHECK_ARG(seq <= ATT_RESIDENT_KEYS && head_dim % 8 == 0 && head_dim <= head_dim_padded && (head_dim_padded == 64 || head_dim_padded == 96 || head_dim_padded == head_dim) &&
                  (dpc == 64 || dpc == 96),
                  "%s: needs seq <= %d, head_dim %% 8 == 0, q / k rows of 64, 96 or head_dim <= 96 channels (got %d, %d, %d)", name, ATT_RESIDENT_KEYS, seq, head_dim, head_dim_padded);
  return dpc;
}
// The scale every attention entry takes: the forward kernels fold it into the exponent of a base-2 power next to the row maximum of the RAW scores
// (exp(scale (s - m)) with m = max s), which is the softmax only for scale > 0
static inline int attn_scale_check(const char* name, float scale) {
  DMVAE_CHECK_ARG(scale > 0.f && isfinite(scale), "%s: needs a finite scale > 0 (got %g)", name, (double)scale);
  return 0;
}
// Row blocks per (sample, head) of a streaming kernel whose workgroups own `rows` rows: ceil(seq / rows), for any seq an int holds
static inline int attn_row_blocks(int seq, int rows) { return (int)(((long long)seq + rows - 1) / rows); }
// The four streaming entries' checks in their one order.  have: every operand pointer is non-null (`operands` lists them for the message); packed: one qkv tensor
// (head dim 64; head_dim_padded unused) or head-major q / k / v (head dim 64 or 72, q / k rows head_dim_padded wide); bwd: lse and delta are required as well;
// block_rows: the rows a workgroup of the entry's smallest-block kernel owns -- its grid is the one that has to fit.
constexpr bool ATTN_PACKED = true, ATTN_HEADS = false, ATTN_FWD = false, ATTN_BWD = true;      // the call sites' words for `packed` and `bwd`
static inline int attn_stream_check(const char* name, const char* operands, bool have, bool packed, bool bwd, const void* lse, const void* delta, int batch, int seq, int heads,
                                    int head_dim, int head_dim_padded, float scale, int block_rows) {
  DMVAE_CHECK_ARG(have, "%s: null %s", name, operands);
  DMVAE_CHECK_ARG(!bwd || lse, "%s: null lse (the forward's row statistics are required)", name);
  DMVAE_CHECK_ARG(!bwd || delta, "%s: null delta scratch (batch * heads * seq floats)", name);
  DMVAE_CHECK_ARG(batch > 0 && heads > 0 && seq >= 1, "%s: needs batch, heads, seq >= 1 (got %d, %d, %d)", name, batch, heads, seq);
  DMVAE_CHECK_ARG(head_dim == 64 || (!packed && head_dim == 72), packed ? "%s: needs head_dim 64 (got %d)" : "%s: needs head_dim 64 or 72 (got %d)", name, head_dim);
  DMVAE_CHECK_ARG(packed || head_dim_padded == head_dim || head_dim_padded == (head_dim + 31) / 32 * 32,
                  "%s: q / k rows hold head_dim channels or head_dim rounded up to 32 (got %d for head_dim %d)", name, head_dim_padded, head_dim);
  if (attn_scale_check(name, scale)) return -22;
  // the row stride (packed: 3 C) and the (sample, head) count are ints in the kernels; the flat grid is one dimension
  const long long bh = (long long)batch * heads, blocks = bh * attn_row_blocks(seq, block_rows);
  DMVAE_CHECK_ARG((!packed || 3LL * heads * head_dim <= 0x7fffffffLL) && bh <= 0x7fffffffLL && blocks <= 0x7fffffffLL,
                  "%s: %d x %d heads x %d tokens does not fit the grid", name, batch, heads, seq);
  return 0;
}

// ---- LDS images of the K and V tiles (resident forward: a whole head; streaming kernels: 64-row tiles), byte offset of 16-B chunk c of row `key` ----------------------
// ROW: bytes per row, 128 (head dim 64) or 256 (96).
// K is read row-wise by ds_read_b128, which is served in four groups of sixteen lanes that are NOT consecutive ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ... --
// MI355X_MICROARCH.md, LDS table), each lane reading key (lane & 31)'s chunk: the sixteen slots of a group must be distinct mod 256 B.  256-B rows: XOR with
// key & 15 (sixteen distinct values in every group).  128-B rows (two keys per 256 B): XOR with (key >> 1) & 7 -- eight values, each met by one even and one odd key
// of the group.  (XOR with key & 7, which every group holds twice, was a 2-way conflict on every K read: SQ_LDS_BANK_CONFLICT 37 % of the LDS cycles.)
template <int ROW>
__device__ __forceinline__ int att_kslot(int key, int c) { return key * ROW + ((c ^ (ROW == 128 ? (key >> 1) & 7 : key & 15)) << 4); }
// V is read by ds_read_b64_tr_b16: channel chunk c (8 channels) -> 64-B segment c >> 2, swizzled per key; 16-B slot c & 3 inside it.  128-B rows: two segments swizzled
// by (key >> 1) & 1 -- the four key rows a transpose-read pass touches then sit in four distinct 64-B bank slots of the 256-B LDS row; 256-B rows: four, by key & 3.
template <int ROW>
__device__ __forceinline__ int att_vslot(int key, int c) {
  return ROW == 128 ? key * 128 + ((((c >> 2) ^ ((key >> 1) & 1))) << 6) + ((c & 3) << 4) : key * 256 + ((((c >> 2) ^ (key & 3))) << 6) + ((c & 3) << 4);
}
// transpose-read addressing in an att_vslot image: the lane supplies 4 channels of row 8 kg + rr (and + 4) of a 16-row step; channel block db is the 64-B segment
// db ^ swizzle, so another block's address is the first's with db << 6 XOR-ed in (one address register; the bits below 6 and the row offset above them do not overlap
// the segment bits)
template <int ROW>
__device__ __forceinline__ int tr_off0(int lane) {
  const int kg = lane >> 5, g16 = (lane >> 4) & 1, rr = (lane & 15) >> 2, qq = lane & 3;
  return (kg * 8 + rr) * ROW + ((ROW == 128 ? (rr >> 1) & 1 : rr) << 6) + (16 * g16 + 4 * qq) * 2;
}
template <int ROW>
__device__ __forceinline__ bf16x8 tr_frag(const char* img, int step16, int off0, int db) {
  union { bf16x8 v; s16x4 hlf[2]; } f;
  f.hlf[0] = tr_read_ordered(img + step16 * (16 * ROW) + (off0 ^ (db << 6)));
  f.hlf[1] = tr_read_ordered(img + step16 * (16 * ROW) + (off0 ^ (db << 6)) + 4 * ROW);
  return f.v;
}

// Tile geometry of the streaming kernels.  DP: head dim as staged.  64: head dim 64, 128-B rows in LDS.  96: head dim 72 (LightningDiT-XL), 256-B rows -- the layouts
// of the 96-wide resident kernel; the channels 72 .. 95 are zeros in LDS (never loaded), the sixth 16-channel step of the products over channels is skipped, the upper
// half of the fifth is zero, columns >= 72 of the results are not stored.  NT: threads of the workgroup.
template <int DP, int NT> struct AttnStreamGeo {
  static_assert(DP == 64 || DP == 96, "staged head dim 64 or 96");
  static constexpr int D = DP == 64 ? 64 : 72;          // real head dim: v / out / dout width, the channels of a q / k row that are read
  static constexpr int ROW = DP == 64 ? 128 : 256;      // bytes per row in LDS
  static constexpr int TILE = ATT_STREAM_TILE * ROW;    // 8 / 16 KiB
  static constexpr int KS = DP == 64 ? 4 : 5;           // 16-channel steps of the products over channels
  static constexpr int DB = DP / 32;                    // 32-channel blocks of the accumulators
  static constexpr int CPR = ROW / 16;                  // staging lanes per row: one 16-B chunk each
  static constexpr int SW = ATT_STREAM_TILE * CPR / NT; // staging sweeps per tile
  static constexpr int BB = 32 * NT / 64;               // rows a workgroup owns: 32 per wave
};

// max / sum of a value with its partner in lane ^ 32 (the other half of a query's keys); both lanes get the same bits
__device__ __forceinline__ float xhalf_max(float x) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float xhalf_sum(float x) {    // r[0] is the low half's value in both lanes, r[1] the high half's: low + high everywhere
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// ---- the backward kernels' fragment helpers ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float dot8(const uint4& a, const uint4& b) {
  const bf16x8 x = *reinterpret_cast<const bf16x8*>(&a), y = *reinterpret_cast<const bf16x8*>(&b);
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 8; e++) s += (float)x[e] * (float)y[e];
  return s;
}
// C-layout registers of a 32 x 32 block (row (r & 3) + 8 (r >> 2) + 4 (lane >> 5), column lane & 31), 16 of them scaled to bf16 -> the two A fragments
// (reduction index = the block's ROW, 8 consecutive per lane) of its two 16-row halves.  The two forward kernels spell the same swaps out inside their PV loops:
// calling this there costs registers (streaming: 137 -> 142 VGPRs at 64, 186 -> 187 at 96; resident: + 4 in all five forms, 104 -> 108 at 64), so those two sites stay as they are.
__device__ __forceinline__ void to_afrag(const f32x16& c, bf16x8 out[2]) {
#pragma unroll
  for (int half = 0; half < 2; half++) {
    const unsigned p0 = dmvae_pack_bf16x2(c[half * 8 + 0], c[half * 8 + 1]), p1 = dmvae_pack_bf16x2(c[half * 8 + 2], c[half * 8 + 3]);
    const unsigned p2 = dmvae_pack_bf16x2(c[half * 8 + 4], c[half * 8 + 5]), p3 = dmvae_pack_bf16x2(c[half * 8 + 6], c[half * 8 + 7]);
    // lanes < 32 hold rows {0-3, 8-11} of the half, lanes >= 32 rows {4-7, 12-15}: the fragment wants {0-7} / {8-15}
    const auto s0 = __builtin_amdgcn_permlane32_swap(p0, p2, false, false);
    const auto s1 = __builtin_amdgcn_permlane32_swap(p1, p3, false, false);
    union { unsigned u[4]; bf16x8 v; } pa;
    pa.u[0] = s0[0]; pa.u[1] = s1[0]; pa.u[2] = s0[1]; pa.u[3] = s1[1];
    out[half] = pa.v;
  }
}
