// Device helpers the attention translation units share (t3_attention.hip: bf16 pool, t3_attention_fp8.hip: FP8 E4M3 pool, t3_attention_fp4.hip:
// MXFP4 pool, t3_alignment.hip: the K-only probability tap over any of them): where a head's K / V live in the paged pool, the FP8 and MXFP4
// dequantisation, the RoPE of one lane's eight
// rotation pairs and the wave reductions in the contract's order (DESIGN.md "Attention", "RoPE").  One copy, so every reader runs the same
// addresses, products, roundings and pairings.
#pragma once
#include "t3_kernels.h"
#include "t3_device.h"

namespace t3 {
// ---- paged pool addressing (layouts: t3_attention.hip for bf16, t3_attention_fp8.hip for FP8)
__device__ __forceinline__ size_t kv_head_base(int blk, int kv, int h) {
    return (size_t)blk * KV_BLOCK_ELEMS + (size_t)(kv * H + h) * KV_HEAD_ELEMS;
}
__device__ __forceinline__ int k_piece(int t, int kg) { return 4 * t + kg; }
__device__ __forceinline__ int k_lane_piece(int lane) { return 4 * (lane & 15) + (lane >> 4); }      // the piece lane (t = lane % 16, kg = lane / 16) loads
constexpr int CHUNK8 = CHUNK * HD;      // FP8 pool: bytes of K (or V) of one chunk of one head
__device__ __forceinline__ size_t kv8_head_base(int blk, int kv, int h) {
    return (size_t)blk * KV_BLOCK_ELEMS + (size_t)(kv * H + h) * KV_HEAD_ELEMS;
}
__device__ __forceinline__ int k8_lane_piece(int lane) { return 4 * (lane & 15) + (lane >> 4); }
// ---- FP8 (E4M3FN) -> bf16, exact
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
template <bool HI>
__device__ __forceinline__ uint32_t dq8_pair(uint32_t w) {                           // two e4m3 of the low / high half of w -> packed bf16 pair (exact)
    union { bf16x2 v; uint32_t u; } c;
    c.v = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, HI);
    return c.u;
}
__device__ __forceinline__ uint4 dq8_frag(uint32_t w0, uint32_t w1) {                // eight e4m3 bytes -> one MFMA operand fragment of eight bf16
    return make_uint4(dq8_pair<false>(w0), dq8_pair<true>(w0), dq8_pair<false>(w1), dq8_pair<true>(w1));
}
// ---- MXFP4 pool (layout and format: t3_attention_fp4.hip).  A head's chunk record is CHUNK4 data bytes followed by its 2 * CHUNK scale bytes.
__device__ __forceinline__ size_t kv4_head_base(int blk, int kv, int h) {
    return (size_t)blk * KV4_BLOCK_BYTES + (size_t)(kv * H + h) * KV4_HEAD_BYTES;
}
// E8M0 scale byte -> the fp32 operand of the scaled converts, 2^(b - 127); b = 0 is the fp32 subnormal 2^-127
__device__ __forceinline__ float sc4(uint32_t b) { return __uint_as_float(max((b & 0xffu) << 23, 0x00400000u)); }
template <int SEL>
__device__ __forceinline__ uint32_t dq4_pair(uint32_t w, float scale) {              // the two E2M1 nibbles of byte SEL of w, times scale -> packed bf16 pair (exact)
    union { bf16x2 v; uint32_t u; } c;
    c.v = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, SEL);
    return c.u;
}
__device__ __forceinline__ uint4 dq4_frag(uint32_t w, float scale) {                 // eight nibbles under one scale -> one MFMA operand fragment of eight bf16
    return make_uint4(dq4_pair<0>(w, scale), dq4_pair<1>(w, scale), dq4_pair<2>(w, scale), dq4_pair<3>(w, scale));
}
// K of one chunk as lane (t = lane % 16, kg = lane / 16) holds it: k[j] = the 16-byte piece j (token tiles tt = 2 j, 2 j + 1: words ds = 0, 1 of each),
// ks = the lane's eight scale bytes [tt][ds].  -> the A fragment of (tt, ds): dims 32 ds + 8 kg .. +7 of token 16 tt + t
template <int TT, int DS>
__device__ __forceinline__ uint4 k4_frag(const uint4 (&k)[2], const uint2& ks) {
    const uint4& p = k[TT >> 1];
    const uint32_t w = (TT & 1) ? (DS ? p.w : p.z) : (DS ? p.y : p.x);
    const uint32_t s = (TT >> 1) ? ks.y : ks.x;
    return dq4_frag(w, sc4(s >> (16 * (TT & 1) + 8 * DS)));
}
// RoPE (rotate-half, llama3-scaled table): pairs i in [8*part, 8*part+8):  o1 = x1*c - x2*s, o2 = x2*c + x1*s
// (cos/sin are bf16-valued so both products are exact; one fp32 rounding, then bf16).
__device__ __forceinline__ void rope8(const uint4& x1, const uint4& x2, const float* c, const float* s, uint4& o1, uint4& o2) {
    float a[8], b[8]; unpack8(x1, a); unpack8(x2, b);
    float r1[8], r2[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { r1[e] = a[e] * c[e] - b[e] * s[e]; r2[e] = b[e] * c[e] + a[e] * s[e]; }
    o1.x = pack2(r1[0], r1[1]); o1.y = pack2(r1[2], r1[3]); o1.z = pack2(r1[4], r1[5]); o1.w = pack2(r1[6], r1[7]);
    o2.x = pack2(r2[0], r2[1]); o2.y = pack2(r2[2], r2[3]); o2.z = pack2(r2[4], r2[5]); o2.w = pack2(r2[6], r2[7]);
}
// v[lane ^ off] for off = 32, 16, 8, 4, 2, 1 without the LDS crossbar (ds_bpermute costs a dependent ~100-cycle round trip per
// level): gfx950's half / row swaps for 32 and 16, DPP row rotate / shifts / quad permutes below that.  Same pairing as __shfl_xor,
// so the butterfly sums keep the contract's order.
template <int OFF>
__device__ __forceinline__ float lane_xor(float v, int lane) {
    const int x = __float_as_int(v);
    if constexpr (OFF == 32) {
        const auto r = __builtin_amdgcn_permlane32_swap((unsigned)x, (unsigned)x, false, false);      // r[0] = {lo, lo}, r[1] = {hi, hi}
        return __int_as_float((int)((lane & 32) ? r[0] : r[1]));
    } else if constexpr (OFF == 16) {
        const auto r = __builtin_amdgcn_permlane16_swap((unsigned)x, (unsigned)x, false, false);      // r[0] = even rows twice, r[1] = odd rows twice
        return __int_as_float((int)((lane & 16) ? r[0] : r[1]));
    } else if constexpr (OFF == 8) {
        return __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0x128, 0xf, 0xf, true));              // row_ror:8
    } else if constexpr (OFF == 4) {
        const int up = __builtin_amdgcn_update_dpp(0, x, 0x104, 0xf, 0xf, true), dn = __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, true);   // row_shl:4 (from lane + 4), row_shr:4 (from lane - 4)
        return __int_as_float((lane & 4) ? dn : up);
    } else if constexpr (OFF == 2) {
        return __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0x4E, 0xf, 0xf, true));               // quad_perm [2,3,0,1]
    } else {
        return __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0xB1, 0xf, 0xf, true));               // quad_perm [1,0,3,2]
    }
}
__device__ __forceinline__ float wave_max_f32(float m, int lane) {
    m = fmaxf(m, lane_xor<32>(m, lane)); m = fmaxf(m, lane_xor<16>(m, lane)); m = fmaxf(m, lane_xor<8>(m, lane));
    m = fmaxf(m, lane_xor<4>(m, lane)); m = fmaxf(m, lane_xor<2>(m, lane)); m = fmaxf(m, lane_xor<1>(m, lane));
    return m;
}
template <int OFF>
__device__ __forceinline__ uint32_t lane_xor_u32(uint32_t v, int lane) { return __float_as_uint(lane_xor<OFF>(__uint_as_float(v), lane)); }
// max over the wave of a u64 key (hi, lo), in every lane: the butterfly of wave_max_f32 on both halves (t3_guard.hip, t3_logprobs.hip)
template <int OFF>
__device__ __forceinline__ void key_max_step(uint32_t& hi, uint32_t& lo, int lane) {
    const uint32_t ohi = lane_xor_u32<OFF>(hi, lane), olo = lane_xor_u32<OFF>(lo, lane);
    const bool take = ohi > hi || (ohi == hi && olo > lo);
    hi = take ? ohi : hi; lo = take ? olo : lo;
}
__device__ __forceinline__ void wave_max_key(uint32_t& hi, uint32_t& lo, int lane) {
    key_max_step<32>(hi, lo, lane); key_max_step<16>(hi, lo, lane); key_max_step<8>(hi, lo, lane);
    key_max_step<4>(hi, lo, lane); key_max_step<2>(hi, lo, lane); key_max_step<1>(hi, lo, lane);
}
__device__ __forceinline__ float wave_bfly_add_f32(float v, int lane) {      // contract order: xor 32, 16, 8, 4, 2, 1
    v = v + lane_xor<32>(v, lane); v = v + lane_xor<16>(v, lane); v = v + lane_xor<8>(v, lane);
    v = v + lane_xor<4>(v, lane); v = v + lane_xor<2>(v, lane); v = v + lane_xor<1>(v, lane);
    return v;
}
}  // namespace t3
