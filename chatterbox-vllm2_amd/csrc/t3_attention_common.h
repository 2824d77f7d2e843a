// Device helpers the two attention translation units share (t3_attention.hip: bf16 pool, t3_attention_fp8.hip: FP8 E4M3 pool): the RoPE of
// one lane's eight rotation pairs and the wave reductions in the contract's order (DESIGN.md "Attention", "RoPE").  One copy, so both
// storage formats run the same products, roundings and pairings.
#pragma once
#include "t3_device.h"

namespace t3 {
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
__device__ __forceinline__ float wave_bfly_add_f32(float v, int lane) {      // contract order: xor 32, 16, 8, 4, 2, 1
    v = v + lane_xor<32>(v, lane); v = v + lane_xor<16>(v, lane); v = v + lane_xor<8>(v, lane);
    v = v + lane_xor<4>(v, lane); v = v + lane_xor<2>(v, lane); v = v + lane_xor<1>(v, lane);
    return v;
}
}  // namespace t3
