// The MXFP4 (OCP microscaling: E2M1 elements, one E8M0 scale per 32) form of the paged KV pool for gfx950 (MI355X, CDNA4): RoPE + quantise +
// paged write, the fused decode attention, the 16-rows-per-workgroup prefill attention, the read-back hook and the format hook.  Opt-in
// (T3EngineConfig.kv_cache_dtype = 4); the bf16 and FP8 pools and their kernels are untouched.
//
// Numerics contract (DESIGN.md "Attention", MXFP4 pool).  One MX block = 32 consecutive head dims of ONE token of one head (a head's 64 dims
// are two blocks; never along tokens: tokens arrive one at a time and a stored block is never requantised).  For the bf16 value x the bf16
// pool would hold (K after RoPE and its bf16 rounding, V as it arrives):
//     amax = max |x| over the block,  E = amax's biased exponent field,  b = max(E - 2, 0) (the E8M0 byte),  X = 2^(b - 127)
//     stored element = E2M1(rne(x / X)) saturating at +-6, the sign of zero kept;   dq(x) = X * element
// Every dq(x) is a bf16 value: the kernels dequantise to bf16 in registers and run the bf16 chain on it (v_mfma_f32_16x16x32_bf16, 64-token
// chunks, softmax, butterfly order, bf16 p, ascending chunk fold), so the output is bit for bit the bf16 contract's result over the
// dequantised K / V.  The scaled f8f6f4 MFMA is not used: it would force q and p out of bf16.  Compile with -ffp-contract=off.
//
// Quantisation is integer / fp32 VALU whose comparisons spell the rounding out (one token per launch: not hot); dequantisation, which runs
// in front of every MFMA, is v_cvt_scalef32_pk_bf16_fp4 (dq4_pair(), t3_attention_common.h).  Both are pinned by the format hook's test.
#include "t3_kernels.h"
#include "t3_device.h"
#include "t3_attention_common.h"

#include <math.h>
#include <type_traits>

namespace t3 {
// ------------------------------------------------------------------------------------------------
// Quantise.  x / X is exact in fp32 (a power of two; |x| / X < 8), so the seven comparisons ARE round-to-nearest-even onto
// {0, .5, 1, 1.5, 2, 3, 4, 6}: a tie goes to the code with the even mantissa bit (codes 0, 2, 4, 6), everything above 5 saturates to 6.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t amax_bits(float x) { return __float_as_uint(x) & 0x7fffffffu; }
__device__ __forceinline__ uint32_t e8m0_of(uint32_t amax) { const int E = (int)(amax >> 23); return (uint32_t)max(E - 2, 0); }
__device__ __forceinline__ uint32_t q4_one(float x, uint32_t b) {                     // -> the E2M1 nibble of x under scale byte b
    const uint32_t u = __float_as_uint(x), mag = u & 0x7fffffffu;
    // a = |x| / X.  A subnormal x goes through its integer mantissa, so the result does not depend on the denormal mode
    const float a = (mag >> 23) == 0 ? (float)(int)mag * __uint_as_float((uint32_t)max(105 - (int)b, 1) << 23)
                                     : __uint_as_float(mag) * __uint_as_float((254u - b) << 23);
    const uint32_t c = (uint32_t)(a > 0.25f) + (uint32_t)(a >= 0.75f) + (uint32_t)(a > 1.25f) + (uint32_t)(a >= 1.75f) +
                       (uint32_t)(a > 2.5f) + (uint32_t)(a >= 3.5f) + (uint32_t)(a > 5.0f);
    return ((u >> 28) & 8u) | c;
}
__device__ __forceinline__ uint32_t amax8(const float* f) {
    uint32_t m = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) m = max(m, amax_bits(f[e]));
    return m;
}
__device__ __forceinline__ uint32_t q4_x8(const float* f, uint32_t b) {              // eight values -> one word, f[0] in the lowest nibble
    uint32_t w = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) w |= q4_one(f[e], b) << (4 * e);
    return w;
}
__device__ __forceinline__ uint32_t dq4_one(uint32_t nib, uint32_t b) { return dq4_pair<0>(nib & 0xfu, sc4(b)) & 0xffffu; }      // one nibble -> bf16 bits

// parity hook: y = the stored value of x over whole blocks of 32, lane = element (a wave holds two blocks)
__global__ __launch_bounds__(256) void fp4_roundtrip_kernel(const float* x, float* y, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const float v = i < n ? x[i] : 0.0f;                      // n is a multiple of 32: a block is whole or absent
    uint32_t m = amax_bits(v);
    m = max(m, lane_xor_u32<16>(m, lane)); m = max(m, lane_xor_u32<8>(m, lane)); m = max(m, lane_xor_u32<4>(m, lane));
    m = max(m, lane_xor_u32<2>(m, lane)); m = max(m, lane_xor_u32<1>(m, lane));
    const uint32_t b = e8m0_of(m);
    if (i < n) y[i] = bf2f((uint16_t)dq4_one(q4_one(v, b), b));
}
hipError_t launch_fp4_roundtrip(const float* x, float* y, int n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (n % 32) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fp4_roundtrip_kernel, dim3((n + 255) / 256), dim3(256), 0, s, x, y, n);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Paged layout of one (block, head): [chunk-in-block] records of CHUNK4_REC = 2048 + 128 bytes for K and for V (17 cache lines; a token is
// 2 x 16 x 34 = 1088 bytes per layer).  A chunk is 2 + 2 fully coalesced 1 KiB wave loads plus one scale load each (the FP8 pool: 4 + 4).
//   K data, piece j (tokens 32 j .. +31), lane (t, kg), 16 bytes at index 4 t + kg (token-major, as the other pools):
//     word 2 u + ds = K[token 32 j + 16 u + t][dims 32 ds + 8 kg .. +7], dim 8 kg + e in nibble e: each word is one MFMA A-fragment octet.
//     A token's 32 data bytes are four 8-byte halves of ONE 64-byte group.
//   K scales, at 2048: byte 8 t + 2 tt + ds = the scale of (token 16 tt + t, block ds): lane (t, kg) gets its eight scales with one 8-byte load.
//     The token's two scale bytes sit in the chunk's 17th line, not in the line of its data: 64 tokens x 34 bytes do not fit 17 lines as
//     whole tokens (three per line at most).  The newest K is therefore two stores into one 2176-byte record.
//   V data, piece j (dims 32 j .. +31), lane (d, kg), 16 bytes at index d + 16 kg:
//     word 2 u + ts = V[tokens 32 ts + 8 kg .. +7][dim 32 j + 16 u + d], token 8 kg + e in nibble e (A fragments of dt = 2 j + u).
//   V scales, at 2048: byte 2 token + g = the scale of (token, dims 32 g .. +31): lane = token reads its pair in the softmax phase.
// The head regions keep KV_HEAD_PAD = 512 elements (here 256 bytes) between them: 8960 bytes per head.  The value is carried over from
// the bf16 pool, not measured for half-byte elements.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ size_t chunk4_base(int tok_in_block) { return (size_t)(tok_in_block / CHUNK) * CHUNK4_REC; }
__device__ __forceinline__ int k4_off(int tc, int kg) { return (tc >> 5) * 1024 + (4 * (tc & 15) + kg) * 16 + ((tc >> 4) & 1) * 8; }      // the 8-byte half (ds = 0, 1) of token-in-chunk tc
__device__ __forceinline__ int k4s_off(int tc) { return CHUNK4 + 8 * (tc & 15) + 2 * (tc >> 4); }                                       // its two scale bytes
__device__ __forceinline__ int v4_off(int tc, int dim) {                                                                                // the WORD that holds (tc, dim); nibble tc & 7
    return (dim >> 5) * 1024 + ((dim & 15) + 16 * ((tc & 31) >> 3)) * 16 + (((dim >> 4) & 1) * 2 + (tc >> 5)) * 4;
}
__device__ __forceinline__ int v4s_off(int tc) { return CHUNK4 + 2 * tc; }

// RoPE + quantise + paged write: one wave per row, lane = 4 * head + part as rope_kv_kernel.  The lane's two rotated K octets are the two
// words of its 8-byte half; a block's amax is an exchange inside the quad (DPP, no LDS).
// V is token-minor with EIGHT tokens per word, so two rows of a launch may own nibbles of one word: per aligned group of eight positions
// the wave of the group's FIRST row in the launch (the leader) quantises every row of the group the launch holds and merges their nibbles
// into the words (read-modify-write where the group is ragged: positions written by an earlier launch stay); the other waves skip V.
// A stream's rows are consecutive in a launch (the scheduler's runs; the hooks'), so a group has one leader.
__global__ __launch_bounds__(256) void rope_kv_fp4_kernel(RopeArgs a) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.rows) return;
    uint8_t* kv = reinterpret_cast<uint8_t*>(a.kv_layer);
    const int* rec = a.rowrec + (size_t)row * a.row_stride;
    const int pos = rec[1];
    const int blk = rec[ROW_HDR + pos / KV_BLOCK], tok = pos % KV_BLOCK, tc = tok % CHUNK;
    const int h = lane >> 2, part = lane & 3, i0 = part * 8;
    float c[8], s[8];
    {
        const float4* cp = reinterpret_cast<const float4*>(a.cos_t + (size_t)pos * 32 + i0);
        const float4* sp = reinterpret_cast<const float4*>(a.sin_t + (size_t)pos * 32 + i0);
        const float4 c0 = cp[0], c1 = cp[1], s0 = sp[0], s1 = sp[1];
        c[0] = c0.x; c[1] = c0.y; c[2] = c0.z; c[3] = c0.w; c[4] = c1.x; c[5] = c1.y; c[6] = c1.z; c[7] = c1.w;
        s[0] = s0.x; s[1] = s0.y; s[2] = s0.z; s[3] = s0.w; s[4] = s1.x; s[5] = s1.y; s[6] = s1.z; s[7] = s1.w;
    }
    const uint16_t* qr = a.qkv + (size_t)row * QKV;
    uint4 o1, o2;
    rope8(*reinterpret_cast<const uint4*>(qr + h * 64 + i0), *reinterpret_cast<const uint4*>(qr + h * 64 + 32 + i0), c, s, o1, o2);
    uint16_t* qo = a.q_out + (size_t)row * D + h * 64;
    *reinterpret_cast<uint4*>(qo + i0) = o1; *reinterpret_cast<uint4*>(qo + 32 + i0) = o2;
    rope8(*reinterpret_cast<const uint4*>(qr + D + h * 64 + i0), *reinterpret_cast<const uint4*>(qr + D + h * 64 + 32 + i0), c, s, o1, o2);
    {
        float f1[8], f2[8]; unpack8(o1, f1); unpack8(o2, f2);
        uint32_t m1 = amax8(f1), m2 = amax8(f2);
        m1 = max(m1, lane_xor_u32<1>(m1, lane)); m1 = max(m1, lane_xor_u32<2>(m1, lane));
        m2 = max(m2, lane_xor_u32<1>(m2, lane)); m2 = max(m2, lane_xor_u32<2>(m2, lane));
        const uint32_t b1 = e8m0_of(m1), b2 = e8m0_of(m2);
        uint8_t* Kb = kv + kv4_head_base(blk, 0, h) + chunk4_base(tok);
        *reinterpret_cast<uint2*>(Kb + k4_off(tc, part)) = make_uint2(q4_x8(f1, b1), q4_x8(f2, b2));
        if (part == 0) *reinterpret_cast<uint16_t*>(Kb + k4s_off(tc)) = (uint16_t)(b1 | (b2 << 8));
    }
    // ---- V: the leader of the row's group of eight positions
    const int p8 = pos & 7;
    int prev_ok = 0, mine = 0;
    if (lane == 0 && row > 0) { const int* r0 = rec - a.row_stride; prev_ok = (r0[0] == rec[0]) && (r0[1] == pos - 1); }
    if (lane < 8 - p8 && row + lane < a.rows) { const int* r2 = rec + (size_t)lane * a.row_stride; mine = (r2[0] == rec[0]) && (r2[1] == pos + lane); }
    if (p8 != 0 && __builtin_amdgcn_readfirstlane(prev_ok)) return;
    const int n = __builtin_ctzll(~__ballot(mine));           // rows of the group this launch holds, from this one on: 1 .. 8 - p8
    const uint32_t keep = ~(uint32_t)(((1ull << (4 * n)) - 1ull) << (4 * p8));      // nibbles of the group's other positions
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int pc = lane + 64 * u, hh = pc >> 3, oct = pc & 7, g = oct >> 2;      // (head, dims 8 oct .. +7): block g, four lanes per block
        uint8_t* Vb = kv + kv4_head_base(blk, 1, hh) + chunk4_base(tok);
        uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (i < n) {
                float f[8]; unpack8(*reinterpret_cast<const uint4*>(a.qkv + (size_t)(row + i) * QKV + 2 * D + hh * 64 + oct * 8), f);
                uint32_t m = amax8(f);
                m = max(m, lane_xor_u32<1>(m, lane)); m = max(m, lane_xor_u32<2>(m, lane));
                const uint32_t b = e8m0_of(m);
                if ((oct & 3) == 0) Vb[v4s_off(tc + i) + g] = (uint8_t)b;
#pragma unroll
                for (int d = 0; d < 8; ++d) w[d] |= q4_one(f[d], b) << (4 * (p8 + i));
            }
        }
#pragma unroll
        for (int d = 0; d < 8; ++d) {
            uint32_t* dst = reinterpret_cast<uint32_t*>(Vb + v4_off(tc, oct * 8 + d));
            *dst = keep ? ((*dst & keep) | w[d]) : w[d];
        }
    }
}
hipError_t launch_rope_kv_fp4(const RopeArgs& a, hipStream_t s) {
    if (a.rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(rope_kv_fp4_kernel, dim3((a.rows + 3) / 4), dim3(256), 0, s, a);
    return hipGetLastError();
}
// parity hook: the stored K / V of a row's (stream, position), dequantised to bf16 -> out [rows][2][1024]; one wave per row, lane = (head, part)
__global__ __launch_bounds__(256) void kv_gather_fp4_kernel(const uint8_t* kv, const int* rowrec, int row_stride, int rows, uint16_t* out) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int* rec = rowrec + (size_t)row * row_stride;
    const int pos = rec[1], blk = rec[ROW_HDR + pos / KV_BLOCK], tok = pos % KV_BLOCK, tc = tok % CHUNK;
    const int h = lane >> 2, part = lane & 3;
    const uint8_t* Kb = kv + kv4_head_base(blk, 0, h) + chunk4_base(tok);
    const uint8_t* Vb = kv + kv4_head_base(blk, 1, h) + chunk4_base(tok);
    uint16_t* ko = out + (size_t)row * 2 * D + h * HD;
    uint16_t* vo = ko + D;
    const uint2 p = *reinterpret_cast<const uint2*>(Kb + k4_off(tc, part));
    const uint32_t ks = *reinterpret_cast<const uint16_t*>(Kb + k4s_off(tc));
    *reinterpret_cast<uint4*>(ko + part * 8) = dq4_frag(p.x, sc4(ks));
    *reinterpret_cast<uint4*>(ko + 32 + part * 8) = dq4_frag(p.y, sc4(ks >> 8));
    const uint32_t vs = Vb[v4s_off(tc) + (part >> 1)];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(Vb + v4_off(tc, part * 16 + e));
        vo[part * 16 + e] = (uint16_t)dq4_one(w >> (4 * (tc & 7)), vs);
    }
}
hipError_t launch_kv_gather_fp4(const uint16_t* kv_layer, const int* rowrec, int row_stride, int rows, uint16_t* out, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(kv_gather_fp4_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, reinterpret_cast<const uint8_t*>(kv_layer), rowrec, row_stride, rows, out);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// V in front of the P.V MFMAs.  A lane's octet spans eight tokens, i.e. eight scales, and a packed convert takes one.  The power-of-two scale
// of (token, dim group g = dt / 2) is therefore folded into the replicated bf16 p operand: p_g[token] = p[token] * 2^(b - 127), an exponent
// add on p's bits, two p variants per chunk, and the A operand is the raw E2M1 value (converts under scale 1).  e * (p 2^k) and (e 2^k) * p are
// the same real product, exact in fp32 either way, PROVIDED every operand is a normal bf16: p is 0 or in [2^-100, 1], so p 2^k can leave
// the normal range (k < -26), and e 2^k is subnormal for b < 2.  That is checked, not assumed: a lane whose token has p != 0 and
// (b < 2 or p's exponent field + b < 128) for either group votes the whole chunk onto the element-wise path, which converts every nibble
// under its own token's scale (two converts and a merge per pair) against the plain p.  p 2^k <= 2^125 never overflows.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool fold_unsafe(uint32_t pb, uint32_t b0, uint32_t b1) {
    const uint32_t bm = min(b0, b1);
    return pb != 0 && (bm < 2 || (pb >> 7) + bm < 128);
}
__device__ __forceinline__ uint32_t fold_p(uint32_t pb, uint32_t b) { return pb ? (uint32_t)((int)pb + (((int)b - 127) << 7)) : 0u; }
// element-wise: word w = eight tokens of one dim, sc = the eight tokens' scale pairs (16 bits each: g = 0 low byte, g = 1 high byte)
template <int G>
__device__ __forceinline__ uint4 dq4_frag_tokens(uint32_t w, const uint4& sc) {
    auto pr = [&](uint32_t s2, auto sel) {
        constexpr int SEL = decltype(sel)::value;
        return (dq4_pair<SEL>(w, sc4(s2 >> (8 * G))) & 0xffffu) | (dq4_pair<SEL>(w, sc4(s2 >> (16 + 8 * G))) & 0xffff0000u);
    };
    return make_uint4(pr(sc.x, std::integral_constant<int, 0>{}), pr(sc.y, std::integral_constant<int, 1>{}),
                      pr(sc.z, std::integral_constant<int, 2>{}), pr(sc.w, std::integral_constant<int, 3>{}));
}
__device__ __forceinline__ uint32_t v4_word(const uint4 (&v)[2], int dt, int ts) {      // compile-time dt, ts after unrolling
    const uint4& p = v[dt >> 1];
    return (dt & 1) ? (ts ? p.w : p.z) : (ts ? p.y : p.x);
}

// ------------------------------------------------------------------------------------------------
// Paged attention for one (row, head) over the MXFP4 pool.  Work split, LDS partials and the fold over chunks are attention_kernel's (one
// workgroup of NW waves, wave w takes chunks w, w + NW, ...).  A raw chunk tile is 2 K + 2 V pieces, 8 K scale bytes and the lane's own
// token's V scale pair: 19 VGPRs (FP8: 32, bf16: 64), six loads.  As in the FP8 kernel each wave keeps TWO raw tiles in flight, A and B, every
// tile is the same six requests so the compiler's counted waits in front of a tile's first use leave the other tile outstanding, and the chunk
// loop is a steady part plus a tail of one to three chunks.  Nothing of a tile needs zeroing: every nibble under every scale byte a writer can
// produce (b <= 252) is finite, masked scores never reach p, and p = 0 meets raw E2M1 values.  The second K piece of the context's last chunk is
// only fetched where it holds tokens of the pool (else piece 0 again, a line the wave has just asked for).
// ------------------------------------------------------------------------------------------------
struct Tile4 { uint4 k[2]; uint2 ks; uint4 v[2]; uint32_t vs; };
constexpr int WAVE4_LDS = 64 + 32 + 32 + 32;      // floats per wave: 64 scores | 64 bf16 p (g = 0) | 64 bf16 p (g = 1) | 64 V scale pairs

template <int NW, bool FUSE>
__global__ __launch_bounds__(NW * 64, NW == 4 ? 4 : 2) void attention_fp4_kernel(AttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float part[];   // [max_chunks] m | [max_chunks] l | [max_chunks][64] o | per wave: WAVE4_LDS | FUSE, per wave: [4][64] newest k / v
    float* pm = part; float* pl = part + a.max_chunks; float* po = part + 2 * a.max_chunks;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* sbuf = part + 66 * a.max_chunks + wave * WAVE4_LDS;
    uint16_t* pbuf = reinterpret_cast<uint16_t*>(sbuf + 64);        // [2][64]
    uint16_t* vsbuf = pbuf + 128;                                   // [64]
    uint32_t* stash = reinterpret_cast<uint32_t*>(part + 66 * a.max_chunks + NW * WAVE4_LDS) + wave * (4 * 64) + lane;
    const int h = blockIdx.x, row = blockIdx.y;
    const int col = lane & 15, kg = lane >> 4;
    const uint8_t* kv = reinterpret_cast<const uint8_t*>(a.kv_layer);
    const int* rec = a.rowrec + (size_t)row * a.row_stride;
    const int L = __builtin_amdgcn_readfirstlane(rec[1]) + 1;
    const int nc = (L + CHUNK - 1) / CHUNK;
    constexpr int CPB = KV_BLOCK / CHUNK;
    // the row's block ids, one per lane, read once (as the FP8 kernel: no vector load of its own in the middle of the tile stream)
    const int nblk = (L + KV_BLOCK - 1) / KV_BLOCK;
    const int btv = lane < nblk ? rec[ROW_HDR + lane] : 0;
    auto bt = [&](int b) { return __builtin_amdgcn_readlane(btv, b); };

    auto load_tile = [&](Tile4& t, int c) __attribute__((always_inline)) {
        const int blk = bt(c / CPB), ci = c % CPB;
        const uint8_t* Kb = kv + kv4_head_base(blk, 0, h) + (size_t)ci * CHUNK4_REC;
        const uint8_t* Vb = kv + kv4_head_base(blk, 1, h) + (size_t)ci * CHUNK4_REC;
        const uint4* Kp = reinterpret_cast<const uint4*>(Kb) + k_lane_piece(lane);
        const uint4* Vp = reinterpret_cast<const uint4*>(Vb) + lane;
        const int npool = L - (FUSE ? 1 : 0) - c * CHUNK;       // tokens of this chunk that live in the pool (wave-uniform; >= 64 except in the last chunk)
        __builtin_amdgcn_sched_barrier(0);                      // the requests stay behind the last use of the registers they fill
        t.k[0] = ld_nt(Kp); t.k[1] = ld_nt(Kp + (32 < npool ? 64 : 0));
        t.ks = *reinterpret_cast<const uint2*>(Kb + CHUNK4 + 8 * col);
        t.v[0] = ld_nt(Vp); t.v[1] = ld_nt(Vp + 64);
        t.vs = *reinterpret_cast<const uint16_t*>(Vb + CHUNK4 + 2 * lane);
        __builtin_amdgcn_sched_barrier(0);
    };

    const int nmine = wave < nc ? (nc - wave + NW - 1) / NW : 0;      // chunks of this wave: wave + i NW, i < nmine
    Tile4 A, B;
    uint4 qfrag[2];                                 // B operand: q[32 ds + 8 kg .. +7], the same in all 16 columns
    if constexpr (FUSE) {
        // RoPE of this head's q and k exactly as rope_kv_fp4_kernel does it; the newest token is quantised BEFORE it joins the tile, so it
        // contributes the same K / V in the step that creates it as in every later step (write-then-read semantics)
        const uint16_t* src = a.qkv + (size_t)row * QKV + h * HD;
        const int pos = L - 1;
        const float4* cp = reinterpret_cast<const float4*>(a.cos_t + (size_t)pos * 32 + kg * 8);
        const float4* sp = reinterpret_cast<const float4*>(a.sin_t + (size_t)pos * 32 + kg * 8);
        const float4 c0 = cp[0], c1 = cp[1], s0 = sp[0], s1 = sp[1];
        const uint4 q1 = *reinterpret_cast<const uint4*>(src + kg * 8), q2 = *reinterpret_cast<const uint4*>(src + 32 + kg * 8);
        const uint4 kr1 = *reinterpret_cast<const uint4*>(src + D + kg * 8), kr2 = *reinterpret_cast<const uint4*>(src + D + 32 + kg * 8);
        const uint16_t v0 = src[2 * D + col], v1 = src[2 * D + 16 + col], v2 = src[2 * D + 32 + col], v3 = src[2 * D + 48 + col];
        asm volatile("" ::: "memory");
        load_tile(A, min(wave, nc - 1));
        const float c[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w}, s[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
        uint4 k1, k2;
        rope8(q1, q2, c, s, qfrag[0], qfrag[1]);
        rope8(kr1, kr2, c, s, k1, k2);
        // K: the lane's octets are dims 8 kg .. +7 of both blocks (every column the same): a block's amax spans the four kg groups
        float f1[8], f2[8]; unpack8(k1, f1); unpack8(k2, f2);
        uint32_t m1 = amax8(f1), m2 = amax8(f2);
        m1 = max(m1, lane_xor_u32<16>(m1, lane)); m1 = max(m1, lane_xor_u32<32>(m1, lane));
        m2 = max(m2, lane_xor_u32<16>(m2, lane)); m2 = max(m2, lane_xor_u32<32>(m2, lane));
        const uint32_t kb1 = e8m0_of(m1), kb2 = e8m0_of(m2);
        const uint32_t kw1 = q4_x8(f1, kb1), kw2 = q4_x8(f2, kb2);      // the newest key, quantised: the lane's 8-byte half (kg)
        // V: lane col holds dims col, 16 + col (block 0) and 32 + col, 48 + col (block 1) (every kg the same): amax over the 16 columns
        const float vf[4] = {bf2f(v0), bf2f(v1), bf2f(v2), bf2f(v3)};
        uint32_t n1 = max(amax_bits(vf[0]), amax_bits(vf[1])), n2 = max(amax_bits(vf[2]), amax_bits(vf[3]));
        n1 = max(n1, lane_xor_u32<8>(n1, lane)); n1 = max(n1, lane_xor_u32<4>(n1, lane)); n1 = max(n1, lane_xor_u32<2>(n1, lane)); n1 = max(n1, lane_xor_u32<1>(n1, lane));
        n2 = max(n2, lane_xor_u32<8>(n2, lane)); n2 = max(n2, lane_xor_u32<4>(n2, lane)); n2 = max(n2, lane_xor_u32<2>(n2, lane)); n2 = max(n2, lane_xor_u32<1>(n2, lane));
        const uint32_t vb1 = e8m0_of(n1), vb2 = e8m0_of(n2);
        const uint32_t vnq = q4_one(vf[0], vb1) | (q4_one(vf[1], vb1) << 4) | (q4_one(vf[2], vb2) << 8) | (q4_one(vf[3], vb2) << 12);      // nibble dt = dim 16 dt + col
        const uint32_t scs = kb1 | (kb2 << 8) | (vb1 << 16) | (vb2 << 24);
        if (wave == 0 && col == 0) {                // paged write of the newest K, early: four 8-byte halves of one 64-byte group, and its scale pair
            const int blk = bt(pos / KV_BLOCK), tok = pos % KV_BLOCK, tc = tok % CHUNK;
            uint8_t* Kw = reinterpret_cast<uint8_t*>(a.kv_layer_w) + kv4_head_base(blk, 0, h) + chunk4_base(tok);
            *reinterpret_cast<uint2*>(Kw + k4_off(tc, kg)) = make_uint2(kw1, kw2);
            if (kg == 0) *reinterpret_cast<uint16_t*>(Kw + k4s_off(tc)) = (uint16_t)(scs & 0xffffu);
        }                                           // V goes back as patched words from the wave that holds the last tile (compute)
        stash[0] = kw1; stash[64] = kw2; stash[128] = scs; stash[192] = vnq;      // parked in the wave's LDS corner until its last chunk
        asm volatile("" ::: "memory");
    } else {
        const uint16_t* qsrc = a.q + (size_t)row * D + h * HD + kg * 8;
        qfrag[0] = *reinterpret_cast<const uint4*>(qsrc); qfrag[1] = *reinterpret_cast<const uint4*>(qsrc + 32);
        asm volatile("" ::: "memory");
        load_tile(A, min(wave, nc - 1));
    }

    // LAST: the tile may be the context's last chunk (only a wave's final chunk can be)
    auto compute = [&](Tile4& t, int c, auto last_tag) __attribute__((always_inline)) {
        constexpr bool LAST = decltype(last_tag)::value;
        if (FUSE && LAST && c == nc - 1) {          // the newest token is patched into the last tile
            const uint32_t kw1 = stash[0], kw2 = stash[64], scs = stash[128], vnq = stash[192];
            const int tc = L - 1 - c * CHUNK;
            const int tts = tc >> 4, ts = tc & 15, half = tc >> 5, kgs = (tc & 31) >> 3, nib = 4 * (tc & 7);
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {        // selects over compile-time registers: nothing is indexed at run time
                const bool hit = (tt == tts) && (col == ts);
                uint4& p = t.k[tt >> 1];
                uint32_t& wa = (tt & 1) ? p.z : p.x; uint32_t& wb = (tt & 1) ? p.w : p.y;
                wa = hit ? kw1 : wa; wb = hit ? kw2 : wb;
                uint32_t& s2 = (tt >> 1) ? t.ks.y : t.ks.x;
                const uint32_t ns = (tt & 1) ? ((s2 & 0x0000ffffu) | (scs << 16)) : ((s2 & 0xffff0000u) | (scs & 0xffffu));
                s2 = hit ? ns : s2;
            }
            const int blk = bt(c / CPB), ci = c % CPB;
            uint8_t* Vw = reinterpret_cast<uint8_t*>(a.kv_layer_w) + kv4_head_base(blk, 1, h) + (size_t)ci * CHUNK4_REC;
            if (lane == tc) { t.vs = scs >> 16; *reinterpret_cast<uint16_t*>(Vw + v4s_off(tc)) = (uint16_t)(scs >> 16); }
            if (kg == kgs) {
                // Paged write of the newest V: one token is 64 nibbles in 64 words.  The patched words (8 consecutive tokens of one dim) ARE the
                // pool's content with the new token merged in: the 16 lanes of the token's group write theirs back, one word per dim tile.
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    uint4& p = t.v[dt >> 1];
                    uint32_t& wa = (dt & 1) ? p.z : p.x; uint32_t& wb = (dt & 1) ? p.w : p.y;      // ts = 0, 1
                    const uint32_t w = ((half ? wb : wa) & ~(0xfu << nib)) | (((vnq >> (4 * dt)) & 0xfu) << nib);
                    wa = half ? wa : w; wb = half ? w : wb;
                    *reinterpret_cast<uint32_t*>(Vw + (dt >> 1) * 1024 + lane * 16 + ((dt & 1) * 2 + half) * 4) = w;
                }
            }
        }
        // ---- scores on the matrix cores: D[token][col] = K[token][:] . q
        f32x4 sacc[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) sacc[tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        sacc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(k4_frag<0, 0>(t.k, t.ks)), as_frag(qfrag[0]), sacc[0], 0, 0, 0);
        sacc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(k4_frag<0, 1>(t.k, t.ks)), as_frag(qfrag[1]), sacc[0], 0, 0, 0);
        sacc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(k4_frag<1, 0>(t.k, t.ks)), as_frag(qfrag[0]), sacc[1], 0, 0, 0);
        sacc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(k4_frag<1, 1>(t.k, t.ks)), as_frag(qfrag[1]), sacc[1], 0, 0, 0);
        sacc[2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(k4_frag<2, 0>(t.k, t.ks)), as_frag(qfrag[0]), sacc[2], 0, 0, 0);
        sacc[2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(k4_frag<2, 1>(t.k, t.ks)), as_frag(qfrag[1]), sacc[2], 0, 0, 0);
        sacc[3] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(k4_frag<3, 0>(t.k, t.ks)), as_frag(qfrag[0]), sacc[3], 0, 0, 0);
        sacc[3] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(k4_frag<3, 1>(t.k, t.ks)), as_frag(qfrag[1]), sacc[3], 0, 0, 0);
        if (col == 0) {                             // lanes 0,16,32,48 hold every score once: rows 4 kg + r of each token tile
#pragma unroll
            for (int tt = 0; tt < 4; ++tt)
                *reinterpret_cast<float4*>(sbuf + 16 * tt + 4 * kg) = make_float4(sacc[tt][0], sacc[tt][1], sacc[tt][2], sacc[tt][3]);
        }
        asm volatile("" ::: "memory");              // wave-private LDS exchange (a wave's DS operations execute in order)
        // ---- softmax statistics, lane = token
        const bool live = (c * CHUNK + lane) < L;
        const float sc = live ? sbuf[lane] * 0.125f : -INFINITY;
        const float m = wave_max_f32(sc, lane);
        const float p = live ? t3_expf(sc - m) : 0.0f;
        const float lsum = wave_bfly_add_f32(p, lane);
        const uint32_t pb = (p < 0x1p-100f) ? 0u : f2bf(p);
        const uint32_t b0 = t.vs & 0xffu, b1 = (t.vs >> 8) & 0xffu;
        const bool slow = __any(fold_unsafe(pb, b0, b1));      // wave-uniform
        pbuf[lane] = (uint16_t)(slow ? pb : fold_p(pb, b0));
        pbuf[64 + lane] = (uint16_t)fold_p(pb, b1);
        vsbuf[lane] = (uint16_t)t.vs;
        asm volatile("" ::: "memory");
        // ---- P.V on the matrix cores: D[dim][col] = sum_token V[token][dim] * p[token]
        f32x4 oacc[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) oacc[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (!slow) {
            uint4 pfrag[2][2];                      // B operand [g][ts]: p_g[32 ts + 8 kg .. +7] as bf16, the same in all 16 columns
#pragma unroll
            for (int g = 0; g < 2; ++g) { pfrag[g][0] = *reinterpret_cast<const uint4*>(pbuf + 64 * g + 8 * kg); pfrag[g][1] = *reinterpret_cast<const uint4*>(pbuf + 64 * g + 32 + 8 * kg); }
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                oacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(dq4_frag(v4_word(t.v, dt, 0), 1.0f)), as_frag(pfrag[dt >> 1][0]), oacc[dt], 0, 0, 0);
                oacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(dq4_frag(v4_word(t.v, dt, 1), 1.0f)), as_frag(pfrag[dt >> 1][1]), oacc[dt], 0, 0, 0);
            }
        } else {
            const uint4 p0 = *reinterpret_cast<const uint4*>(pbuf + 8 * kg), p1 = *reinterpret_cast<const uint4*>(pbuf + 32 + 8 * kg);
            const uint4 s0 = *reinterpret_cast<const uint4*>(vsbuf + 8 * kg), s1 = *reinterpret_cast<const uint4*>(vsbuf + 32 + 8 * kg);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const uint4 f0 = dt < 2 ? dq4_frag_tokens<0>(v4_word(t.v, dt, 0), s0) : dq4_frag_tokens<1>(v4_word(t.v, dt, 0), s0);
                const uint4 f1 = dt < 2 ? dq4_frag_tokens<0>(v4_word(t.v, dt, 1), s1) : dq4_frag_tokens<1>(v4_word(t.v, dt, 1), s1);
                oacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(f0), as_frag(p0), oacc[dt], 0, 0, 0);
                oacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(f1), as_frag(p1), oacc[dt], 0, 0, 0);
            }
        }
        if (col == 0) {
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                *reinterpret_cast<float4*>(po + c * 64 + 16 * dt + 4 * kg) = make_float4(oacc[dt][0], oacc[dt][1], oacc[dt][2], oacc[dt][3]);
        }
        if (lane == 0) { pm[c] = m; pl[c] = lsum; }
        asm volatile("" ::: "memory");              // the next chunk reuses the wave's LDS corner
    };

    constexpr std::false_type INNER{}; constexpr std::true_type FINAL{};
    int i = 0;
    auto chunk = [&](int k) { return wave + k * NW; };
    load_tile(B, nmine > 1 ? chunk(1) : min(wave, nc - 1));
    for (; i + 3 < nmine; i += 2) {                 // steady part: A holds chunk i, B chunk i + 1 (in flight), chunks i + 2 and i + 3 exist
        compute(A, chunk(i), INNER);     load_tile(A, chunk(i + 2));
        compute(B, chunk(i + 1), INNER); load_tile(B, chunk(i + 3));
    }
    if (nmine - i == 3) {                           // tail: one to three chunks left, A holds the first of them
        compute(A, chunk(i), INNER); load_tile(A, chunk(i + 2));
        compute(B, chunk(i + 1), INNER);
        i += 2;
    } else if (nmine - i == 2) {
        compute(A, chunk(i), INNER);
        compute(B, chunk(i + 1), FINAL);
    }
    if (nmine - i == 1) compute(A, chunk(i), FINAL);
    __syncthreads();
    if (wave == 0) {
        // fold in ascending chunk order (contract), as attention_kernel: M and the weights w_c = exp(m_c - M) side by side, then two fmas per chunk
        float M = -INFINITY;
        for (int c0 = 0; c0 < nc; c0 += 64) M = fmaxf(M, (c0 + lane < nc) ? pm[c0 + lane] : -INFINITY);
        M = wave_max_f32(M, lane);
        for (int c0 = 0; c0 < nc; c0 += 64) if (c0 + lane < nc) pm[c0 + lane] = t3_expf(pm[c0 + lane] - M);
        asm volatile("" ::: "memory");
        float l = 0.0f, o = 0.0f;
        int c = 0;
        for (; c + 4 <= nc; c += 4) {
            float wc[4], lc[4], oc[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { wc[u] = pm[c + u]; lc[u] = pl[c + u]; oc[u] = po[(c + u) * 64 + lane]; }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                l = __builtin_fmaf(wc[u], lc[u], l);
                o = __builtin_fmaf(wc[u], oc[u], o);
            }
        }
        for (; c < nc; ++c) {
            const float w = pm[c];
            l = __builtin_fmaf(w, pl[c], l);
            o = __builtin_fmaf(w, po[c * 64 + lane], o);
        }
        a.out[(size_t)row * D + h * HD + lane] = (uint16_t)f2bf(o / l);
    }
}

// ------------------------------------------------------------------------------------------------
// Prefill form over the MXFP4 pool: one workgroup per (head, 16 consecutive rows of the launch), the segment logic, register layout and
// fold of attention_tile_kernel.  A lane holds p of tokens 16 tt + 4 kg + r of row col, so the V scale pairs it folds in are the 8 bytes at
// token 16 tt + 4 kg, one small load per token tile; the wave's probability image exists once per dim group.
// ------------------------------------------------------------------------------------------------
constexpr int TILE4_OS = 68;            // floats per (chunk, row) line of partial outputs (64 + padding against LDS bank conflicts)
constexpr int TILE4_PS = 72;            // bf16 per row of a wave's probability image
__global__ __launch_bounds__(256, 2) void attention_tile_fp4_kernel(AttnArgs a, int row_base, int chunks_cap) {
    extern __shared__ __attribute__((aligned(16))) float part[];   // [cap][16][TILE4_OS] o | [cap][16] m | [cap][16] l | per wave: [2][16][TILE4_PS] bf16 p
    float* po = part; float* pm = part + (size_t)chunks_cap * 16 * TILE4_OS; float* pl = pm + chunks_cap * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint16_t* pimg = reinterpret_cast<uint16_t*>(pl + chunks_cap * 16) + wave * (2 * 16 * TILE4_PS);
    const int col = lane & 15, kg = lane >> 4;
    const int h = blockIdx.x, r0 = row_base + blockIdx.y * 16;
    const int nrows = min(16, a.rows - r0);
    const int myrow = r0 + min(col, nrows - 1);
    const uint8_t* kv = reinterpret_cast<const uint8_t*>(a.kv_layer);
    const int* myrec = a.rowrec + (size_t)myrow * a.row_stride;
    const int my_stream = myrec[0], my_L = myrec[1] + 1;
    uint4 qfrag[2];                                 // B operand: column col = row r0 + col
    {
        const uint16_t* qsrc = a.q + (size_t)myrow * D + h * HD + kg * 8;
        qfrag[0] = *reinterpret_cast<const uint4*>(qsrc); qfrag[1] = *reinterpret_cast<const uint4*>(qsrc + 32);
    }
    constexpr int CPB = KV_BLOCK / CHUNK;
    const unsigned valid = nrows >= 16 ? 0xffffu : ((1u << nrows) - 1u);
    unsigned done = 0;
    while ((done & valid) != valid) {               // one pass per stream present in the tile (wave-uniform control flow)
        const int lead = __builtin_ctz(~done & valid);
        const int lead_stream = __builtin_amdgcn_readlane(my_stream, lead);
        const bool in_seg = col < nrows && my_stream == lead_stream;
        const unsigned seg = (unsigned)(__ballot(in_seg) & 0xffffull);
        int Lmax = in_seg ? my_L : 0;
#pragma unroll
        for (int off = 8; off >= 1; off >>= 1) Lmax = max(Lmax, __shfl_xor(Lmax, off));
        Lmax = __builtin_amdgcn_readfirstlane(Lmax);
        const int nc = min((Lmax + CHUNK - 1) / CHUNK, chunks_cap);
        const int* bt = a.rowrec + (size_t)(r0 + lead) * a.row_stride + ROW_HDR;
        for (int c = wave; c < nc; c += 4) {
            uint4 tk[2], tv[2]; uint2 tks, tvs[4];
            const int blk = bt[c / CPB], ci = c % CPB;
            const uint8_t* Kb = kv + kv4_head_base(blk, 0, h) + (size_t)ci * CHUNK4_REC;
            const uint8_t* Vb = kv + kv4_head_base(blk, 1, h) + (size_t)ci * CHUNK4_REC;
            {
                const uint4* Kp = reinterpret_cast<const uint4*>(Kb) + k_lane_piece(lane);
                const uint4* Vp = reinterpret_cast<const uint4*>(Vb) + lane;
                tk[0] = Kp[0]; tk[1] = Kp[64]; tks = *reinterpret_cast<const uint2*>(Kb + CHUNK4 + 8 * col);
                tv[0] = Vp[0]; tv[1] = Vp[64];
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) tvs[tt] = *reinterpret_cast<const uint2*>(Vb + CHUNK4 + 2 * (16 * tt + 4 * kg));
            }
            f32x4 sacc[4];                          // sacc[tt][r] = score of token 16 tt + 4 kg + r of the chunk for row col
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) sacc[tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
            sacc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(k4_frag<0, 0>(tk, tks)), as_frag(qfrag[0]), sacc[0], 0, 0, 0);
            sacc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(k4_frag<0, 1>(tk, tks)), as_frag(qfrag[1]), sacc[0], 0, 0, 0);
            sacc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(k4_frag<1, 0>(tk, tks)), as_frag(qfrag[0]), sacc[1], 0, 0, 0);
            sacc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(k4_frag<1, 1>(tk, tks)), as_frag(qfrag[1]), sacc[1], 0, 0, 0);
            sacc[2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(k4_frag<2, 0>(tk, tks)), as_frag(qfrag[0]), sacc[2], 0, 0, 0);
            sacc[2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(k4_frag<2, 1>(tk, tks)), as_frag(qfrag[1]), sacc[2], 0, 0, 0);
            sacc[3] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(k4_frag<3, 0>(tk, tks)), as_frag(qfrag[0]), sacc[3], 0, 0, 0);
            sacc[3] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(k4_frag<3, 1>(tk, tks)), as_frag(qfrag[1]), sacc[3], 0, 0, 0);
            const int nlive = my_L - c * CHUNK;     // tokens of this chunk the row sees (causal), may be <= 0 or >= 64
            float sc[4][4], m = -INFINITY;
#pragma unroll
            for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    sc[tt][r] = (16 * tt + 4 * kg + r) < nlive ? sacc[tt][r] * 0.125f : -INFINITY;
                    m = fmaxf(m, sc[tt][r]);
                }
            m = fmaxf(m, lane_xor<16>(m, lane)); m = fmaxf(m, lane_xor<32>(m, lane));
            float pr[4][4];
#pragma unroll
            for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                for (int r = 0; r < 4; ++r) pr[tt][r] = (16 * tt + 4 * kg + r) < nlive ? t3_expf(sc[tt][r] - m) : 0.0f;
            // the contract's butterfly sum over the 64 tokens (partners t ^ 32, 16, 8, 4, 2, 1): bits 5, 4 of the token are tt,
            // bits 3, 2 are kg (lane bits 5, 4), bits 1, 0 are r
            float b4[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) b4[r] = (pr[0][r] + pr[2][r]) + (pr[1][r] + pr[3][r]);
#pragma unroll
            for (int r = 0; r < 4; ++r) b4[r] = b4[r] + lane_xor<32>(b4[r], lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) b4[r] = b4[r] + lane_xor<16>(b4[r], lane);
            const float lsum = (b4[0] + b4[2]) + (b4[1] + b4[3]);
            uint32_t pk[4][4];
            bool unsafe = false;
#pragma unroll
            for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    pk[tt][r] = (pr[tt][r] < 0x1p-100f) ? 0u : f2bf(pr[tt][r]);
                    const uint32_t s2 = ((r >> 1) ? tvs[tt].y : tvs[tt].x) >> (16 * (r & 1));
                    unsafe = unsafe || fold_unsafe(pk[tt][r], s2 & 0xffu, (s2 >> 8) & 0xffu);
                }
            const bool slow = __any(unsafe);        // wave-uniform
#pragma unroll
            for (int g = 0; g < 2; ++g)
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                    uint32_t q[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const uint32_t s2 = ((r >> 1) ? tvs[tt].y : tvs[tt].x) >> (16 * (r & 1) + 8 * g);
                        q[r] = (slow && g == 0) ? pk[tt][r] : fold_p(pk[tt][r], s2 & 0xffu);
                    }
                    *reinterpret_cast<uint2*>(pimg + (g * 16 + col) * TILE4_PS + 16 * tt + 4 * kg) = make_uint2(q[0] | (q[1] << 16), q[2] | (q[3] << 16));
                }
            asm volatile("" ::: "memory");          // wave-private LDS exchange (a wave's DS operations execute in order)
            uint4 pfrag[2][2];
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                pfrag[g][0] = *reinterpret_cast<const uint4*>(pimg + (g * 16 + col) * TILE4_PS + 8 * kg);
                pfrag[g][1] = *reinterpret_cast<const uint4*>(pimg + (g * 16 + col) * TILE4_PS + 32 + 8 * kg);
            }
            asm volatile("" ::: "memory");
            if (kg == 0) { pm[c * 16 + col] = m; pl[c * 16 + col] = lsum; }
            uint4 s0 = make_uint4(0, 0, 0, 0), s1 = s0;
            if (slow) { s0 = *reinterpret_cast<const uint4*>(Vb + CHUNK4 + 16 * kg); s1 = *reinterpret_cast<const uint4*>(Vb + CHUNK4 + 64 + 16 * kg); }
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                uint4 f0, f1;
                if (!slow) { f0 = dq4_frag(v4_word(tv, dt, 0), 1.0f); f1 = dq4_frag(v4_word(tv, dt, 1), 1.0f); }
                else if (dt < 2) { f0 = dq4_frag_tokens<0>(v4_word(tv, dt, 0), s0); f1 = dq4_frag_tokens<0>(v4_word(tv, dt, 1), s1); }
                else { f0 = dq4_frag_tokens<1>(v4_word(tv, dt, 0), s0); f1 = dq4_frag_tokens<1>(v4_word(tv, dt, 1), s1); }
                const bool g1 = !slow && dt >= 2;   // the element-wise path meets the plain p, which sits in image 0
                const uint4 pa = g1 ? pfrag[1][0] : pfrag[0][0], pb = g1 ? pfrag[1][1] : pfrag[0][1];
                f32x4 oacc = (f32x4){0.f, 0.f, 0.f, 0.f};
                oacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(f0), as_frag(pa), oacc, 0, 0, 0);
                oacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(f1), as_frag(pb), oacc, 0, 0, 0);
                *reinterpret_cast<float4*>(po + (size_t)(c * 16 + col) * TILE4_OS + 16 * dt + 4 * kg) = make_float4(oacc[0], oacc[1], oacc[2], oacc[3]);
            }
        }
        __syncthreads();
        {   // fold: thread = (row, 4 dims), ascending chunk order over the row's own chunks
            const int row = tid >> 4, d4 = (tid & 15) * 4;
            if ((seg >> row) & 1u) {
                const int L = a.rowrec[(size_t)(r0 + row) * a.row_stride + 1] + 1;
                const int ncr = min((L + CHUNK - 1) / CHUNK, chunks_cap);
                float M = -INFINITY;
                for (int c = 0; c < ncr; ++c) M = fmaxf(M, pm[c * 16 + row]);
                float l = 0.0f, o[4] = {0.f, 0.f, 0.f, 0.f};
                for (int c = 0; c < ncr; ++c) {
                    const float w = t3_expf(pm[c * 16 + row] - M);
                    const float4 oc = *reinterpret_cast<const float4*>(po + (size_t)(c * 16 + row) * TILE4_OS + d4);
                    l = __builtin_fmaf(w, pl[c * 16 + row], l);
                    o[0] = __builtin_fmaf(w, oc.x, o[0]); o[1] = __builtin_fmaf(w, oc.y, o[1]);
                    o[2] = __builtin_fmaf(w, oc.z, o[2]); o[3] = __builtin_fmaf(w, oc.w, o[3]);
                }
                const uint32_t lo = (uint32_t)f2bf(o[0] / l) | ((uint32_t)f2bf(o[1] / l) << 16), hi = (uint32_t)f2bf(o[2] / l) | ((uint32_t)f2bf(o[3] / l) << 16);
                *reinterpret_cast<uint2*>(a.out + (size_t)(r0 + row) * D + h * HD + d4) = make_uint2(lo, hi);
            }
        }
        done |= seg;
        if ((done & valid) != valid) __syncthreads();      // the next segment reuses the partial slots
    }
}

// Same dispatch as launch_attention_fp8: prefill rows [tile_from, rows) of an unfused launch take the tile kernel while its partials fit the
// CU's LDS, everything else the per-row kernel with 8 waves up to 8 rows and 4 beyond.
hipError_t launch_attention_fp4(const AttnArgs& a, hipStream_t s) {
    if (a.rows <= 0) return hipSuccess;
    const int cap = a.tile_chunks > 0 ? min(a.tile_chunks, a.max_chunks) : a.max_chunks;
    const size_t lds_t = ((size_t)cap * 16 * (TILE4_OS + 2)) * sizeof(float) + (size_t)4 * 2 * 16 * TILE4_PS * 2;
    constexpr size_t LDS_PER_CU = 160 * 1024;
    if (!a.qkv && a.tile_from >= 0 && a.tile_from < a.rows && lds_t <= LDS_PER_CU) {
        static size_t raised[MAX_DEVICES] = {};
        size_t& have = raised[cur_device()];
        if (have < 64 * 1024) have = 64 * 1024;
        if (lds_t > have) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(attention_tile_fp4_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_t);
            if (e != hipSuccess) return e;
            have = lds_t;
        }
        hipLaunchKernelGGL(attention_tile_fp4_kernel, dim3(H, (a.rows - a.tile_from + 15) / 16), dim3(256), lds_t, s, a, a.tile_from, cap);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess || a.tile_from == 0) return e;
        AttnArgs head = a; head.rows = a.tile_from; head.tile_from = -1;
        return launch_attention_fp4(head, s);
    }
    if ((size_t)a.max_chunks * CHUNK > (size_t)64 * KV_BLOCK) return hipErrorInvalidValue;      // the per-row kernel keeps a row's block ids one per lane
    const int nw = a.force_waves == 4 || a.force_waves == 8 ? a.force_waves : (a.rows <= 8 ? 8 : 4);
    const dim3 grid(H, a.rows);
    const size_t lds = ((size_t)a.max_chunks * 66 + (size_t)nw * (WAVE4_LDS + (a.qkv ? 4 * 64 : 0))) * sizeof(float);
    if (nw == 8) { if (a.qkv) launch_k((attention_fp4_kernel<8, true>), grid, dim3(512), lds, s, a); else launch_k((attention_fp4_kernel<8, false>), grid, dim3(512), lds, s, a); }
    else { if (a.qkv) launch_k((attention_fp4_kernel<4, true>), grid, dim3(256), lds, s, a); else launch_k((attention_fp4_kernel<4, false>), grid, dim3(256), lds, s, a); }
    return hipGetLastError();
}

}  // namespace t3
