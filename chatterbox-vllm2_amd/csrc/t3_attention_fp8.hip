// The FP8 (OCP E4M3FN) form of the paged KV pool for gfx950 (MI355X, CDNA4): RoPE + quantise + paged write, the fused decode attention,
// the 16-rows-per-workgroup prefill attention and the read-back hook.  Opt-in (T3EngineConfig.kv_cache_dtype = 1); the bf16 pool and its
// kernels (t3_attention.hip) are untouched.
//
// Numerics contract (DESIGN.md "Attention", FP8 pool): the pool holds q8(x) = e4m3fn(rne(clamp(x, -448, 448))) of the bf16 value the
// bf16 pool would hold (K after RoPE and its bf16 rounding, V as it arrives), scale 1.0.  Every e4m3 value is a bf16 value: the kernels
// dequantise to bf16 in registers right in front of each MFMA and run the bf16 chain on it (v_mfma_f32_16x16x32_bf16, 64-token chunks,
// softmax, butterfly order, bf16 p, ascending chunk fold), so the output is bit for bit the bf16 contract's result over the dequantised
// K / V.  The fp8 MFMA is not used: it would force q and p into fp8.  Compile with -ffp-contract=off.
#include "t3_kernels.h"
#include "t3_device.h"
#include "t3_attention_common.h"

#include <math.h>
#include <type_traits>

namespace t3 {
// ------------------------------------------------------------------------------------------------
// q8 / dequantise.  The clamp runs in VALU in front of the convert, so saturation does not depend on a mode-register bit; NaN stays NaN.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float clamp8(float x) { const float c = fminf(fmaxf(x, -448.0f), 448.0f); return x != x ? x : c; }
__device__ __forceinline__ uint32_t q8_x4(float a, float b, float c, float d) {      // four fp32 -> four e4m3 bytes, a in the lowest
    const int w = __builtin_amdgcn_cvt_pk_fp8_f32(clamp8(a), clamp8(b), 0, false);
    return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(clamp8(c), clamp8(d), w, true);
}
__device__ __forceinline__ uint2 q8_bf8(const uint4& v) {                            // eight bf16 -> eight e4m3 bytes
    float f[8]; unpack8(v, f);
    return make_uint2(q8_x4(f[0], f[1], f[2], f[3]), q8_x4(f[4], f[5], f[6], f[7]));
}
__device__ __forceinline__ uint32_t q8_one(uint32_t bf) { return q8_x4(bf2f((uint16_t)bf), 0.0f, 0.0f, 0.0f) & 0xffu; }
// (dq8_pair() / dq8_frag(), the dequantisation in front of every MFMA: t3_attention_common.h, shared with t3_alignment.hip)
__device__ __forceinline__ uint32_t dq8_one(uint32_t byte) { return dq8_pair<false>(byte) & 0xffffu; }

__global__ __launch_bounds__(256) void fp8_roundtrip_kernel(const float* x, float* y, int n) {      // parity hook: y = dequantised q8(x), four values per lane
    const int i = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    float f[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) f[e] = i + e < n ? x[i + e] : 0.0f;
    const uint32_t w = q8_x4(f[0], f[1], f[2], f[3]);
    const uint32_t lo = dq8_pair<false>(w), hi = dq8_pair<true>(w);
    const float g[4] = {bf_lo(lo), bf_hi(lo), bf_lo(hi), bf_hi(hi)};
#pragma unroll
    for (int e = 0; e < 4; ++e) if (i + e < n) y[i + e] = g[e];
}
hipError_t launch_fp8_roundtrip(const float* x, float* y, int n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(fp8_roundtrip_kernel, dim3((n + 1023) / 1024), dim3(256), 0, s, x, y, n);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Paged layout of one (block, head), one byte per element: [chunk-in-block][4 pieces][64 lanes][16 B] for K and for V: a chunk is 4 + 4
// fully coalesced 1 KiB wave loads (the bf16 pool: 8 + 8).  One 16-byte piece carries BOTH halves the bf16 layout splits in two:
//   K piece tt, lane (t, kg):  bytes 0-7 = K[token 16 tt + t][dims 8 kg .. +7], bytes 8-15 = dims 32 + 8 kg .. +7: the lane's RoPE pairs and its
//     two MFMA A fragments (ds = 0, 1).  In memory the piece sits at index 4 t + kg (token-major, as the bf16 pool): a token's K is ONE 64-byte line.
//   V piece dt, lane (d, kg):  bytes 0-7 = V[tokens 8 kg .. +7][dim 16 dt + d], bytes 8-15 = tokens 32 + 8 kg .. +7 (A fragments ts = 0, 1), at index d + 16 kg.
// The head regions keep KV_HEAD_PAD = 512 elements (here 512 bytes) between them: 16.5 KiB per head instead of a power of two, and a block of
// exactly half the bf16 block's bytes.  The value is carried over from the bf16 pool, not measured for one-byte elements.
// ------------------------------------------------------------------------------------------------
// (CHUNK8, kv8_head_base() and k8_lane_piece(): t3_attention_common.h)
__device__ __forceinline__ size_t k8_off(int tok_in_block, int kg) { return (size_t)tok_in_block * HD + kg * 16; }      // 16 tt-major tokens x 64 B = the piece order above
__device__ __forceinline__ size_t v8_off(int tok_in_block, int dim) {                                                     // one byte
    const int ci = tok_in_block / CHUNK, tc = tok_in_block % CHUNK;
    return (size_t)ci * CHUNK8 + (size_t)(dim >> 4) * 1024 + (size_t)((dim & 15) + 16 * ((tc & 31) >> 3)) * 16 + (tc >> 5) * 8 + (tc & 7);
}

// RoPE + quantise + paged write: one wave per row, lane = 4 * head + part as rope_kv_kernel.  The lane's two rotated K octets ARE its 16-byte piece.
__global__ __launch_bounds__(256) void rope_kv_fp8_kernel(RopeArgs a) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.rows) return;
    uint8_t* kv = reinterpret_cast<uint8_t*>(a.kv_layer);
    const int* rec = a.rowrec + (size_t)row * a.row_stride;
    const int pos = rec[1];
    const int blk = rec[ROW_HDR + pos / KV_BLOCK], tok = pos % KV_BLOCK;
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
        const uint2 lo = q8_bf8(o1), hi = q8_bf8(o2);
        *reinterpret_cast<uint4*>(kv + kv8_head_base(blk, 0, h) + k8_off(tok, part)) = make_uint4(lo.x, lo.y, hi.x, hi.y);
    }
    // V, token-minor: where the launch holds all 8 rows of an aligned token group, the wave of the group's first row transposes the
    // 8 x 1024 block in registers and writes 8-byte half pieces (8 consecutive tokens of one dim); the other seven waves skip V.
    // Anything else (ragged ends of a run) writes single bytes.
    const int p8 = pos & 7, jl = row - p8;
    bool full = false;
    if (jl >= 0 && jl + 7 < a.rows) {
        int ok = 1;
        if (lane < 8) { const int* r2 = a.rowrec + (size_t)(jl + lane) * a.row_stride; ok = (r2[0] == rec[0]) && (r2[1] == pos - p8 + lane); }
        full = __all(ok);
    }
    if (full) {
        if (p8 != 0) return;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int pc = lane + 64 * u, hh = pc >> 3, oct = pc & 7;          // (head, 8 dims 8 oct .. 8 oct + 7)
            uint4 x[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) x[i] = *reinterpret_cast<const uint4*>(a.qkv + (size_t)(row + i) * QKV + 2 * D + hh * 64 + oct * 8);
            uint8_t* dst = kv + kv8_head_base(blk, 1, hh) + v8_off(tok, oct * 8);      // dim 8 oct + d: 16 d bytes further
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                auto el = [&](const uint4& v) { const uint32_t w = (d >> 1) == 0 ? v.x : (d >> 1) == 1 ? v.y : (d >> 1) == 2 ? v.z : v.w; return (d & 1) ? bf_hi(w) : bf_lo(w); };
                *reinterpret_cast<uint2*>(dst + 16 * d) = make_uint2(q8_x4(el(x[0]), el(x[1]), el(x[2]), el(x[3])), q8_x4(el(x[4]), el(x[5]), el(x[6]), el(x[7])));
            }
        }
        return;
    }
    uint8_t* vb = kv + kv8_head_base(blk, 1, h);
    const uint16_t* vs = qr + 2 * D + h * 64 + part * 16;
#pragma unroll
    for (int e = 0; e < 16; ++e) vb[v8_off(tok, part * 16 + e)] = (uint8_t)q8_one(vs[e]);
}
hipError_t launch_rope_kv_fp8(const RopeArgs& a, hipStream_t s) {
    if (a.rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(rope_kv_fp8_kernel, dim3((a.rows + 3) / 4), dim3(256), 0, s, a);
    return hipGetLastError();
}
// parity hook: the stored K / V of a row's (stream, position), dequantised to bf16 -> out [rows][2][1024]; one wave per row, lane = (head, part)
__global__ __launch_bounds__(256) void kv_gather_fp8_kernel(const uint8_t* kv, const int* rowrec, int row_stride, int rows, uint16_t* out) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int* rec = rowrec + (size_t)row * row_stride;
    const int pos = rec[1], blk = rec[ROW_HDR + pos / KV_BLOCK], tok = pos % KV_BLOCK;
    const int h = lane >> 2, part = lane & 3;
    const uint8_t* vb = kv + kv8_head_base(blk, 1, h);
    uint16_t* ko = out + (size_t)row * 2 * D + h * HD;
    uint16_t* vo = ko + D;
    const uint4 p = *reinterpret_cast<const uint4*>(kv + kv8_head_base(blk, 0, h) + k8_off(tok, part));
    *reinterpret_cast<uint4*>(ko + part * 8) = dq8_frag(p.x, p.y);
    *reinterpret_cast<uint4*>(ko + 32 + part * 8) = dq8_frag(p.z, p.w);
#pragma unroll
    for (int e = 0; e < 16; ++e) vo[part * 16 + e] = (uint16_t)dq8_one(vb[v8_off(tok, part * 16 + e)]);
}
hipError_t launch_kv_gather_fp8(const uint16_t* kv_layer, const int* rowrec, int row_stride, int rows, uint16_t* out, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(kv_gather_fp8_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, reinterpret_cast<const uint8_t*>(kv_layer), rowrec, row_stride, rows, out);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Paged attention for one (row, head) over the FP8 pool.  Work split, LDS partials and the fold are attention_kernel's (one workgroup of NW
// waves, wave w takes chunks w, w + NW, ...).  What differs is how the bytes move: a raw chunk tile is 4 K + 4 V pieces = 32 VGPRs, half the
// bf16 tile, so with the same occupancy one tile per wave would keep half as many bytes in flight.  Each wave therefore keeps TWO raw tiles in
// flight, A and B (the 64 registers the bf16 kernel spends on one tile): chunk c + NW is requested before chunk c is computed, chunk c + 2 NW
// goes out the moment A's registers are free.  Loads retire in issue order, so the wait in front of a tile's first use is a counted
// vmcnt(8) that leaves the other tile's eight requests outstanding.  The count is the compiler's own bookkeeping (plain loads, no hand-counted
// asm), which is exact only where every path issues the same requests: so EVERY tile is exactly eight loads (pieces of the last chunk that
// hold no pool token are pointed at piece 0 again -- a line the wave has just asked for -- and zeroed when the tile is used), and the chunk
// loop is a steady part whose two requests per round are unconditional plus a tail of one to three chunks.  A piece is dequantised to its
// two bf16 A fragments right in front of the two MFMAs that read them: 8 v_cvt_scalef32_pk_bf16_fp8 per piece, 64 per chunk.
// ------------------------------------------------------------------------------------------------
struct Tile8 { uint4 k[4], v[4]; };
__device__ __forceinline__ void patch8(uint4& v, int j, uint32_t val) {      // replace byte j (0..15) of v
    const uint32_t sh = (j & 3) * 8, keep = ~(0xffu << sh), ins = val << sh;
    const int w = j >> 2;
    v.x = w == 0 ? ((v.x & keep) | ins) : v.x; v.y = w == 1 ? ((v.y & keep) | ins) : v.y;
    v.z = w == 2 ? ((v.z & keep) | ins) : v.z; v.w = w == 3 ? ((v.w & keep) | ins) : v.w;
}

template <int NW, bool FUSE>
__global__ __launch_bounds__(NW * 64, NW == 4 ? 4 : 2) void attention_fp8_kernel(AttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float part[];   // [max_chunks] m | [max_chunks] l | [max_chunks][64] o | per wave: 64 scores, 64 bf16 p | FUSE, per wave: [5][64] newest k / v
    float* pm = part; float* pl = part + a.max_chunks; float* po = part + 2 * a.max_chunks;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* sbuf = part + 66 * a.max_chunks + wave * 96;
    uint16_t* pbuf = reinterpret_cast<uint16_t*>(sbuf + 64);
    uint32_t* stash = reinterpret_cast<uint32_t*>(part + 66 * a.max_chunks + NW * 96) + wave * (5 * 64) + lane;      // FUSE: the newest key / value park here
    const int h = blockIdx.x, row = blockIdx.y;
    const int col = lane & 15, kg = lane >> 4;
    const uint8_t* kv = reinterpret_cast<const uint8_t*>(a.kv_layer);
    const int* rec = a.rowrec + (size_t)row * a.row_stride;
    const int L = __builtin_amdgcn_readfirstlane(rec[1]) + 1;
    const int nc = (L + CHUNK - 1) / CHUNK;
    constexpr int CPB = KV_BLOCK / CHUNK;
    // The row's block ids, one per lane (max_model_len 8192 = 32 blocks), read ONCE: a block id fetched per chunk would be a vector load of
    // its own in the middle of the tile stream, and the wait for it (loads retire in order) would drain both tiles in flight.
    const int nblk = (L + KV_BLOCK - 1) / KV_BLOCK;
    const int btv = lane < nblk ? rec[ROW_HDR + lane] : 0;
    auto bt = [&](int b) { return __builtin_amdgcn_readlane(btv, b); };

    // Always eight requests (see above).  Of the context's LAST chunk only the K pieces that hold tokens of the pool cost bytes (the fused
    // form's newest token comes from registers); a V piece spans the whole chunk, so all four are needed as soon as one token is in the pool.
    auto load_tile = [&](Tile8& t, int c) __attribute__((always_inline)) {
        const int blk = bt(c / CPB), ci = c % CPB;
        const uint4* Kp = reinterpret_cast<const uint4*>(kv + kv8_head_base(blk, 0, h) + (size_t)ci * CHUNK8) + k8_lane_piece(lane);
        const uint4* Vp = reinterpret_cast<const uint4*>(kv + kv8_head_base(blk, 1, h) + (size_t)ci * CHUNK8) + lane;
        const int npool = L - (FUSE ? 1 : 0) - c * CHUNK;       // tokens of this chunk that live in the pool (wave-uniform; >= 64 except in the last chunk)
        // the requests stay behind the last use of the registers they fill: hoisted into the arithmetic of the previous tile, they would keep
        // three tiles' worth of registers alive and spill at the 128-VGPR budget of four waves per SIMD
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) t.k[tt] = ld_nt(Kp + (16 * tt < npool ? tt * 64 : 0));
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) t.v[dt] = ld_nt(Vp + dt * 64);
        __builtin_amdgcn_sched_barrier(0);
    };

    // Order of the requests: the small operands of the prologue first (they retire first), then tile A -- of a chunk that exists even for a
    // wave without work (nc < NW), so that the request is unconditional; the RoPE arithmetic runs while it is in flight.  Tile B goes out
    // behind the arithmetic (in front of it, the prologue's operands and two tiles do not fit 128 registers), unconditionally as well: a wave
    // with a single chunk asks for tile A's lines again, which costs no HBM traffic, and keeps the steady part's waits counted.
    const int nmine = wave < nc ? (nc - wave + NW - 1) / NW : 0;      // chunks of this wave: wave + i NW, i < nmine
    Tile8 A, B;
    uint4 qfrag[2];                                 // B operand: q[32 ds + 8 kg .. +7], the same in all 16 columns
    if constexpr (FUSE) {
        // RoPE of this head's q and k exactly as rope_kv_fp8_kernel does it; the newest token is quantised BEFORE it joins the tile, so it
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
        const uint2 lo = q8_bf8(k1), hi = q8_bf8(k2);
        const uint4 knq = make_uint4(lo.x, lo.y, hi.x, hi.y);        // the newest key, quantised: the lane's piece (kg)
        const uint32_t vnq = q8_x4(bf2f(v0), bf2f(v1), bf2f(v2), bf2f(v3));      // the newest value, quantised: byte dt = dim 16 dt + col
        if (wave == 0 && col == 0) {                // paged write of the newest K: four lanes, one 64-byte line per (row, head), early
            const int blk = bt(pos / KV_BLOCK), tok = pos % KV_BLOCK;
            *reinterpret_cast<uint4*>(reinterpret_cast<uint8_t*>(a.kv_layer_w) + kv8_head_base(blk, 0, h) + k8_off(tok, kg)) = knq;
        }                                           // V goes back as patched half pieces from the wave that holds the last tile (compute)
        // the newest key / value wait in the wave's LDS corner until its last chunk: 5 registers less across the chunk loop, which sits at
        // the 128-VGPR budget of four waves per SIMD
        stash[0] = knq.x; stash[64] = knq.y; stash[128] = knq.z; stash[192] = knq.w; stash[256] = vnq;
        asm volatile("" ::: "memory");
    } else {
        const uint16_t* qsrc = a.q + (size_t)row * D + h * HD + kg * 8;
        qfrag[0] = *reinterpret_cast<const uint4*>(qsrc); qfrag[1] = *reinterpret_cast<const uint4*>(qsrc + 32);
        asm volatile("" ::: "memory");
        load_tile(A, min(wave, nc - 1));
    }

    // LAST: the tile may be the context's last chunk (only a wave's final chunk can be)
    auto compute = [&](Tile8& t, int c, auto last_tag) __attribute__((always_inline)) {
        constexpr bool LAST = decltype(last_tag)::value;
        if (LAST && c == nc - 1) {
            // pieces that hold no token of the pool are zeroed: their scores are masked anyway, but a V piece meets p = 0 in the MFMA and
            // 0 x (stale bits, which may spell NaN) would not be 0
            const int npool = L - (FUSE ? 1 : 0) - c * CHUNK;
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) if (16 * tt >= npool) t.k[tt] = make_uint4(0, 0, 0, 0);
            if (npool <= 0) {
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) t.v[dt] = make_uint4(0, 0, 0, 0);
            }
        }
        if (FUSE && LAST && c == nc - 1) {          // the newest token is patched into the last tile
            const uint4 knq = make_uint4(stash[0], stash[64], stash[128], stash[192]);
            const uint32_t vnq = stash[256];
            const int tc = L - 1 - c * CHUNK;
            const int tts = tc >> 4, ts = tc & 15, half = tc >> 5, kgs = (tc & 31) >> 3, bi = half * 8 + (tc & 7);
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                const bool hit = (tt == tts) && (col == ts);
                t.k[tt].x = hit ? knq.x : t.k[tt].x; t.k[tt].y = hit ? knq.y : t.k[tt].y;
                t.k[tt].z = hit ? knq.z : t.k[tt].z; t.k[tt].w = hit ? knq.w : t.k[tt].w;
            }
            if (kg == kgs) {
                // Paged write of the newest V: one token is 64 single bytes 16 bytes apart.  The patched half pieces (8 consecutive tokens of one dim)
                // ARE the pool's content with the new token merged in: the 16 lanes of the token's group write theirs back, 8 bytes each; the other
                // half of the piece (32 tokens away) is not touched.
                const int blk = bt(c / CPB), ci = c % CPB;
                uint8_t* Vw = reinterpret_cast<uint8_t*>(a.kv_layer_w) + kv8_head_base(blk, 1, h) + (size_t)ci * CHUNK8 + lane * 16 + half * 8;
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    patch8(t.v[dt], bi, (vnq >> (8 * dt)) & 0xffu);
                    *reinterpret_cast<uint2*>(Vw + dt * 1024) = half ? make_uint2(t.v[dt].z, t.v[dt].w) : make_uint2(t.v[dt].x, t.v[dt].y);
                }
            }
        }
        // ---- scores on the matrix cores: D[token][col] = K[token][:] . q
        f32x4 sacc[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            sacc[tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
            sacc[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(dq8_frag(t.k[tt].x, t.k[tt].y)), as_frag(qfrag[0]), sacc[tt], 0, 0, 0);
            sacc[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(dq8_frag(t.k[tt].z, t.k[tt].w)), as_frag(qfrag[1]), sacc[tt], 0, 0, 0);
        }
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
        pbuf[lane] = (p < 0x1p-100f) ? (uint16_t)0 : (uint16_t)f2bf(p);
        asm volatile("" ::: "memory");
        uint4 pfrag[2];                             // B operand: p[32 ts + 8 kg .. +7] as bf16, the same in all 16 columns
        pfrag[0] = *reinterpret_cast<const uint4*>(pbuf + 8 * kg);
        pfrag[1] = *reinterpret_cast<const uint4*>(pbuf + 32 + 8 * kg);
        // ---- P.V on the matrix cores: D[dim][col] = sum_token V[token][dim] * p[token]
        f32x4 oacc[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            oacc[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
            oacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(dq8_frag(t.v[dt].x, t.v[dt].y)), as_frag(pfrag[0]), oacc[dt], 0, 0, 0);
            oacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(dq8_frag(t.v[dt].z, t.v[dt].w)), as_frag(pfrag[1]), oacc[dt], 0, 0, 0);
        }
        if (col == 0) {
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                *reinterpret_cast<float4*>(po + c * 64 + 16 * dt + 4 * kg) = make_float4(oacc[dt][0], oacc[dt][1], oacc[dt][2], oacc[dt][3]);
        }
        if (lane == 0) { pm[c] = m; pl[c] = lsum; }
        asm volatile("" ::: "memory");              // the next chunk reuses sbuf / pbuf
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
// Prefill form over the FP8 pool: one workgroup per (head, 16 consecutive rows of the launch), the segment logic, register layout and fold of
// attention_tile_kernel; a raw tile is 32 registers, dequantised piece by piece in front of its MFMAs.
// ------------------------------------------------------------------------------------------------
constexpr int TILE8_OS = 68;            // floats per (chunk, row) line of partial outputs (64 + padding against LDS bank conflicts)
constexpr int TILE8_PS = 72;            // bf16 per row of a wave's probability image
__global__ __launch_bounds__(256, 2) void attention_tile_fp8_kernel(AttnArgs a, int row_base, int chunks_cap) {
    extern __shared__ __attribute__((aligned(16))) float part[];   // [cap][16][TILE8_OS] o | [cap][16] m | [cap][16] l | per wave: [16][TILE8_PS] bf16 p
    float* po = part; float* pm = part + (size_t)chunks_cap * 16 * TILE8_OS; float* pl = pm + chunks_cap * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint16_t* pimg = reinterpret_cast<uint16_t*>(pl + chunks_cap * 16) + wave * (16 * TILE8_PS);
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
            Tile8 t;
            {
                const int blk = bt[c / CPB], ci = c % CPB;
                const uint4* Kp = reinterpret_cast<const uint4*>(kv + kv8_head_base(blk, 0, h) + (size_t)ci * CHUNK8) + k8_lane_piece(lane);
                const uint4* Vp = reinterpret_cast<const uint4*>(kv + kv8_head_base(blk, 1, h) + (size_t)ci * CHUNK8) + lane;
#pragma unroll
                for (int f = 0; f < 4; ++f) t.k[f] = Kp[f * 64];
#pragma unroll
                for (int f = 0; f < 4; ++f) t.v[f] = Vp[f * 64];
            }
            f32x4 sacc[4];                          // sacc[tt][r] = score of token 16 tt + 4 kg + r of the chunk for row col
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                sacc[tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
                sacc[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(dq8_frag(t.k[tt].x, t.k[tt].y)), as_frag(qfrag[0]), sacc[tt], 0, 0, 0);
                sacc[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(dq8_frag(t.k[tt].z, t.k[tt].w)), as_frag(qfrag[1]), sacc[tt], 0, 0, 0);
            }
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
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                uint32_t pk[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) pk[r] = (pr[tt][r] < 0x1p-100f) ? 0u : (uint32_t)f2bf(pr[tt][r]);
                *reinterpret_cast<uint2*>(pimg + col * TILE8_PS + 16 * tt + 4 * kg) = make_uint2(pk[0] | (pk[1] << 16), pk[2] | (pk[3] << 16));
            }
            asm volatile("" ::: "memory");          // wave-private LDS exchange (a wave's DS operations execute in order)
            uint4 pfrag[2];
            pfrag[0] = *reinterpret_cast<const uint4*>(pimg + col * TILE8_PS + 8 * kg);
            pfrag[1] = *reinterpret_cast<const uint4*>(pimg + col * TILE8_PS + 32 + 8 * kg);
            asm volatile("" ::: "memory");
            if (kg == 0) { pm[c * 16 + col] = m; pl[c * 16 + col] = lsum; }
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                f32x4 oacc = (f32x4){0.f, 0.f, 0.f, 0.f};
                oacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(dq8_frag(t.v[dt].x, t.v[dt].y)), as_frag(pfrag[0]), oacc, 0, 0, 0);
                oacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(dq8_frag(t.v[dt].z, t.v[dt].w)), as_frag(pfrag[1]), oacc, 0, 0, 0);
                *reinterpret_cast<float4*>(po + (size_t)(c * 16 + col) * TILE8_OS + 16 * dt + 4 * kg) = make_float4(oacc[0], oacc[1], oacc[2], oacc[3]);
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
                    const float4 oc = *reinterpret_cast<const float4*>(po + (size_t)(c * 16 + row) * TILE8_OS + d4);
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

// Same dispatch as launch_attention: prefill rows [tile_from, rows) of an unfused launch take the tile kernel while its partials fit the
// CU's LDS, everything else the per-row kernel with 8 waves up to 8 rows and 4 beyond.  No measurement switches: this path has none.
hipError_t launch_attention_fp8(const AttnArgs& a, hipStream_t s) {
    if (a.rows <= 0) return hipSuccess;
    const int cap = a.tile_chunks > 0 ? min(a.tile_chunks, a.max_chunks) : a.max_chunks;
    const size_t lds_t = ((size_t)cap * 16 * (TILE8_OS + 2)) * sizeof(float) + (size_t)4 * 16 * TILE8_PS * 2;
    constexpr size_t LDS_PER_CU = 160 * 1024;
    if (!a.qkv && a.tile_from >= 0 && a.tile_from < a.rows && lds_t <= LDS_PER_CU) {
        static size_t raised[MAX_DEVICES] = {};
        size_t& have = raised[cur_device()];
        if (have < 64 * 1024) have = 64 * 1024;
        if (lds_t > have) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(attention_tile_fp8_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_t);
            if (e != hipSuccess) return e;
            have = lds_t;
        }
        hipLaunchKernelGGL(attention_tile_fp8_kernel, dim3(H, (a.rows - a.tile_from + 15) / 16), dim3(256), lds_t, s, a, a.tile_from, cap);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess || a.tile_from == 0) return e;
        AttnArgs head = a; head.rows = a.tile_from; head.tile_from = -1;
        return launch_attention_fp8(head, s);
    }
    if ((size_t)a.max_chunks * CHUNK > (size_t)64 * KV_BLOCK) return hipErrorInvalidValue;      // the per-row kernel keeps a row's block ids one per lane
    const int nw = a.force_waves == 4 || a.force_waves == 8 ? a.force_waves : (a.rows <= 8 ? 8 : 4);
    const dim3 grid(H, a.rows);
    const size_t lds = ((size_t)a.max_chunks * 66 + (size_t)nw * (96 + (a.qkv ? 5 * 64 : 0))) * sizeof(float);
    if (nw == 8) { if (a.qkv) launch_k((attention_fp8_kernel<8, true>), grid, dim3(512), lds, s, a); else launch_k((attention_fp8_kernel<8, false>), grid, dim3(512), lds, s, a); }
    else { if (a.qkv) launch_k((attention_fp8_kernel<4, true>), grid, dim3(256), lds, s, a); else launch_k((attention_fp8_kernel<4, false>), grid, dim3(256), lds, s, a); }
    return hipGetLastError();
}

}  // namespace t3
