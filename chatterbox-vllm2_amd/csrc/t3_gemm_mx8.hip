// The layer projections over MXFP8 weights for gfx950 (MI355X, CDNA4): the host quantiser / packer of t3_finalize_weights
// (t3_set_weight_dtype = 1) and the one GEMM kernel that reads what it packs.  wave = 64 lanes.
//
// Format (OCP microscaling, E4M3 elements, one E8M0 scale per 32): an MX block is 32 consecutive k of one output row n of the matrix the
// bf16 engine would pack (norm weight folded in already).  With E the biased exponent field of the block's max |w|:
//     b = max(E - 8, 0) (the scale byte),  X = 2^(b - 127),  element = e4m3fn(rne(clamp(w / X, -448, 448))),  stored value = X * element
// (q8 is the FP8 pool's, t3_attention_fp8.hip).  E4M3 has three mantissa bits and X is a power of two, so every stored value of a block in
// bf16's normal range is a bf16 value: the kernel rebuilds it EXACTLY with v_cvt_scalef32_pk_bf16_fp8 under the block's scale, directly in
// front of the bf16 MFMA that reads it, and the result is bit for bit the bf16 engine's over the dequantised matrix.  The numerics contract
// of DESIGN.md section 3 is untouched: K cut into one segment per wave (4 x 256: qkv, gate/up; 16 x 64: o; 16 x 256: down), a segment = one
// chain of v_mfma_f32_16x16x32_bf16 from +0 in ascending k, ((s0 + s1) + s2) + s3 and ((G0 + G1) + G2) + G3, the RMSNorm statistic from
// the MFMA diagonal of the activations, rstd in the epilogue.
//
// Packed layout (pack_weight_mx8): one MX block is one k-block of one row of an MFMA B operand, i.e. the eight values a lane holds share a scale.
//   data   [n-tile][k-block pair kp][lane][16 B]: bytes 8 h .. 8 h + 7 = W[16 nt + lane % 16][32 (2 kp + h) + 8 (lane / 16) + 0 .. 7]
//          -- a wave's load of two k-blocks of a tile is one contiguous, coalesced 1 KiB, as the bf16 tiles' is of one;
//   scales [n-tile][segment][row c of the tile][KBS bytes], behind the data: a wave's scales of a tile are ONE load of 16 * KBS contiguous
//          bytes (KBS = k-blocks per segment: 8, or 2 for o), lane (c, q) reading the KBS bytes of row c.
//
// Schedule (gemm_mx8_kernel, the same for every row count): weights stationary.  A workgroup owns NT n-tiles and every blockIdx.y-th 16-row
// group; wave w keeps its K segment of those tiles in registers as OCTETS -- 2 registers per (tile, k-block), 16 per tile and 256-wide
// segment where the bf16 forms hold 32 -- and walks the groups.  Per group: the wave's slice of the 16 rows comes as full row segments into
// a wave-private XOR-swizzled LDS image (no barrier: a wave's DS operations execute in order); the next group's rows are requested from
// global memory before this group's MFMAs and wait in registers; the A fragments are read from the image a few k-blocks ahead; each octet
// is converted in front of its MFMA.  The partial sums overwrite the wave's own (dead) image, one barrier hands them to ALL waves, which
// fold and finish one column pair per thread, a second barrier frees the images for the rows that are waiting.
// Every load is an ordinary, compiler-counted load: no hand-counted waits in this file.
#include "t3_kernels.h"
#include "t3_device.h"

#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

namespace t3 {
// ------------------------------------------------------------------------------------------------
// device
// ------------------------------------------------------------------------------------------------
typedef __bf16 mx8_bf16x2 __attribute__((ext_vector_type(2)));
// E8M0 byte (bits 8 i .. 8 i + 7 of w) -> the fp32 operand of the scaled convert, 2^(b - 127); b = 0 is the fp32 subnormal 2^-127
template <int I> __device__ __forceinline__ float mx8_scale(uint32_t w) { return __uint_as_float(max(((w >> (8 * I)) & 0xffu) << 23, 0x00400000u)); }
template <bool HI> __device__ __forceinline__ uint32_t mx8_pair(uint32_t w, float s) {          // two e4m3 of the low / high half of w, times s -> packed bf16 pair
    union { mx8_bf16x2 v; uint32_t u; } c;
    c.v = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, s, HI);
    return c.u;
}
__device__ __forceinline__ bf16x8 mx8_frag(const uint2& o, float s) {                           // one octet under its block's scale -> an MFMA B fragment
    return as_frag(make_uint4(mx8_pair<false>(o.x, s), mx8_pair<true>(o.x, s), mx8_pair<false>(o.y, s), mx8_pair<true>(o.y, s)));
}
// byte offset of 16-byte chunk ch of row `row` in a wave's A image (rows of KBS * 64 bytes): the fragment read of a k-block (16 rows x 4 chunks)
// and the staging store (full rows) both spread over the banks
template <int KBS> __device__ __forceinline__ unsigned mx8_img_off(int row, int ch) {
    if constexpr (KBS == 8) return (unsigned)(row * 512 + ((ch ^ (row & 15)) << 4));
    else return (unsigned)(row * 128 + ((ch ^ ((row >> 1) & 7)) << 4));
}

// a wave's slice of the 16 rows of group g: instruction t covers rows t * RPI .. of the group, a lane one 16-byte chunk (xw: the lane's chunk of row 0)
template <int KBS> __device__ __forceinline__ void mx8_issue_a(u32x4 (&ar)[KBS], const uint16_t* xw, int M, int K, int g, int rsub) {
#pragma unroll
    for (int t = 0; t < KBS; ++t) {
        int m = g * 16 + t * (16 / KBS) + rsub;
        m = m < M ? m : M - 1;                                     // padded rows re-read the last row; their outputs are dropped
        ar[t] = *reinterpret_cast<const u32x4*>(xw + (size_t)m * K);
    }
}
template <int KBS> __device__ __forceinline__ void mx8_stage_a(const u32x4 (&ar)[KBS], unsigned char* img, int rsub, int ch) {
#pragma unroll
    for (int t = 0; t < KBS; ++t) *reinterpret_cast<u32x4*>(img + mx8_img_off<KBS>(t * (16 / KBS) + rsub, ch)) = ar[t];
}

// NT packed n-tiles per workgroup (EPI_SILU: NT / 2 (gate, up) pairs), NW waves = K segments of KBS k-blocks.  NW = 4: the NORM forms
// (EPI_BF16 qkv, EPI_SILU gate/up; K = 1024); NW = 16: EPI_RESID (o: KBS 2, down: KBS 8).
template <int NT, int EPI, int NW, int KBS>
__global__ __launch_bounds__(NW * 64) void gemm_mx8_kernel(Mx8GemmArgs a) {
    static_assert((NW == 4 && KBS == 8 && (EPI == EPI_BF16 || EPI == EPI_SILU)) || (NW == 16 && (KBS == 2 || KBS == 8) && EPI == EPI_RESID), "gemm_mx8 forms");
    constexpr bool NORM = NW == 4;
    constexpr int LPR = KBS * 4;                                   // lanes (16-byte chunks) per row slice: a wave instruction covers 16 / KBS rows
    constexpr int WREG = (KBS > NT ? KBS : NT) * 1024;             // a wave's LDS region: its A image (KBS KiB), then its partials (NT KiB)
    constexpr int NU = EPI == EPI_SILU ? 2 : 1, NTO = NT / NU;     // packed tiles per output tile, output tiles per workgroup
    constexpr int PIECES = NTO * 128, TH = NW * 64;                // a group's outputs in column pairs
    constexpr int AFD = (NW == 16 && KBS == 8) ? 3 : KBS;          // A fragments this many k-blocks ahead of their MFMAs (128 registers at 16 waves)
    // down (16 waves x 8 k-blocks, 128 registers per wave): the next group's rows (32 registers) are requested behind the MFMAs, not ahead of them,
    // and fly under the fold and its two barriers
    constexpr bool LATE_A = NW == 16 && KBS == 8;
    static_assert(EPI != EPI_RESID || PIECES <= TH, "the residual operand is one prefetched word per thread");
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_mx8[];      // [NW] wave regions | float [NW][16] row statistic
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, q = lane >> 4;
    const int KB = a.K >> 5, kb0 = wave * KBS;
    unsigned char* img = lds_mx8 + (size_t)wave * WREG;
    float* rowsum = reinterpret_cast<float*>(lds_mx8 + (size_t)NW * WREG);
    const int mgroups = (a.M + 15) / 16, g0 = blockIdx.y, gs = gridDim.y;
    if (g0 >= mgroups) return;                                     // the whole workgroup
    const int ng = (mgroups - g0 + gs - 1) / gs;

    // ---- this wave's slice of a group's rows: KBS instructions of 16 / KBS full row segments each (mx8_issue_a / mx8_stage_a)
    const int rsub = lane / LPR, ch = lane % LPR;
    const uint16_t* xw = a.X + kb0 * 32 + ch * 8;
    u32x4 ar[KBS];
    mx8_issue_a<KBS>(ar, xw, a.M, a.K, g0, rsub);
    // ---- the stationary operand: octets and scale bytes of this wave's segment of the workgroup's NT tiles
    uint2 wq[NT][KBS];
    uint32_t sb[NT][KBS == 8 ? 2 : 1];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const size_t tile = (size_t)blockIdx.x * NT + t;
#pragma unroll
        for (int kp = 0; kp < KBS / 2; ++kp) {
            const uint4 v = ld_nt(a.Wq + (tile * (KB >> 1) + (kb0 >> 1) + kp) * 64 + lane);
            wq[t][2 * kp] = make_uint2(v.x, v.y); wq[t][2 * kp + 1] = make_uint2(v.z, v.w);
        }
        const unsigned char* sp = a.Ws + (tile * KB + kb0) * 16 + c * KBS;
        if constexpr (KBS == 8) { const uint2 s = *reinterpret_cast<const uint2*>(sp); sb[t][0] = s.x; sb[t][1] = s.y; }
        else sb[t][0] = *reinterpret_cast<const uint16_t*>(sp);
    }
    mx8_stage_a<KBS>(ar, img, rsub, ch);

    // this thread's piece of a group's outputs: column pair l2 % 8 of output tile `to`, row 4 (l2 / 8) + r -- 32 consecutive threads read one
    // contiguous 256-byte plane [r] of a tile's partials
    auto piece_row = [](int p) { return 4 * ((p & 31) >> 3) + ((p >> 5) & 3); };
    for (int j = 0; j < ng; ++j) {
        const int g = g0 + j * gs;
        const bool more = j + 1 < ng;
        uint32_t hres = 0;
        if constexpr (EPI == EPI_RESID) {                          // the residual operand, ahead of everything it could wait behind
            const int m = g * 16 + piece_row(tid), n = (blockIdx.x * NTO + (tid >> 7)) * 16 + 2 * (tid & 7);
            if (tid < PIECES && m < a.M && n < a.N) hres = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint16_t*>(a.out) + (size_t)m * a.ldo + n);
        }
        if (!LATE_A && more) mx8_issue_a<KBS>(ar, xw, a.M, a.K, g + gs, rsub);      // the next group's rows fly while this one is on the matrix cores
        // the octets stay octets: without this (empty) statement hipcc hoists the group-invariant converts out of the group loop and keeps the
        // tiles as bf16, 32 registers per tile again
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int kb = 0; kb < KBS; ++kb) asm volatile("" : "+v"(wq[t][kb].x), "+v"(wq[t][kb].y));
        f32x4 acc[NT], ss = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        uint4 afr[AFD];
#pragma unroll
        for (int d = 0; d < AFD; ++d) afr[d] = *reinterpret_cast<const uint4*>(img + mx8_img_off<KBS>(c, 4 * d + q));
#pragma unroll
        for (int kb = 0; kb < KBS; ++kb) {
            const uint4 af = afr[kb % AFD];
            if (kb + AFD < KBS) afr[kb % AFD] = *reinterpret_cast<const uint4*>(img + mx8_img_off<KBS>(c, 4 * (kb + AFD) + q));
            if constexpr (NORM) ss = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(af), as_frag(af), ss, 0, 0, 0);      // diagonal = sum of squares
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const uint32_t sw = sb[t][kb >> 2];
                const float s = (kb & 3) == 0 ? mx8_scale<0>(sw) : (kb & 3) == 1 ? mx8_scale<1>(sw) : (kb & 3) == 2 ? mx8_scale<2>(sw) : mx8_scale<3>(sw);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(af), mx8_frag(wq[t][kb], s), acc[t], 0, 0, 0);
            }
        }
        if (LATE_A && more) mx8_issue_a<KBS>(ar, xw, a.M, a.K, g + gs, rsub);
        // ---- partials over the wave's own image (dead: the MFMAs above consumed every fragment): [tile][r][lane]
        float* red = reinterpret_cast<float*>(img);
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[(t * 4 + r) * 64 + lane] = acc[t][r];
        if constexpr (NORM) {
            // D[row = 4 q + r][col = c]: the diagonal element of row c sits in lane group q = c / 4, register c % 4
            const int r = c & 3;
            const float d = r == 0 ? ss[0] : r == 1 ? ss[1] : r == 2 ? ss[2] : ss[3];
            if ((c >> 2) == q) rowsum[wave * 16 + c] = d;
        }
        __syncthreads();
        // ---- fold + epilogue: every wave, one column pair per thread and pass
        for (int p = tid; p < PIECES; p += TH) {
            const int l2 = p & 31, r = (p >> 5) & 3, to = p >> 7;
            const int r16 = piece_row(p), m = g * 16 + r16, n = (blockIdx.x * NTO + to) * 16 + 2 * (l2 & 7);
            if (m >= a.M || n >= a.N) continue;
            float v[NU][2];
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int o = ((NU * to + u) * 4 + r) * 64 + 2 * l2;
#pragma unroll
                for (int gq = 0; gq < NW / 4; ++gq) {
                    float2 s4 = *reinterpret_cast<const float2*>(lds_mx8 + (size_t)(4 * gq) * WREG + o * 4);
#pragma unroll
                    for (int w = 1; w < 4; ++w) {
                        const float2 sw = *reinterpret_cast<const float2*>(lds_mx8 + (size_t)(4 * gq + w) * WREG + o * 4);
                        s4.x = s4.x + sw.x; s4.y = s4.y + sw.y;
                    }
                    if (gq == 0) { v[u][0] = s4.x; v[u][1] = s4.y; } else { v[u][0] = v[u][0] + s4.x; v[u][1] = v[u][1] + s4.y; }
                }
            }
            uint32_t* op = reinterpret_cast<uint32_t*>(reinterpret_cast<uint16_t*>(a.out) + (size_t)m * a.ldo + n);
            if constexpr (NORM) {
                const float ssum = ((rowsum[r16] + rowsum[16 + r16]) + rowsum[32 + r16]) + rowsum[48 + r16];
                const float rstd = 1.0f / sqrtf(ssum * (1.0f / 1024.0f) + 1e-5f);
                uint32_t ob[2];
#pragma unroll
                for (int e = 0; e < 2; ++e)
                    ob[e] = EPI == EPI_SILU ? silu_mul_bf(f2bf(v[0][e] * rstd), f2bf(v[NU - 1][e] * rstd)) : f2bf(v[0][e] * rstd);
                *op = ob[0] | (ob[1] << 16);
            } else {
                // h = bf16(h + bf16(y))
                *op = f2bf(bf_lo(hres) + rbf(v[0][0])) | (f2bf(bf_hi(hres) + rbf(v[0][1])) << 16);
            }
        }
        if (more) {
            __syncthreads();                                       // every wave has read this group's partials
            mx8_stage_a<KBS>(ar, img, rsub, ch);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
// a == nullptr: only raise the kernel's dynamic-LDS limit (prepare_gemm_mx8, before any stream capture)
template <int NT, int EPI, int NW, int KBS>
static hipError_t launch_mx8_t(const Mx8GemmArgs* a, hipStream_t s) {
    constexpr size_t lds = (size_t)NW * (KBS > NT ? KBS : NT) * 1024 + (size_t)NW * 16 * sizeof(float);
    auto kern = gemm_mx8_kernel<NT, EPI, NW, KBS>;
    static bool raised[MAX_DEVICES] = {};
    if (lds > 64 * 1024 && !raised[cur_device()]) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        raised[cur_device()] = true;
    }
    if (!a) return hipSuccess;
    const int tiles = a->N / 16 * (EPI == EPI_SILU ? 2 : 1), gx = tiles / NT, mgroups = (a->M + 15) / 16;
    // one workgroup per CU where the tiles alone do not give that many: the row groups of a tile group are dealt to 256 / gx workgroups
    const int gy = std::max(1, std::min(mgroups, 256 / gx));
    launch_k(kern, dim3(gx, gy), dim3(NW * 64), lds, s, *a);
    return hipGetLastError();
}
// The tile group: the wide one (every row group re-read a quarter / half as often) where its workgroups still cover the chip, else the narrow one
template <int EPI, int NW, int KBS, int NT_NARROW, int NT_WIDE>
static hipError_t launch_mx8_nt(const Mx8GemmArgs& a, hipStream_t s) {
    const int tiles = a.N / 16 * (EPI == EPI_SILU ? 2 : 1), mgroups = (a.M + 15) / 16;
    if (tiles % NT_WIDE == 0 && (long)(tiles / NT_WIDE) * mgroups >= 256) return launch_mx8_t<NT_WIDE, EPI, NW, KBS>(&a, s);
    return launch_mx8_t<NT_NARROW, EPI, NW, KBS>(&a, s);
}
hipError_t launch_gemm_mx8(const Mx8GemmArgs& a, int epi, hipStream_t s) {
    if (a.M <= 0) return hipSuccess;
    if (a.N <= 0 || a.N % 16 || (a.ldo & 1) || !a.X || !a.Wq || !a.Ws || !a.out) return hipErrorInvalidValue;
    if (epi == EPI_BF16 && a.K == D) return launch_mx8_nt<EPI_BF16, 4, 8, 1, 4>(a, s);
    if (epi == EPI_SILU && a.K == D) return launch_mx8_nt<EPI_SILU, 4, 8, 2, 8>(a, s);
    if (epi == EPI_RESID && a.K == D) return launch_mx8_nt<EPI_RESID, 16, 2, 1, 4>(a, s);
    if (epi == EPI_RESID && a.K == F) return launch_mx8_t<1, EPI_RESID, 16, 8>(&a, s);      // two tiles of down do not fit 128 registers without spills
    return hipErrorInvalidValue;      // not a projection of the layer
}
hipError_t prepare_gemm_mx8() {
    hipError_t e;
    if ((e = launch_mx8_t<1, EPI_BF16, 4, 8>(nullptr, nullptr)) != hipSuccess) return e;
    if ((e = launch_mx8_t<4, EPI_BF16, 4, 8>(nullptr, nullptr)) != hipSuccess) return e;
    if ((e = launch_mx8_t<2, EPI_SILU, 4, 8>(nullptr, nullptr)) != hipSuccess) return e;
    if ((e = launch_mx8_t<8, EPI_SILU, 4, 8>(nullptr, nullptr)) != hipSuccess) return e;
    if ((e = launch_mx8_t<1, EPI_RESID, 16, 2>(nullptr, nullptr)) != hipSuccess) return e;
    if ((e = launch_mx8_t<4, EPI_RESID, 16, 2>(nullptr, nullptr)) != hipSuccess) return e;
    if ((e = launch_mx8_t<1, EPI_RESID, 16, 8>(nullptr, nullptr)) != hipSuccess) return e;
    return hipSuccess;
}

// ------------------------------------------------------------------------------------------------
// host: the quantiser of t3_finalize_weights and its inverse
// ------------------------------------------------------------------------------------------------
static inline float mx8_b2f(uint16_t b) { uint32_t u = (uint32_t)b << 16; float f; memcpy(&f, &u, 4); return f; }
static inline uint16_t mx8_f2b(float f) {
    uint32_t u; memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
// q8: e4m3fn(round-to-nearest-even(clamp(v, -448, 448))), NaN -> NaN
static uint8_t mx8_q8(float v) {
    uint32_t u; memcpy(&u, &v, 4);
    const uint8_t sign = (uint8_t)((u >> 24) & 0x80u);
    float x = fabsf(v);
    if (x != x) return sign | 0x7f;
    if (x > 448.0f) x = 448.0f;
    if (x < 0.015625f) return sign | (uint8_t)(int)rintf(x * 512.0f);      // below 2^-6: the subnormal grid of 2^-9 (8 = the smallest normal)
    int e; (void)frexpf(x, &e);                                              // x in [2^(e - 1), 2^e)
    int ex = e - 1, m = (int)rintf(ldexpf(x, 3 - ex));                       // 8 .. 16
    if (m == 16) { m = 8; ++ex; }
    return sign | (uint8_t)(((ex + 7) << 3) | (m - 8));
}
static float mx8_dq8(uint8_t code) {
    const int e = (code >> 3) & 15, m = code & 7;
    float x = (code & 0x7f) == 0x7f ? NAN : e == 0 ? ldexpf((float)m, -9) : ldexpf((float)(8 + m), e - 10);
    return (code & 0x80) ? -x : x;
}
// one MX block: 32 bf16 values -> 32 e4m3 elements and the scale byte
static uint8_t mx8_block(const uint16_t* w, uint8_t* elems) {
    uint32_t amax = 0;
    for (int i = 0; i < 32; ++i) amax = std::max(amax, (uint32_t)(w[i] & 0x7fffu));
    const int E = (int)(amax >> 7), b = std::max(E - 8, 0);
    const float X = ldexpf(1.0f, b - 127);
    for (int i = 0; i < 32; ++i) elems[i] = mx8_q8(mx8_b2f(w[i]) / X);
    return (uint8_t)b;
}
void mx8_roundtrip(const uint16_t* w, uint16_t* y, int rows, int cols) {
    uint8_t el[32];
    for (size_t blk = 0; blk < (size_t)rows * cols / 32; ++blk) {
        const float X = ldexpf(1.0f, (int)mx8_block(w + blk * 32, el) - 127);
        for (int i = 0; i < 32; ++i) y[blk * 32 + i] = mx8_f2b(X * mx8_dq8(el[i]));
    }
}
size_t mx8_packed_bytes(int N, int K) { return (size_t)N * K + (size_t)N * K / 32; }
void pack_weight_mx8(const uint16_t* W, int N, int K, int kbs, unsigned char* out) {
    const int KB = K / 32;
    unsigned char* scales = out + (size_t)N * K;
    uint8_t el[32];
    for (int nt = 0; nt < N / 16; ++nt)
        for (int c = 0; c < 16; ++c)
            for (int kb = 0; kb < KB; ++kb) {
                const uint8_t b = mx8_block(W + (size_t)(nt * 16 + c) * K + kb * 32, el);
                scales[((size_t)nt * KB + (kb / kbs) * kbs) * 16 + c * kbs + kb % kbs] = b;
                for (int qd = 0; qd < 4; ++qd)
                    memcpy(out + ((((size_t)nt * (KB / 2) + kb / 2) * 64 + 16 * qd + c) * 16 + (kb & 1) * 8), el + 8 * qd, 8);
            }
}
void pack_gate_up_mx8(const uint16_t* Wg, const uint16_t* Wu, int Fdim, int K, unsigned char* out) {
    std::vector<uint16_t> il((size_t)2 * Fdim * K);                 // packed tile 2 t = gate tile t, 2 t + 1 = up tile t (pack_gate_up)
    for (int t = 0; t < Fdim / 16; ++t) {
        memcpy(il.data() + (size_t)(2 * t) * 16 * K, Wg + (size_t)t * 16 * K, (size_t)16 * K * 2);
        memcpy(il.data() + (size_t)(2 * t + 1) * 16 * K, Wu + (size_t)t * 16 * K, (size_t)16 * K * 2);
    }
    pack_weight_mx8(il.data(), 2 * Fdim, K, 8, out);
}

}  // namespace t3
