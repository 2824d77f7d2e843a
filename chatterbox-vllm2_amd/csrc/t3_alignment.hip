// Text-speech alignment tap for gfx950 (MI355X, CDNA4): the attention PROBABILITIES one head of one layer pays to a span of its context,
// written out as fp32.  wave = 64 lanes.  Compile with -ffp-contract=off.
//
// What it is for: Chatterbox's AlignmentStreamAnalyzer is built on the attention that three Llama heads (LLAMA_ALIGNED_HEADS) pay to the
// text positions of the prompt while each speech frame is generated.  The fused decode attention (t3_attention.hip) keeps its probabilities
// in registers and LDS; this kernel recomputes them for ONE head of the sampled conditional rows, K only:
//
//     P[j] = softmax_j( q . K_j / 8 )      over the row's whole causal context j = 0 .. pos,      out[t] (+)= P[lo + t],  t < n_text
//
// with q the row's pre-RoPE query rotated here by rope8() with the table row the attention used (nothing rotated is read from anywhere, so
// one path serves prefill-last-row, decode and mixed steps) and K as the pool stores it (bf16, or the dequantised E4M3 / MXFP4 value).
//
// Split: one workgroup of 4 waves per sampled row; wave w takes the 64-token chunks w, w + 4, ...  A chunk's K is 8 fully coalesced 1 KiB
// wave loads (FP8 pool: 4, MXFP4 pool: 2 and 8 scale bytes) straight into MFMA A operands; q is replicated over the 16 B columns (v_mfma_f32_16x16x32_bf16: the products
// and the fp32 accumulation of the attention kernel).  No V is touched: a tap costs 128 B x context per row (FP8: 64 B).  Scores x 1/8 go
// to an LDS strip [max_chunks x 64] fp32 with the per-chunk maxima beside it.  Behind a barrier M = max over chunks; every wave turns its own
// chunks of the strip into e_j = t3_expf(s_j - M) IN PLACE and leaves the chunk's butterfly sum (contract pairing: xor 32, 16, 8, 4, 2, 1);
// behind a second barrier l = the chunk sums folded in ascending chunk order, and all 256 threads write e_j / l for j in the span as
// coalesced fp32 stores.  (Two barriers where one would do: with one, every output thread would evaluate the polynomial exp a second time
// for the span on top of the pass that forms l; the strip already holds the value.)  Every order is fixed, so a row's numbers do not depend
// on the launch form (eager, graph, burst) nor on what else is in the batch.
//
// Taps of several layers accumulate into one matrix: they run in ascending layer order on one stream, the first stores, later ones add,
// the last one scales by 1 / n_taps -- plain vector stores, no atomics.
#include "t3_kernels.h"
#include "t3_device.h"
#include "t3_attention_common.h"

#include <math.h>
#include <algorithm>

namespace t3 {

template <int FMT>      // T3EngineConfig.kv_cache_dtype: 0 bf16, 1 FP8 E4M3, 4 MXFP4
__global__ __launch_bounds__(256) void alignment_kernel(AlignArgs a) {
    extern __shared__ __attribute__((aligned(16))) float strip[];      // [max_chunks][64] scores, then e | [max_chunks] chunk max | [max_chunks] chunk sum
    float* cm = strip + (size_t)a.max_chunks * CHUNK; float* cl = cm + a.max_chunks;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row = a.sel_rows ? a.sel_rows[2 * blockIdx.x] : (int)blockIdx.x;
    const int* rec = a.rowrec + (size_t)row * a.row_stride;
    const int frame = rec[ROW_ALIGN_FRAME];
    if (frame < 0) return;                          // not tapped (uniform over the workgroup): the grid stays a function of the step's shape
    const int n_text = rec[ROW_ALIGN_NTEXT];
    const int L = min(rec[1] + 1, a.max_chunks * CHUNK);      // never beyond the strip
    const int nc = (L + CHUNK - 1) / CHUNK;
    const int h = a.head, col = lane & 15, kg = lane >> 4;
    constexpr int CPB = KV_BLOCK / CHUNK;

    // ---- q: RoPE of the head's pre-RoPE query exactly as rope_kv_kernel / the fused attention do it (lane = (col, kg): rotation pairs 8 kg + j)
    uint4 qfrag[2];                                 // B operand: q[32 ds + 8 kg .. +7], the same in all 16 columns
    {
        const int pos = rec[1];
        const uint16_t* src = a.qkv + (size_t)row * QKV + h * HD;
        const float4* cp = reinterpret_cast<const float4*>(a.cos_t + (size_t)pos * 32 + kg * 8);
        const float4* sp = reinterpret_cast<const float4*>(a.sin_t + (size_t)pos * 32 + kg * 8);
        const float4 c0 = cp[0], c1 = cp[1], s0 = sp[0], s1 = sp[1];
        const float c[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w}, s[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
        rope8(*reinterpret_cast<const uint4*>(src + kg * 8), *reinterpret_cast<const uint4*>(src + 32 + kg * 8), c, s, qfrag[0], qfrag[1]);
        if (a.q_rot_out && wave == 0 && col == 0) {      // parity hook: the q this tap used
            uint16_t* qo = a.q_rot_out + (size_t)row * HD;
            *reinterpret_cast<uint4*>(qo + kg * 8) = qfrag[0]; *reinterpret_cast<uint4*>(qo + 32 + kg * 8) = qfrag[1];
        }
    }

    // ---- scores of the wave's chunks -> strip, chunk maxima -> cm
    for (int c = wave; c < nc; c += 4) {
        const int blk = rec[ROW_HDR + c / CPB], ci = c % CPB;
        const int npool = L - c * CHUNK;            // tokens of this chunk (wave-uniform; >= 64 except in the last chunk)
        uint4 kf[8];                                // A operands: fragment (tt, ds) at 2 tt + ds
        // of the context's last chunk only the fragments that hold tokens are requested; the rest are zeroed (their scores are masked)
        if constexpr (FMT == 4) {
            // two 16-byte pieces (token tiles 2 j, 2 j + 1) and the lane's eight scale bytes; the second piece only where it holds tokens
            const uint8_t* Kb = reinterpret_cast<const uint8_t*>(a.kv_layer) + kv4_head_base(blk, 0, h) + (size_t)ci * CHUNK4_REC;
            const uint4* Kp = reinterpret_cast<const uint4*>(Kb) + k_lane_piece(lane);
            const uint4 k4[2] = {ld_nt(Kp), 32 < npool ? ld_nt(Kp + 64) : make_uint4(0, 0, 0, 0)};
            const uint2 ks = *reinterpret_cast<const uint2*>(Kb + CHUNK4 + 8 * col);
            kf[0] = k4_frag<0, 0>(k4, ks); kf[1] = k4_frag<0, 1>(k4, ks); kf[2] = k4_frag<1, 0>(k4, ks); kf[3] = k4_frag<1, 1>(k4, ks);
            kf[4] = k4_frag<2, 0>(k4, ks); kf[5] = k4_frag<2, 1>(k4, ks); kf[6] = k4_frag<3, 0>(k4, ks); kf[7] = k4_frag<3, 1>(k4, ks);
        } else if constexpr (FMT == 1) {
            const uint4* Kp = reinterpret_cast<const uint4*>(reinterpret_cast<const uint8_t*>(a.kv_layer) + kv8_head_base(blk, 0, h) + (size_t)ci * CHUNK8) + k8_lane_piece(lane);
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {        // one 16-byte piece carries both halves (ds = 0, 1) of the lane's operands
                const uint4 p = 16 * tt < npool ? ld_nt(Kp + tt * 64) : make_uint4(0, 0, 0, 0);
                kf[2 * tt] = dq8_frag(p.x, p.y); kf[2 * tt + 1] = dq8_frag(p.z, p.w);
            }
        } else {
            const uint4* Kp = reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(a.kv_layer) + kv_head_base(blk, 0, h) + (size_t)ci * (CHUNK * HD)) + k_lane_piece(lane);
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                const bool in = 16 * tt < npool;
                kf[2 * tt] = in ? ld_nt(Kp + (2 * tt) * 64) : make_uint4(0, 0, 0, 0);
                kf[2 * tt + 1] = in ? ld_nt(Kp + (2 * tt + 1) * 64) : make_uint4(0, 0, 0, 0);
            }
        }
        f32x4 sacc[4];                              // D[token][col] = K[token][:] . q
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            sacc[tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
            sacc[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(kf[2 * tt]), as_frag(qfrag[0]), sacc[tt], 0, 0, 0);
            sacc[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(kf[2 * tt + 1]), as_frag(qfrag[1]), sacc[tt], 0, 0, 0);
        }
        float* sc = strip + c * CHUNK;
        if (col == 0) {                             // lanes 0, 16, 32, 48 hold every score once: rows 4 kg + r of each token tile
#pragma unroll
            for (int tt = 0; tt < 4; ++tt)
                *reinterpret_cast<float4*>(sc + 16 * tt + 4 * kg) = make_float4(sacc[tt][0] * 0.125f, sacc[tt][1] * 0.125f, sacc[tt][2] * 0.125f, sacc[tt][3] * 0.125f);
        }
        asm volatile("" ::: "memory");              // wave-private LDS exchange: keep the read below the writes (a wave's DS operations execute in order)
        const float m = wave_max_f32(lane < npool ? sc[lane] : -INFINITY, lane);
        if (lane == 0) cm[c] = m;
    }
    __syncthreads();
    float M = -INFINITY;
    for (int c0 = 0; c0 < nc; c0 += 64) M = fmaxf(M, c0 + lane < nc ? cm[c0 + lane] : -INFINITY);
    M = wave_max_f32(M, lane);
    // ---- e_j = exp(s_j - M) in place, per-chunk butterfly sums
    for (int c = wave; c < nc; c += 4) {
        float* sc = strip + c * CHUNK;
        const float e = c * CHUNK + lane < L ? t3_expf(sc[lane] - M) : 0.0f;
        sc[lane] = e;
        const float lsum = wave_bfly_add_f32(e, lane);
        if (lane == 0) cl[c] = lsum;
    }
    __syncthreads();
    float l = 0.0f;
    for (int c = 0; c < nc; ++c) l = l + cl[c];     // ascending chunk order, the same in every thread
    // ---- the span [lo, lo + n_text) of the row, positions beyond the context are 0
    float* dst = a.out + ((size_t)(rec[0] >> 1) * a.frames_per_slot + frame) * a.ld;
    for (int t = tid; t < n_text; t += 256) {
        const int j = a.lo + t;
        float p = j < L ? strip[j] / l : 0.0f;
        if (a.tap > 0) p = dst[t] + p;
        if (a.tap == a.n_taps - 1) p = p * a.inv_taps;
        dst[t] = p;
    }
}

hipError_t launch_alignment(const AlignArgs& a, int kv_dtype, hipStream_t s) {
    if (a.n_wg <= 0) return hipSuccess;
    const size_t lds = (size_t)a.max_chunks * (CHUNK + 2) * sizeof(float);      // 4.1 KiB at max_model_len 1000, 33 KiB at 8192: under the 64 KiB every kernel may ask for
    if (lds > 64 * 1024) return hipErrorInvalidValue;      // a context beyond 15 872 tokens: the engine stops at 8192 (t3_create), the parity hook checks max_pos
    if (kv_dtype == 4) launch_k(alignment_kernel<4>, dim3(a.n_wg), dim3(256), lds, s, a);
    else if (kv_dtype == 1) launch_k(alignment_kernel<1>, dim3(a.n_wg), dim3(256), lds, s, a);
    else if (kv_dtype == 0) launch_k(alignment_kernel<0>, dim3(a.n_wg), dim3(256), lds, s, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// Stream-ordered clear of a slot's frame buffer (a kernel, not a memset node: the engine's steps may be recorded into graphs)
__global__ __launch_bounds__(256) void alignment_clear_kernel(float4* p, size_t n4) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) p[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}
hipError_t launch_alignment_clear(float* p, size_t n, hipStream_t s) {      // n a multiple of 4, p 16-byte aligned
    if (n == 0) return hipSuccess;
    const size_t n4 = n / 4;
    hipLaunchKernelGGL(alignment_clear_kernel, dim3((unsigned)std::min<size_t>((n4 + 255) / 256, 1024)), dim3(256), 0, s, reinterpret_cast<float4*>(p), n4);
    return hipGetLastError();
}

}  // namespace t3
