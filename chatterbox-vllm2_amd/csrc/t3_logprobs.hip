// Per-token log-probabilities for gfx950 (MI355X, CDNA4): a kernel of its own directly behind the sampler.  wave = 64 lanes.  Compile with
// -ffp-contract=off.
//
// What it is for: the post-CFG logits exist only on the device and only for one step (the bf16 CFG mix of the two head rows happens inside
// sampler_kernel), so the log-probability of the id a step drew, its rank and the k most likely ids can only be taken here.  These are vLLM's
// RAW log-probabilities: over x_v = the post-CFG logit as sampler_kernel's phase A forms it (cfg_logit, t3_device.h -- the value t3_debug_logits
// reports), before penalties, temperature, min-p / top-k / top-p and the guard's suppression.  include/t3_engine.h ("per-token log-probabilities")
// spells the definitions out.
//
// Split: one workgroup of 256 threads per sampled utterance, grid = n_sel -- a function of the step's shape only, so a captured step stays valid
// whatever the slots hold.  A workgroup whose slot is not marked (lp_k[slot] < 0) or whose step lies beyond the record buffer leaves at once;
// the launch itself is only part of steps that sample a marked request (engine.cpp).
//
// Data movement: ids 0 .. 8191 are 1024 vectors of 8 bf16 per head row; thread t takes the vectors t, t + 256, t + 512, t + 768 of both rows
// -- eight 16-byte loads, all issued before the first use -- and the ids 8192 and 8193 go element by element to lanes 0 and 1 of the last wave.
// The pad columns 8194 .. 8207 are never loaded.  A thread keeps its 32 (33) logits in registers as the order-preserving integer image of the
// fp32 value (-0 folded into +0); with ~id as the low word that is the u64 key of t3_guard.hip: a u64 max is the largest logit with the lowest id
// among equals.  The low word is a function of the thread and the register index, so only the high words are held.
//
// Passes.  (1) thread best -> wave_max_key butterfly (DPP / permlane, no LDS) -> 4 LDS keys -> every thread folds them: M = max_v x_v and the
// first of the top ids.  (2) Z = sum_v t3_expf(x_v - M) in fp32 in ONE fixed order -- a thread adds its terms in register order (vector t,
// t + 256, ..., elements 0 .. 7 of each, then the tail id), wave_bfly_add_f32 (xor 32, 16, 8, 4, 2, 1), then the four waves in ascending order --
// and rank = #{v : x_v >= x_tok} as an integer sum beside it: one barrier for both.  lp_v = (x_v - M) - logf(Z).  (3) k rounds of workgroup
// arg-max on the exact keys, never on lp (logits that went through bf16 tie in droves): the thread that owns the winner stores (id, lp), clears
// that register and rescans its own 33; the key words alternate between two LDS sets, so a round is one barrier.  k <= 20 rounds of ~0.3 us sit
// behind the sampler of marked steps only.  No matrix in here: no MFMA.
//
// Record: slot `slot`, step `step`, 2 (K + 1) 32-bit words {rank, lp_tok, (id, lp) x k}, K = the reserved maximum; words beyond k stay untouched.
// Plain vector stores, no atomics, nothing depends on the batch: a request's records are bit-identical between eager steps, graphs, bursts and
// batch compositions.  A row holding NaN, or all -inf, is outside the numeric contract; it still runs the same fixed number of rounds and writes
// the same words.
#include "t3_kernels.h"
#include "t3_device.h"
#include "t3_attention_common.h"

#include <math.h>

namespace t3 {

constexpr int LPT = 256, LPW = LPT / 64;                 // threads, waves
constexpr int LP_KF = (V / 8) / LPT;                     // full vectors per thread and row: 4
constexpr int LP_TAIL0 = LP_KF * LPT * 8;                // first id that goes element by element: 8192
constexpr int LP_N = LP_KF * 8 + 1;                      // registers per thread: 32 + the tail id
static_assert(LP_TAIL0 <= V && V - LP_TAIL0 <= 64 && VPAD >= LP_TAIL0, "log-probability vector layout");

__device__ __forceinline__ uint32_t lp_mono(float x) {   // order-preserving image of a float; every non-NaN value maps above 0
    const uint32_t b = __float_as_uint(x + 0.0f);        // -0 -> +0: the key order equals '>' on floats
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float lp_unmono(uint32_t b) { return __uint_as_float((b & 0x80000000u) ? (b & 0x7fffffffu) : ~b); }

__global__ __launch_bounds__(LPT) void logprobs_kernel(LogprobArgs a) {
    __shared__ uint2 s_key[2][LPW];
    __shared__ float s_z[LPW];
    __shared__ int s_c[LPW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, u = blockIdx.x;
    const int slot = a.sel[u].x, step = a.sel[u].y;
    int k = a.lp_k[slot];
    if (k < 0 || step < 0 || step >= a.rec_steps) return;      // not marked / no record for this step: uniform, in front of every barrier
    k = k > a.K ? a.K : k;
    const uint16_t* lc = a.logits + (size_t)(2 * u) * a.ldl;
    const uint16_t* lu = lc + a.ldl;

    uint4 c4[LP_KF], u4[LP_KF];
#pragma unroll
    for (int q = 0; q < LP_KF; ++q) {
        c4[q] = reinterpret_cast<const uint4*>(lc)[tid + LPT * q];
        u4[q] = reinterpret_cast<const uint4*>(lu)[tid + LPT * q];
    }
    const bool tail = wave == LPW - 1 && lane < V - LP_TAIL0;
    uint16_t tc = 0, tu = 0;
    if (tail) { tc = lc[LP_TAIL0 + lane]; tu = lu[LP_TAIL0 + lane]; }
    int tok = a.out_tok[u];
    tok = tok < 0 ? 0 : (tok >= V ? V - 1 : tok);
    const float x_tok = cfg_logit(lc[tok], lu[tok], a.cfg) + 0.0f;

    // id of register i of this thread
    auto id_of = [&](int i) { return i < LP_KF * 8 ? (tid + LPT * (i >> 3)) * 8 + (i & 7) : LP_TAIL0 + lane; };
    uint32_t hi[LP_N];
#pragma unroll
    for (int q = 0; q < LP_KF; ++q) {
        const uint32_t cw[4] = {c4[q].x, c4[q].y, c4[q].z, c4[q].w}, uw[4] = {u4[q].x, u4[q].y, u4[q].z, u4[q].w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int sh = (j & 1) * 16;
            hi[q * 8 + j] = lp_mono(cfg_logit((uint16_t)(cw[j >> 1] >> sh), (uint16_t)(uw[j >> 1] >> sh), a.cfg));
        }
    }
    hi[LP_N - 1] = tail ? lp_mono(cfg_logit(tc, tu, a.cfg)) : 0u;      // 0: no entry (also what a drawn-out entry becomes); loses against every real key

    // the thread's best key: ids ascend with the register index, so among equal values the first one met has the largest ~id
    uint32_t bhi, blo;
    auto rescan = [&]() {
        bhi = 0; blo = 0;
#pragma unroll
        for (int i = 0; i < LP_N; ++i) if (hi[i] > bhi) { bhi = hi[i]; blo = ~(uint32_t)id_of(i); }
    };
    // workgroup arg-max: key words of set `par`, one barrier
    uint32_t whi, wlo;
    auto block_best = [&](int par) {
        whi = bhi; wlo = blo;
        wave_max_key(whi, wlo, lane);
        if (lane == 0) s_key[par][wave] = make_uint2(whi, wlo);
        __syncthreads();
#pragma unroll
        for (int w = 0; w < LPW; ++w) {
            const uint2 o = s_key[par][w];
            const bool take = o.x > whi || (o.x == whi && o.y > wlo);
            whi = take ? o.x : whi; wlo = take ? o.y : wlo;
        }
    };
    rescan();
    block_best(0);
    const float M = lp_unmono(whi);

    // ---- Z and the rank, one fixed order
    float z = 0.0f; int cnt = 0;
#pragma unroll
    for (int i = 0; i < LP_N; ++i) {
        if (i == LP_N - 1 && !tail) continue;
        const float x = lp_unmono(hi[i]);
        z = z + t3_expf(x - M);
        cnt += x >= x_tok ? 1 : 0;
    }
    z = wave_bfly_add_f32(z, lane);
    {
        uint32_t c = (uint32_t)cnt;
        c += lane_xor_u32<32>(c, lane); c += lane_xor_u32<16>(c, lane); c += lane_xor_u32<8>(c, lane);
        c += lane_xor_u32<4>(c, lane); c += lane_xor_u32<2>(c, lane); c += lane_xor_u32<1>(c, lane);
        cnt = (int)c;
    }
    if (lane == 0) { s_z[wave] = z; s_c[wave] = cnt; }
    __syncthreads();
    const float Z = ((s_z[0] + s_z[1]) + s_z[2]) + s_z[3];
    const float logZ = logf(Z);
    int* rec = a.rec + ((size_t)slot * a.rec_steps + step) * (size_t)(2 * (a.K + 1));
    if (tid == 0) {
        rec[0] = (s_c[0] + s_c[1]) + (s_c[2] + s_c[3]);
        rec[1] = __float_as_int((x_tok - M) - logZ);
    }

    // ---- the k most likely ids: (x descending, id ascending), on the exact logits
    for (int r = 0; r < k; ++r) {
        if (r > 0) block_best(r & 1);
        if (bhi == whi && blo == wlo && whi != 0u) {      // this thread owns the winner
            rec[2 + 2 * r] = (int)~wlo;
            rec[3 + 2 * r] = __float_as_int((lp_unmono(whi) - M) - logZ);
#pragma unroll
            for (int i = 0; i < LP_N; ++i) if (~(uint32_t)id_of(i) == wlo) hi[i] = 0u;
            rescan();
        }
    }
}

hipError_t launch_logprobs(const LogprobArgs& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    if (!a.logits || !a.sel || !a.out_tok || !a.lp_k || !a.rec || a.ldl < V || (a.ldl & 7) /* 16-byte row loads */ || a.K < 0 || a.K > T3_MAX_LOGPROBS || a.rec_steps <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(logprobs_kernel, dim3(a.n), dim3(LPT), 0, s, a);
    return hipGetLastError();
}

// lp_k[slot] = k by a kernel: admission and finish are stream-ordered against captured steps
__global__ __launch_bounds__(64) void logprobs_mark_kernel(int* lp_k, int slot, int k) {
    if (threadIdx.x == 0) lp_k[slot] = k;
}
hipError_t launch_logprobs_mark(int* lp_k, int slot, int k, hipStream_t s) {
    hipLaunchKernelGGL(logprobs_mark_kernel, dim3(1), dim3(64), 0, s, lp_k, slot, k);
    return hipGetLastError();
}

}  // namespace t3
