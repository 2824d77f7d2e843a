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
//
// PROCESSED (logprobs_kernel<true>, t3_set_logprobs_mode(h, 1)): the same passes over z_v, the value the sampler draws from -- the post-CFG logit behind
// the slot's logit processors, the guard's suppression, the penalties and the temperature (include/t3_engine.h, "processed log-probabilities").  What
// differs is only how a register gets its value:
//   * beside its eight head-row loads a thread loads the four 16-byte vectors of the slot's counts that cover the same ids (a slot's count row is
//     VPAD * 2 = 16 416 bytes, a multiple of 16), the 32-bit allow word that holds the byte of each of its vectors, the record's header and the
//     guard's control word: nothing depends on another load;
//   * the 64 sorted (id, bias) pairs are loaded by the first wave beside all that and shared through LDS (ids, 8 sentinels, biases: 544 bytes) behind
//     ONE workgroup barrier, which only a marked slot with a bias list reaches.  (The raw kernel's first barrier stands behind the thread's best key,
//     which already needs the biases, so it cannot carry the table.)  A thread's ids are four runs of eight: one branch-free lower bound per run, as
//     in the sampler;
//   * the sampler has counted the id it drew by the time this kernel runs (finish() in sampler_kernel), so the drawn id's count is taken back by one --
//     a stored 65535 is read as saturated before the draw;
//   * z_tok is formed by every thread from scalar loads of the drawn id's own words: no broadcast, no barrier.
// The penalty arithmetic restates sampler_kernel's `element` operation by operation (the file is compiled with the same flags); the raw instantiation
// compiles to the instructions it had before the template existed (profiles/NOTES.md).
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

// PROCESSED: penalties and temperature on a logit the processors and the guard have been through -- sampler_kernel's `element`, restated
__device__ __forceinline__ float lp_penalise(float x, uint32_t cnt, const T3Sampling& sp, float T) {
    if (cnt > 0) {
        if (sp.repetition_penalty != 1.0f) x = (x > 0.0f) ? x / sp.repetition_penalty : x * sp.repetition_penalty;
        x = x - sp.frequency_penalty * (float)cnt;
        x = x - sp.presence_penalty;
    }
    return x / T;
}
constexpr int LP_TAB = PROC_MAX_BIAS + 8 + PROC_MAX_BIAS;      // [64] ids, [8] sentinels, [64] biases
static_assert((VPAD * 2) % 16 == 0, "a slot's count row starts on a 16-byte boundary");

template <bool PROCESSED>
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

    // PROCESSED: the slot's sampling parameters, its counts, its processor record (nullable, as SampleArgs.proc) and the guard's control word
    [[maybe_unused]] T3Sampling sp = {};
    [[maybe_unused]] const uint16_t* counts = nullptr;
    [[maybe_unused]] const uint32_t* prec = nullptr;
    [[maybe_unused]] uint4 n4[LP_KF] = {}, ph0 = make_uint4(0, 0, 0, 0), ph1 = ph0;
    [[maybe_unused]] uint32_t aw[LP_KF] = {}, awt = 0, tab_id = 0x7fffffffu, tab_val = 0;
    [[maybe_unused]] int ctl = GUARD_NONE;
    if constexpr (PROCESSED) {
        sp = a.sp[slot];
        counts = a.counts + (size_t)slot * VPAD;
        if (sp.alignment == 2 && a.eos_ctl) ctl = a.eos_ctl[slot];      // the sampler's condition
        if (a.proc) {
            prec = a.proc + (size_t)slot * PROC_WORDS;
            ph0 = reinterpret_cast<const uint4*>(prec + PROC_HDR)[0]; ph1 = reinterpret_cast<const uint4*>(prec + PROC_HDR)[1];
            if (tid < PROC_MAX_BIAS) { tab_id = prec[PROC_IDS + tid]; tab_val = prec[PROC_VALS + tid]; }
        }
    }
    uint4 c4[LP_KF], u4[LP_KF];
#pragma unroll
    for (int q = 0; q < LP_KF; ++q) {
        c4[q] = reinterpret_cast<const uint4*>(lc)[tid + LPT * q];
        u4[q] = reinterpret_cast<const uint4*>(lu)[tid + LPT * q];
        if constexpr (PROCESSED) {
            n4[q] = reinterpret_cast<const uint4*>(counts)[tid + LPT * q];
            if (prec) aw[q] = prec[(tid + LPT * q) >> 2];      // ids 8 vi .. 8 vi + 7: byte vi & 3 of it
        }
    }
    const bool tail = wave == LPW - 1 && lane < V - LP_TAIL0;
    uint16_t tc = 0, tu = 0;
    [[maybe_unused]] uint16_t tn = 0;
    if (tail) {
        tc = lc[LP_TAIL0 + lane]; tu = lu[LP_TAIL0 + lane];
        if constexpr (PROCESSED) { tn = counts[LP_TAIL0 + lane]; if (prec) awt = prec[(LP_TAIL0 + lane) >> 5]; }
    }
    int tok = a.out_tok[u];
    tok = tok < 0 ? 0 : (tok >= V ? V - 1 : tok);
    float x_tok;

    // id of register i of this thread
    auto id_of = [&](int i) { return i < LP_KF * 8 ? (tid + LPT * (i >> 3)) * 8 + (i & 7) : LP_TAIL0 + lane; };
    uint32_t hi[LP_N];
    if constexpr (PROCESSED) {
        __shared__ uint32_t s_tab[LP_TAB];
        const uint32_t tok_cnt = counts[tok], tok_aw = prec ? prec[tok >> 5] : ~0u;
        const float tok_x = cfg_logit(lc[tok], lu[tok], a.cfg);
        const bool marked = prec && ph0.x != 0u, biased = marked && ph0.w != 0u;
        if (biased) {                                        // uniform: the one barrier the bias table costs
            if (tid < PROC_MAX_BIAS) { s_tab[tid] = tab_id; s_tab[PROC_MAX_BIAS + 8 + tid] = tab_val; }
            if (tid < 8) s_tab[PROC_MAX_BIAS + tid] = 0x7fffffffu;
            __syncthreads();
        }
        const float* tabf = reinterpret_cast<const float*>(s_tab + PROC_MAX_BIAS + 8);
        auto lower_bound = [&](int key) -> int {             // pairs with an id below key, capped at 63: enough, since only an EQUAL id is ever used
            int p = 0;
#pragma unroll
            for (int s = PROC_MAX_BIAS / 2; s >= 1; s >>= 1) p += ((int)s_tab[p + s - 1] < key) ? s : 0;
            return p;
        };
        const bool hold = marked && (uint32_t)step < ph0.y;  // min_tokens: token `step` may not be a stop id yet
        const int n_stop = (int)ph0.z < PROC_MAX_STOP ? (int)ph0.z : PROC_MAX_STOP;
        const int stops[PROC_MAX_STOP] = {(int)ph1.x, (int)ph1.y, (int)ph1.z, (int)ph1.w};
        const int suppress = ctl == GUARD_SUPPRESS ? sp.stop_token : -1;      // GUARD_FORCE changes no logit: the forced id reports its z
        const float T = sp.temperature < 1e-5f ? 1.0f : sp.temperature;      // greedy: vLLM's substitute
        // one id: processors (keep bit, bias), suppression, the count the sampler used, penalties, temperature
        auto z_of = [&](float x, bool keep, bool has_b, float b, uint32_t cnt, int v) -> float {
            if (!keep) x = -INFINITY; else if (has_b) x = x + b;
            if (v == suppress) x = -INFINITY;
            if (v == tok && cnt > 0u && cnt < 65535u) cnt -= 1u;      // the sampler has counted its draw already; 65535 = saturated before it
            return lp_penalise(x, cnt, sp, T);
        };
#pragma unroll
        for (int q = 0; q < LP_KF; ++q) {
            const int vi = tid + LPT * q, base = vi * 8;
            uint32_t keep8 = marked ? (aw[q] >> ((vi & 3) * 8)) & 0xffu : 0xffu, bias8 = 0;
            float pb[8] = {};
            if (hold) {
#pragma unroll
                for (int s = 0; s < PROC_MAX_STOP; ++s) { const uint32_t d = (uint32_t)(stops[s] - base); if (s < n_stop && d < 8u) keep8 &= ~(1u << d); }
            }
            if (biased) {
                int p = lower_bound(base);
                int idp = (int)s_tab[p];
                if (idp < base + 8) {                        // the run holds a biased id (or p stopped at 63 below it: nothing will match)
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (idp == base + j) { pb[j] = tabf[p]; bias8 |= 1u << j; ++p; idp = (int)s_tab[p]; }
                }
            }
            const uint32_t cw[4] = {c4[q].x, c4[q].y, c4[q].z, c4[q].w}, uw[4] = {u4[q].x, u4[q].y, u4[q].z, u4[q].w},
                           nw[4] = {n4[q].x, n4[q].y, n4[q].z, n4[q].w};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int sh = (j & 1) * 16;
                const float x = cfg_logit((uint16_t)(cw[j >> 1] >> sh), (uint16_t)(uw[j >> 1] >> sh), a.cfg);
                hi[q * 8 + j] = lp_mono(z_of(x, (keep8 >> j) & 1u, (bias8 >> j) & 1u, pb[j], (nw[j >> 1] >> sh) & 0xffffu, base + j));
            }
        }
        auto single = [&](float x, uint32_t word, uint32_t cnt, int v) -> float {      // an id on its own: the tail lanes' one, and the drawn one
            bool keep = marked ? (word >> (v & 31)) & 1u : true, has_b = false;
            float b = 0.0f;
            if (hold) {
#pragma unroll
                for (int s = 0; s < PROC_MAX_STOP; ++s) if (s < n_stop && stops[s] == v) keep = false;
            }
            if (biased) { const int p = lower_bound(v); if ((int)s_tab[p] == v) { b = tabf[p]; has_b = true; } }
            return z_of(x, keep, has_b, b, cnt, v);
        };
        hi[LP_N - 1] = tail ? lp_mono(single(cfg_logit(tc, tu, a.cfg), awt, tn, LP_TAIL0 + lane)) : 0u;
        x_tok = single(tok_x, tok_aw, tok_cnt, tok) + 0.0f;
    } else {
        x_tok = cfg_logit(lc[tok], lu[tok], a.cfg) + 0.0f;
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
    }

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
    if (a.mode != 0 && (a.mode != 1 || !a.counts || !a.sp || ((uintptr_t)a.counts & 15) /* 16-byte count loads */)) return hipErrorInvalidValue;
    if (a.mode == 1) hipLaunchKernelGGL(logprobs_kernel<true>, dim3(a.n), dim3(LPT), 0, s, a);
    else hipLaunchKernelGGL(logprobs_kernel<false>, dim3(a.n), dim3(LPT), 0, s, a);
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
