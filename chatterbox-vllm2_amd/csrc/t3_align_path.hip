// Token time spans for gfx950 (MI355X, CDNA4): the monotonic path through a finished request's alignment matrix A[frame][text id]
// (t3_alignment.hip), and from it the [start, end) frames every text id is spoken in.  wave = 64 lanes.  Compile with -ffp-contract=off.
//
// What it is for: subtitle, karaoke and lip-sync timestamps.  The search is Glow-TTS's monotonic alignment search with a free end (DESIGN.md
// section 8 states the contract): cell scores w = round(1024 log2 a) as int32, then pure integer arithmetic
//
//     D[0][0] = w[0][0],   D[k][t] = w[k][t] + max(D[k-1][t], D[k-1][t-1])  for t <= k  (step from t - 1 only when STRICTLY larger),   NEG above the diagonal
//
// last = the lowest t with the largest D[n-1][t], backtrack to (0, 0).  Integer sums make the path exact and independent of any order.
//
// Split: the problem is a latency chain along the frames (up to 1000 dependent rows) with parallelism only across the text ids, so ONE WAVE
// serves one request and the grid is the number of requests of the call.  No LDS, no barrier, and no MFMA: there is no matrix product here.
//   * Lane l, slot j owns text id 64 j + l: a row of A is C = ceil(S / 64) coalesced 256-byte loads at the request's pitch.  D of the previous
//     row lives in registers, C words per lane; the kernel is instantiated for C = 2, 4, 8, 16 and 33 (128 .. 1024 and 2112 ids; the engine stops
//     at 2050) and a launch takes the smallest that holds its widest request.  A slot beyond a request's own text costs its instructions and no
//     more: its lanes re-read the row's last column and its cells stay at NEG (a test per slot would be a scalar mask per slot held across the loop).
//   * The left neighbour D[k-1][t-1] is one DPP rotate of the wave by a lane (wave_ror:1) per slot; lane 0 takes lane 63's value of slot j - 1,
//     which the previous slot's rotate has already brought to it, and NEG for slot 0.
//   * Row loads do not depend on the DP: a ring of R row registers (R = 8, 8, 4, 4, 2) keeps R - 1 rows in flight ahead of the row
//     being folded.  They are ordinary loads, so the compiler places the waits.  Only rotate / compare / select / add is serial; the polynomial
//     of the score is not.
//   * Back-pointers are one bit per cell: per row and slot the 64-bit ballot of "came from t - 1".  Lane (j + k) & 63 keeps slot j's ballot of row k,
//     and those lanes write the row's words with one plain vector store into the workspace [n][ceil(S / 64)] (at most 2.1 MiB, L2-resident).
//   * End cell: wave max over the u64 key (D biased to unsigned) << 32 | ~t, as t3_guard.hip's argmax.
//   * Backtrack in chunks of 64 frames from the top.  Lane i loads the words of frame k0 + i for t's column block and the one below it (within
//     64 frames t leaves its block at most once); 64 register-only steps read frame k's word with a constant lane index and collect the
//     steps down as a 64-bit mask, from which lane k & 63 counts its path[k]; a chunk ends in one coalesced store.  t is clamped at 0, so a path index can never leave [0, last].
//   * A last pass over path, every lane taking the frames lane, lane + 64, ..., writes start[t] where the path enters t and end[t] where it
//     leaves.  start / end were filled with -1 first.  Words another lane wrote are read behind a fence.
#include "t3_kernels.h"
#include "t3_device.h"
#include "t3_attention_common.h"

#include <algorithm>

namespace t3 {

constexpr int PATH_NEG = -(1 << 30);

// Cell score: a clamped into [2^-64, 2^64] (NaN, zero and negatives to 2^-64), exponent + degree-5 polynomial for
// log2(1 + f) / f fitted at the Chebyshev nodes of [0, 1] (max error 7.5e-6), every operation rounded on its own, rint to 1/1024 octave.
__device__ __forceinline__ int align_score(float a) {
    const float lo = 5.42101086242752217003726400434970855712890625e-20f, hi = 18446744073709551616.0f;      // 2^-64, 2^64
    a = a > lo ? a : lo;
    a = a < hi ? a : hi;
    const uint32_t u = __float_as_uint(a);
    const int e = (int)(u >> 23) - 127;
    const float f = __uint_as_float((u & 0x7fffffu) | 0x3f800000u) - 1.0f;
    float p = -0.03382204473018646f;
    p = 0.14447109401226044f + f * p;
    p = -0.30163800716400146f + f * p;
    p = 0.4686588644981384f + f * p;
    p = -0.7203587889671326f + f * p;
    p = 1.4426814317703247f + f * p;
    p = f * p;
    return (int)__builtin_rintf(((float)e + p) * 1024.0f);
}

// v of lane (l - 1) & 63
__device__ __forceinline__ int wave_ror1(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x13C, 0xf, 0xf, false); }      // wave_ror:1

// A row's slots.  A lane beyond the text reads the row's last column instead of being masked off (its value never enters a result: the fold
// keeps such a cell at NEG), so a row costs no lane mask per slot.
// The items' pointers are loaded from memory, where the compiler cannot see that they are global: said here, the accesses become global_load / global_store
// with a scalar base and a 32-bit lane offset instead of flat ones with a 64-bit address per slot.
#define T3_GLOBAL __attribute__((address_space(1)))
typedef const float T3_GLOBAL* gfloat_cp;
typedef int T3_GLOBAL* gint_p;
typedef unsigned long long T3_GLOBAL* gu64_p;

template <int C>
__device__ __forceinline__ void load_row(float (&row)[C], gfloat_cp p /* the row */, int lane, int S) {
#pragma unroll
    for (int j = 0; j < C; ++j) row[j] = p[(unsigned)min(64 * j + lane, S - 1)];
}

template <int C, int R>
__global__ __launch_bounds__(64) void align_path_kernel(const AlignPathItem* items, int span_ld) {
    const AlignPathItem it = items[blockIdx.x];
    const int lane = threadIdx.x;
    const int n = it.n_frames, S = it.n_text;
    const gfloat_cp A = (gfloat_cp)it.A;
    const gu64_p bp = (gu64_p)it.bp;
    const gint_p path = (gint_p)it.path, start = (gint_p)it.start, end = (gint_p)it.end, res = (gint_p)it.res;
    const int ns = __builtin_amdgcn_readfirstlane((S + 63) >> 6);      // the request's own slots, <= C (the launcher's choice)
    for (int t = lane; t < span_ld; t += 64) { start[t] = -1; end[t] = -1; }
    if (n <= 0 || S <= 0 || ns > C) { if (lane == 0) { res[0] = -1; res[1] = 0; } return; }

    // ---- forward: D of the previous row in prev[], rows of A through the ring
    int prev[C];
    float ring[R][C];
#pragma unroll
    for (int j = 0; j < C; ++j) prev[j] = PATH_NEG;
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int j = 0; j < C; ++j) ring[r][j] = 0.0f;
        if (r < n) load_row<C>(ring[r], A + (size_t)r * it.ld, lane, S);
    }
    for (int k0 = 0; k0 < n; k0 += R) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int k = k0 + r;
            if (k < n) {
                int carry = k == 0 ? 0 : PATH_NEG;      // what lane 0 of slot 0 sees to its left: D[0][0] = w[0][0] + 0
                const int lim = min(k, S - 1);          // cells beyond it are above the diagonal or beyond the text
                // slot j's ballot is kept by lane (j + k) & 63: the lane that keeps a word moves with the row, so "is it mine" is one compare per
                // slot against a per-row value and not a lane mask per slot held in scalar registers across the whole loop
                const int mine = (lane - k) & 63;
                unsigned long long word = 0;
#pragma unroll
                for (int j = 0; j < C; ++j) {
                    const int t = 64 * j + lane;
                    const int w = align_score(ring[r][j]);
                    const int rot = wave_ror1(prev[j]);
                    const int left = lane == 0 ? carry : rot;
                    carry = rot;                        // lane 0: lane 63's D of this slot, the next slot's left neighbour
                    const bool from = left > prev[j];
                    const int m = from ? left : prev[j];
                    prev[j] = t <= lim ? w + m : PATH_NEG;      // unreachable: nothing is added
                    const unsigned long long b = __ballot(from);
                    if (mine == j) word = b;
                    // a slot is finished here, before the next one starts: the wave's slots are independent, and a compiler that runs all the rotates and
                    // compares of a row first holds a scalar pair and a register per slot meanwhile.  One wave issues in order, so that buys nothing.
                    asm volatile("" : "+v"(prev[j]), "+v"(word));
                }
                if (mine < ns) bp[(size_t)k * ns + mine] = word;
                if (k + R < n) load_row<C>(ring[r], A + (size_t)(k + R) * it.ld, lane, S);
            }
        }
    }

    // ---- end cell: the lowest t with the largest D[n-1][t]
    uint32_t khi = 0, klo = 0;
#pragma unroll
    for (int j = 0; j < C; ++j) {
        const int t = 64 * j + lane;
        const uint32_t hi = (uint32_t)prev[j] + 0x80000000u, lo = ~(uint32_t)t;
        if (t < S && (hi > khi || (hi == khi && lo > klo))) { khi = hi; klo = lo; }
    }
    wave_max_key(khi, klo, lane);
    const int last = __builtin_amdgcn_readfirstlane((int)~klo), score = __builtin_amdgcn_readfirstlane((int)(khi - 0x80000000u));
    __threadfence();                                // the back-pointer words were written by other lanes

    // ---- backtrack, 64 frames per chunk
    int t = last;
    for (int k0 = ((n - 1) >> 6) << 6; k0 >= 0; k0 -= 64) {
        const int b = t >> 6, k = k0 + lane;
        unsigned long long whi = 0, wlo = 0;
        if (k < n) {
            whi = bp[(size_t)k * ns + b];
            if (b > 0) wlo = bp[(size_t)k * ns + b - 1];
        }
        const int t0 = t;
        unsigned long long dec = 0;                 // bit kk: the path steps down between frames k0 + kk and k0 + kk - 1
#pragma unroll
        for (int kk = 63; kk >= 0; --kk) {
            if (k0 + kk >= n) continue;             // the top chunk's frames beyond the matrix (uniform)
            const unsigned long long wsel = (t >> 6) == b ? whi : wlo;      // t is wave-uniform: every lane shifts its own frame's word, lane kk's counts
            const int bit = __builtin_amdgcn_readlane((int)((uint32_t)(wsel >> (t & 63)) & 1u), kk);
            const int d = (k0 + kk > 0 && t > 0) ? bit : 0;
            t -= d;
            dec |= (unsigned long long)d << kk;
        }
        const int p = t0 - __popcll((dec >> lane) >> 1);      // path[k0 + lane]: the chunk's entry id less the steps taken above this frame
        if (k < n) path[k] = p;
    }
    __threadfence();                                // path was written by other lanes

    // ---- spans: the path enters t at start[t] and leaves it at end[t]
    for (int k = lane; k < n; k += 64) {
        const int tk = path[k];
        if (k == 0 || path[k - 1] != tk) start[tk] = k;
        if (k == n - 1 || path[k + 1] != tk) end[tk] = k + 1;
    }
    if (lane == 0) { res[0] = last; res[1] = score; }
}

hipError_t launch_align_path(const AlignPathItem* items, int n, int max_text, int span_ld, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (!items || max_text < 0 || max_text > ALIGN_PATH_MAX_TEXT || span_ld < max_text || span_ld <= 0) return hipErrorInvalidValue;
    if (max_text <= 128) launch_k(align_path_kernel<2, 8>, dim3(n), dim3(64), 0, s, items, span_ld);
    else if (max_text <= 256) launch_k(align_path_kernel<4, 8>, dim3(n), dim3(64), 0, s, items, span_ld);
    else if (max_text <= 512) launch_k(align_path_kernel<8, 4>, dim3(n), dim3(64), 0, s, items, span_ld);
    else if (max_text <= 1024) launch_k(align_path_kernel<16, 4>, dim3(n), dim3(64), 0, s, items, span_ld);
    else launch_k(align_path_kernel<33, 2>, dim3(n), dim3(64), 0, s, items, span_ld);
    return hipGetLastError();
}

// The cell score alone (the format pin of the parity tests)
__global__ __launch_bounds__(256) void align_scores_kernel(const float* a, int* w, int n) {
    for (int i = (int)blockIdx.x * 256 + threadIdx.x; i < n; i += (int)gridDim.x * 256) w[i] = align_score(a[i]);
}
hipError_t launch_align_scores(const float* a, int* w, int n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(align_scores_kernel, dim3(std::min((n + 255) / 256, 1024)), dim3(256), 0, s, a, w, n);
    return hipGetLastError();
}

}  // namespace t3
