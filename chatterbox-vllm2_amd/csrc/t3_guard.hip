// Alignment guard for gfx950 (MI355X, CDNA4): the consumer of the alignment frames INSIDE the step.  wave = 64 lanes.  Compile with
// -ffp-contract=off.
//
// What it is for: upstream Chatterbox's AlignmentStreamAnalyzer rewrites the logits of every frame from the attention three Llama heads pay
// to the text -- it holds the stop id back until the text is spoken and forces it once the model lingers on, or goes back over, text it has
// already spoken.  The engine replays several decode steps per graph with no host in between, so the analyzer's state machine runs here, on the
// frame the step's last tap (t3_alignment.hip) has just completed, and leaves ONE control word per slot that the step's sampler obeys
// (sampler_kernel, guarded instantiation).  include/t3_engine.h ("alignment guard") spells the rules out; DESIGN.md repeats them.  The parameter
// defaults (T3GuardParams) follow upstream's analyzer as its rules are known to the maintainers and have NOT been validated against a real
// checkpoint on this project: that is why they are parameters.
//
// Split: one wave per sampled utterance, four waves per workgroup, grid = ceil(n_sel / 4) -- a function of the step's shape only, so a captured
// step stays valid whatever the slots hold.  A wave whose slot is not guarded (sp.alignment != 2) or whose row is not tapped this step leaves
// at once.  Launched once per step behind the last tap and in front of the sampler; a row is at most a few KiB and the work a few hundred
// instructions, so the launch is latency, not bandwidth.
//
// Row pass: the frame a_k[0 .. S) (S = n_text; rows are ld-pitched and 16-byte aligned) is read ONCE, one 16-byte load per lane and pass, 256
// floats per pass.  A lane keeps three things: the u64 key (value bits << 32 | ~index) of its best column -- probabilities are >= 0, so their
// bit patterns order like the values, and the lowest index among equal values has the largest key: the argmax with numpy's tie rule is one
// u64 max --, the largest value among the columns [0, S - skip), and the three tail columns S - 3 .. S - 1 (each column is met by exactly one
// lane of one pass; the other lanes hold 0, so a max brings it to all).  Columns >= S (the pitch's padding, and whatever a longer text left
// there) are loaded with their vector but never selected into any of the three.  The wave reductions are the DPP / permlane butterflies of
// t3_attention_common.h: no LDS, no atomics.  Every lane ends up with the same values and computes the same state; lane 0 stores it.
//
// State: GUARD_STATE_WORDS = 8 words per slot (t3_kernels.h), read as two 16-byte loads of one address by every lane and written back by lane
// 0 with two 16-byte vector stores; the control word goes to ctl[slot].  All zero is the state of a freshly admitted slot (forced_at is kept
// as forced_at + 1), so admission clears it with guard_reset_kernel -- a kernel, not a memset node: admission work is stream-ordered against
// captured steps.  The two running sums take ONE fp32 add per step, in step order: the state is bit-identical between eager steps, graphs and
// bursts, and a numpy restatement with float32 adds reproduces it exactly.
//
// Token repetition reads the sampler's own history (SampleArgs.hist) at frames k - 1 .. k - tok_rep: lane i compares frame k - 1 - i with frame
// k - 1, one ballot.  The same word tells a step that runs BEHIND the utterance's stop id (run-ahead and bursts schedule up to seven of them
// before the host has seen the id): such a step changes nothing and is forced, so the state a finished request reports is the state after
// its last token, wherever the stop id came from.
#include "t3_kernels.h"
#include "t3_device.h"
#include "t3_attention_common.h"

#include <string.h>

namespace t3 {

__global__ __launch_bounds__(256) void guard_kernel(GuardArgs a) {
    const int lane = threadIdx.x & 63;
    const int u = (int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    if (u >= a.n_sel) return;
    const int slot = a.sel[u].x, k = a.sel[u].y;
    if (a.sp[slot].alignment != 2) return;                      // not guarded: its sampler never looks at ctl[slot]
    const int* rec = a.rowrec + (size_t)(a.sel_rows ? a.sel_rows[2 * u] : u) * a.row_stride;
    const int frame = rec[ROW_ALIGN_FRAME], S = rec[ROW_ALIGN_NTEXT];
    if (frame < 0) return;                                      // not tapped this step
    int* stw = a.state + (size_t)slot * GUARD_STATE_WORDS;
    const int4 s0 = reinterpret_cast<const int4*>(stw)[0];
    const float4 s1 = reinterpret_cast<const float4*>(stw)[1];
    int pos = s0.x, complete = s0.y & 1, completed_at = s0.z;
    // frozen: forced earlier, or this step runs behind the step that drew the utterance's stop id
    const int* hist = a.hist + (size_t)slot * a.hist_cap;
    const int last = (k >= 1 && k - 1 < a.hist_cap) ? hist[k - 1] : -1;
    if (s0.w != 0 || (k >= 1 && last == a.sp[slot].stop_token)) { if (lane == 0) a.ctl[slot] = GUARD_FORCE; return; }
    if (S <= 0 || S > a.ld) { if (lane == 0) a.ctl[slot] = GUARD_NONE; return; }      // no text: nothing to follow

    // ---- one pass over the frame
    const float4* row = reinterpret_cast<const float4*>(a.frames + ((size_t)slot * a.frames_per_slot + frame) * a.ld);
    const int n_rep = S - a.p.skip;                             // repetition looks at the columns [0, n_rep)
    uint32_t khi = 0, klo = 0;                                  // best (value bits, ~index) of the lane; (0, 0) loses against every real column
    float rmax = 0.0f, tl[3] = {0.0f, 0.0f, 0.0f};
    for (int base = 0; base < S; base += 256) {
        const int c0 = base + 4 * lane;
        if (c0 >= S) continue;                                  // the vector [c0, c0 + 4) lies inside the row's pitch: ld is S rounded up to 4, or more
        const float4 v4 = row[c0 >> 2];
        const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = c0 + j;
            if (t >= S) continue;                               // padding of the pitch: never into a result
            const uint32_t b = __float_as_uint(v[j]), ni = ~(uint32_t)t;
            if (b > khi || (b == khi && ni > klo)) { khi = b; klo = ni; }
            if (t < n_rep) rmax = fmaxf(rmax, v[j]);
#pragma unroll
            for (int i = 0; i < 3; ++i) if (t == S - 3 + i) tl[i] = v[j];
        }
    }
    wave_max_key(khi, klo, lane);
    rmax = wave_max_f32(rmax, lane);
#pragma unroll
    for (int i = 0; i < 3; ++i) tl[i] = wave_max_f32(tl[i], lane);

    // ---- the state machine (the same in every lane)
    const int c = (int)~klo;
    const int d = c - pos;
    if (d > -a.p.back && d < a.p.fwd) pos = c;
    if (!complete && pos >= S - a.p.end) { complete = 1; completed_at = k; }
    float tail[3] = {s1.x, s1.y, s1.z}, rep = s1.w;
    if (complete) {
#pragma unroll
        for (int i = 0; i < 3; ++i) if (S - 3 + i >= 0) tail[i] = tail[i] + tl[i];
        rep = rep + rmax;
    }
    const bool long_tail = complete && fmaxf(fmaxf(tail[0], tail[1]), tail[2]) >= a.p.tail_thr;
    const bool align_rep = complete && rep > a.p.rep_thr;
    bool tok_hit = false;
    if (a.p.tok_rep > 0 && k >= a.p.tok_rep && k - 1 < a.hist_cap) {
        const bool same = lane >= a.p.tok_rep || hist[k - 1 - lane] == last;
        tok_hit = __ballot(same) == ~0ull;
    }
    const int reason = tok_hit ? 1 : long_tail ? 2 : align_rep ? 3 : 0;
    const int ctl = reason ? GUARD_FORCE : (pos < S - a.p.end && S > a.p.skip) ? GUARD_SUPPRESS : GUARD_NONE;
    if (lane == 0) {
        reinterpret_cast<int4*>(stw)[0] = make_int4(pos, complete | (reason << 8), completed_at, reason ? k + 1 : 0);
        reinterpret_cast<float4*>(stw)[1] = make_float4(tail[0], tail[1], tail[2], rep);
        a.ctl[slot] = ctl;
    }
}

hipError_t launch_guard(const GuardArgs& a, hipStream_t s) {
    if (a.n_sel <= 0) return hipSuccess;
    if (a.ld <= 0 || (a.ld & 3) || !a.frames || !a.state || !a.ctl || !a.hist) return hipErrorInvalidValue;
    launch_k(guard_kernel, dim3((a.n_sel + 3) / 4), dim3(256), 0, s, a);
    return hipGetLastError();
}

// A slot's state and control word start at zero
__global__ __launch_bounds__(64) void guard_reset_kernel(int* state, int* ctl, int slot) {
    const int lane = threadIdx.x;
    if (lane < GUARD_STATE_WORDS) state[(size_t)slot * GUARD_STATE_WORDS + lane] = 0;
    else if (lane == GUARD_STATE_WORDS) ctl[slot] = GUARD_NONE;
}
hipError_t launch_guard_reset(int* state, int* ctl, int slot, hipStream_t s) {
    hipLaunchKernelGGL(guard_reset_kernel, dim3(1), dim3(64), 0, s, state, ctl, slot);
    return hipGetLastError();
}

void guard_unpack_state(const int* w, T3GuardState* out) {
    out->pos = w[0]; out->complete = w[1] & 1; out->reason = w[1] >> 8; out->completed_at = w[2]; out->forced_at = w[3] - 1;
    memcpy(out->tail, w + 4, 12); memcpy(&out->rep, w + 7, 4);
}

}  // namespace t3
