// Logit processors for gfx950 (MI355X, CDNA4): the build and reset kernels of a slot's processor record, and the host's check and staging of a
// request's lists.  The record is consumed by sampler_kernel<true, true> (t3_kernels.hip); its layout and the staging image's stand in t3_kernels.h,
// the contract in include/t3_engine.h ("logit processors").  wave = 64 lanes.
//
// Why a kernel builds the record: the sampler wants the allow list as a bitmask (one word covers a thread's eight ids) and the bias list sorted by id
// (a thread's ids are a run, so ONE lower bound finds all of its biases); the caller hands over unsorted lists.  Building on the device keeps the
// admission path free of a second host pass over up to 8194 ids and puts the record's writes on the slot's group stream, behind the previous
// occupant's last step, where guard_reset_kernel and the log-probability mark already are.
//
// Split: ONE workgroup of 256 threads.  (1) the mask starts in LDS as all ones (no list) or zero; the listed ids set their bits by LDS atomics, 256
// ids per pass, in any order and with duplicates; (2) meanwhile the 64 (id, bias) pairs -- padded with (INT32_MAX, 0) -- sit in LDS as 64-bit keys
// id << 32 | bias bits and the first wave sorts them with a bitonic network: 21 compare-exchange rounds, one key per lane, the partner read from LDS;
// ids are distinct, so the order of the keys is the order of the ids; (3) the record leaves LDS by plain 16-byte stores, the flag word last in
// program order (nothing reads the record before the kernel has ended: the sampler follows on the same stream).  Nothing is rejected here -- the
// host has checked the lists -- but every index is clamped, so a torn staging image cannot address outside LDS or the record.
#include "t3_kernels.h"

#include <math.h>
#include <string.h>

namespace t3 {

constexpr int LB_T = 256;
__device__ __forceinline__ uint32_t proc_full_word(int w) {      // the allow word of "every id": bits from V on are clear
    return w < (V >> 5) ? ~0u : w == (V >> 5) ? (1u << (V & 31)) - 1u : 0u;
}

__global__ __launch_bounds__(LB_T) void logitproc_build_kernel(const int32_t* __restrict__ st, uint32_t* __restrict__ rec) {
    __shared__ __attribute__((aligned(16))) uint32_t s_mask[PROC_ALLOW_WORDS];
    __shared__ __attribute__((aligned(16))) unsigned long long s_key[PROC_MAX_BIAS];
    const int tid = threadIdx.x;
    const int4 h0 = reinterpret_cast<const int4*>(st)[0], h1 = reinterpret_cast<const int4*>(st)[1];
    const bool all = h0.x < 0;
    const int n_allowed = h0.x > V ? V : h0.x;
    const int n_bias = h0.y < 0 ? 0 : (h0.y > PROC_MAX_BIAS ? PROC_MAX_BIAS : h0.y);
    const int n_stop = h0.w < 0 ? 0 : (h0.w > PROC_MAX_STOP ? PROC_MAX_STOP : h0.w);
    for (int w = tid; w < PROC_ALLOW_WORDS; w += LB_T) s_mask[w] = all ? proc_full_word(w) : 0u;
    if (tid < PROC_MAX_BIAS) {
        const uint32_t id = tid < n_bias ? (uint32_t)st[PROC_STAGE_IDS + tid] : 0x7fffffffu;
        const uint32_t bits = tid < n_bias ? (uint32_t)st[PROC_STAGE_VALS + tid] : 0u;
        s_key[tid] = ((unsigned long long)id << 32) | bits;
    }
    __syncthreads();
    for (int i = tid; i < n_allowed; i += LB_T) {
        const int id = st[PROC_STAGE_ALLOW + i];
        if ((unsigned)id < (unsigned)V) atomicOr(&s_mask[id >> 5], 1u << (id & 31));
    }
    // bitonic network over the 64 keys, ascending: the loops are uniform, every thread reaches every barrier
    for (int k = 2; k <= PROC_MAX_BIAS; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            unsigned long long mine = 0, other = 0;
            if (tid < PROC_MAX_BIAS) { mine = s_key[tid]; other = s_key[tid ^ j]; }
            __syncthreads();
            if (tid < PROC_MAX_BIAS) {
                const bool lower = (tid & j) == 0, up = (tid & k) == 0;      // this lane keeps the smaller key of the pair when lower == up
                const unsigned long long lo = mine < other ? mine : other, hi = mine < other ? other : mine;
                s_key[tid] = (lower == up) ? lo : hi;
            }
            __syncthreads();
        }
    }
    if (tid < PROC_ALLOW_WORDS / 4) reinterpret_cast<uint4*>(rec)[tid] = reinterpret_cast<const uint4*>(s_mask)[tid];
    if (tid < PROC_MAX_BIAS) {
        const unsigned long long key = s_key[tid];
        rec[PROC_IDS + tid] = (uint32_t)(key >> 32);
        rec[PROC_VALS + tid] = (uint32_t)key;
    }
    if (tid == 0) {
        reinterpret_cast<uint4*>(rec + PROC_HDR)[1] = make_uint4((uint32_t)h1.x, (uint32_t)h1.y, (uint32_t)h1.z, (uint32_t)h1.w);
        reinterpret_cast<uint4*>(rec + PROC_HDR)[0] = make_uint4(1u, (uint32_t)(h0.z < 0 ? 0 : h0.z), (uint32_t)n_stop, (uint32_t)n_bias);
    }
}
hipError_t launch_logitproc_build(const int32_t* stage, uint32_t* rec, hipStream_t s) {
    if (!stage || !rec) return hipErrorInvalidValue;
    hipLaunchKernelGGL(logitproc_build_kernel, dim3(1), dim3(LB_T), 0, s, stage, rec);
    return hipGetLastError();
}

// The record of a slot whose request has finished: unmarked
__global__ __launch_bounds__(64) void logitproc_reset_kernel(uint32_t* rec) {
    if (threadIdx.x == 0) rec[PROC_HDR] = 0u;
}
hipError_t launch_logitproc_reset(uint32_t* rec, hipStream_t s) {
    if (!rec) return hipErrorInvalidValue;
    hipLaunchKernelGGL(logitproc_reset_kernel, dim3(1), dim3(64), 0, s, rec);
    return hipGetLastError();
}

// ---- host --------------------------------------------------------------------------------------------
const char* logitproc_check(const T3LogitProcessors* p) {
    if (!p) return "T3LogitProcessors is NULL";
    if (p->struct_size != (int32_t)sizeof(T3LogitProcessors)) return "T3LogitProcessors.struct_size is not sizeof(T3LogitProcessors)";
    if (p->allowed_ids) {
        if (p->n_allowed < 0 || p->n_allowed > V) return "n_allowed outside [0, 8194]";
        for (int i = 0; i < p->n_allowed; ++i) if (p->allowed_ids[i] < 0 || p->allowed_ids[i] >= V) return "an allowed id outside [0, 8194)";
    }
    if (p->n_bias < 0 || p->n_bias > PROC_MAX_BIAS) return "n_bias outside [0, 64]";
    if (p->n_bias > 0 && (!p->bias_ids || !p->bias_vals)) return "n_bias > 0 without bias_ids / bias_vals";
    for (int i = 0; i < p->n_bias; ++i) {
        if (p->bias_ids[i] < 0 || p->bias_ids[i] >= V) return "a biased id outside [0, 8194)";
        for (int j = 0; j < i; ++j) if (p->bias_ids[j] == p->bias_ids[i]) return "a biased id is listed twice";
        const float b = p->bias_vals[i];
        if (b != b || b == INFINITY) return "a bias is NaN or +inf";
    }
    if (p->min_tokens < 0) return "min_tokens is negative";
    if (p->n_extra_stop < 0 || p->n_extra_stop > PROC_MAX_STOP - 1) return "n_extra_stop outside [0, 3]";
    for (int i = 0; i < p->n_extra_stop; ++i) if (p->extra_stop_ids[i] < 0 || p->extra_stop_ids[i] >= V) return "an extra stop id outside [0, 8194)";
    return nullptr;
}
int logitproc_stage(const T3LogitProcessors* p, int stop_token, int32_t* w, int32_t* stops) {
    memset(w, 0, (size_t)PROC_STAGE_ALLOW * 4);
    int n_stop = 0;
    if (stop_token >= 0 && stop_token < V) stops[n_stop++] = stop_token;
    for (int i = 0; i < p->n_extra_stop; ++i) stops[n_stop++] = p->extra_stop_ids[i];
    for (int i = n_stop; i < PROC_MAX_STOP; ++i) stops[i] = -1;
    w[0] = p->allowed_ids ? p->n_allowed : -1; w[1] = p->n_bias; w[2] = p->min_tokens; w[3] = n_stop;
    for (int i = 0; i < PROC_MAX_STOP; ++i) w[4 + i] = stops[i];
    for (int i = 0; i < p->n_bias; ++i) { w[PROC_STAGE_IDS + i] = p->bias_ids[i]; memcpy(w + PROC_STAGE_VALS + i, p->bias_vals + i, 4); }
    if (p->allowed_ids) memcpy(w + PROC_STAGE_ALLOW, p->allowed_ids, (size_t)p->n_allowed * 4);
    return n_stop;
}

}  // namespace t3
