// Internal launcher interface between engine.cpp / kernel_abi.cpp and the kernel translation units t3_gemm.hip, t3_attention.hip,
// t3_kernels.hip (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include "../../include/t3_engine.h"

namespace t3 {

constexpr int D = 1024, H = 16, HD = 64, F = 4096, V = 8194, VPAD = 8208, QKV = 3072;
constexpr int HEAD_TILES = 516;                   // speech head packed to a multiple of 4 n-tiles (513 hold rows)
constexpr int CHUNK = 64;                          // attention chunk in tokens (numerics contract)
#ifndef T3_KV_BLOCK
#define T3_KV_BLOCK 256
#endif
constexpr int KV_BLOCK = T3_KV_BLOCK;              // tokens per physical KV block (a multiple of CHUNK): per head 32 KiB K + 32 KiB V contiguous
#ifndef T3_KV_PAD
#define T3_KV_PAD 512
#endif
constexpr int KV_HEAD_PAD = T3_KV_PAD;               // elements of padding after every (kv, head) region: breaks the power-of-two
                                                   // strides (32 KiB per head, 512 KiB K->V) that make concurrent workgroups hit the same HBM channels
constexpr int KV_HEAD_ELEMS = KV_BLOCK * HD + KV_HEAD_PAD;
constexpr int KV_BLOCK_ELEMS = 2 * H * KV_HEAD_ELEMS;  // per layer per block: [kv][head][chunk][8 fragments][64 lanes][8]

// MXFP4 pool (t3_attention_fp4.hip, T3EngineConfig.kv_cache_dtype = 4), sized in BYTES: a head's 64-token chunk of K (or V) is CHUNK4 bytes of
// E2M1 nibbles followed by its 2 * CHUNK E8M0 scale bytes; the head regions keep KV_HEAD_PAD elements (here half a byte each) between them.
constexpr int CHUNK4 = CHUNK * HD / 2;
constexpr int CHUNK4_REC = CHUNK4 + 2 * CHUNK;
constexpr int KV4_HEAD_BYTES = (KV_BLOCK / CHUNK) * CHUNK4_REC + KV_HEAD_PAD / 2;
constexpr int KV4_BLOCK_BYTES = 2 * H * KV4_HEAD_BYTES;     // per layer per block
static_assert(KV4_HEAD_BYTES % 128 == 0, "a head region of the MXFP4 pool starts on a cache line");

enum GemmEpi { EPI_F32 = 0, EPI_BF16 = 1, EPI_RESID = 2, EPI_SILU = 3 };

// Weights of a LATER launch on the stream, pulled into the L2 of the XCD that will read them while this launch leaves the memory system
// idle: the fold + epilogue of a 4-wave GEMM form (0.4-1.3 us with nothing in flight), or behind the first group's barrier of the pipelined
// gate/up form (gemm2_pipe16_kernel: every weight tile has landed, only rows move).  The consumer is a gemm2_kernel whose workgroup bx
// reads the `group` packed n-tiles bx * group ... (tile_lines 128-byte lines each, contiguous); block b of EVERY launch lands on XCD
// (x0 + b) % 8 with the same x0 (tools/xcd_probe.hip: eager and graph launches, 1-D and 2-D grids of any size), so the lines of tile group g
// are requested by workgroups of this launch whose linear id is g mod 8, one line per lane and instruction, by LDS-DMA into a 256-byte
// corner of LDS nobody reads (a load into a register would be written whenever it lands, long after the compiler has given the register
// to something else: that build faulted).  Speed only: nothing depends on where the lines end up.
struct PrefetchArgs {
    const unsigned char* base = nullptr;   // null: nothing to prefetch
    int n_tiles = 0, tile_lines = 0, group = 1;
    int max_lines = 0;                     // > 0: only the first max_lines lines of every tile group
};

struct GemmArgs {
    const uint16_t* X;   // [M][K] bf16 row-major (NORM form: the un-normalised residual stream)
    const uint4* Wp;     // packed weight, see pack_weight() (NORM form: with the norm weight folded in, fold_norm_weight())
    int M, K, N;         // N = number of valid output columns (EPI_SILU: F)
    void* out;           // EPI_F32: float [M][ldo]; else bf16 [M][ldo]; EPI_RESID: residual stream, updated in place
    int ldo;
    int nw;              // waves = K segments per workgroup: 4 (qkv, gate/up, head) or 16 (o_proj, down_proj)
    int norm;                // 1: NORM form -- scale every row by rstd = 1/sqrt(mean(x^2) + eps) in the epilogue (K = 1024, nw = 4)
    const int* row_index;    // optional gather: source row of X per GEMM row (speech head over the sampled rows)
    int packed_tiles = 0;    // > 0: the packed weight holds this many n-tiles (zero rows beyond N), so tile groups may overhang N
    float* rstd_scratch = nullptr;   // [M] floats: lets the NORM forms take the prefill-sized schedule (row statistic in its own pass)
    PrefetchArgs pf;                 // gemm2_kernel, 4-wave forms: requested by the epilogue waves once the workgroup's own operands have landed
    int gx_real = 0;                 // set by the launcher: > 0 = the grid's x extent was padded (to a multiple of 8), workgroups with blockIdx.x >= gx_real leave at once
};

// Host-side packing of a [N][K] bf16 matrix into MFMA-B-operand order:
// out[((nt*KB + kb)*64 + lane)*8 + j] = W[nt*16 + (lane&15)][kb*32 + 8*(lane>>4) + j], rows >= N are zero.
void pack_weight(const uint16_t* W, int N, int K, int Npad, uint16_t* out);
// gate/up interleave: packed tile 2t = gate tile t, 2t+1 = up tile t.
void pack_gate_up(const uint16_t* Wg, const uint16_t* Wu, int Fdim, int K, uint16_t* out);
// W'[n][k] = bf16(W[n][k] * ln[k]) (host): an RMSNorm weight folded into the projection behind it, before packing
void fold_norm_weight(const uint16_t* W, int N, int K, const uint16_t* ln, uint16_t* out);

int choose_mt(int M, int ntiles_x, int nw = 4, bool norm = false);
hipError_t launch_gemm(const GemmArgs& a, int epi, int mt, hipStream_t s);
void set_pgemm_min_rows(int rows);   // row count from which launch_gemm takes the prefill schedule (process-wide; < 0 = default)
void set_pgemm_wide_rows(int rows);  // row count from which its 4-segment forms take 128 x 128 tiles (0 = never; < 0 = default 2048)

// The layer projections over MXFP8 weights (t3_gemm_mx8.hip, t3_set_weight_dtype = 1): format, packed layout and schedule stand at the head of that
// file.  epi: EPI_BF16 (qkv) / EPI_SILU (gate/up; N = F) with the RMSNorm statistic and rstd, K = 1024, 4 segments; EPI_RESID with 16 segments,
// K = 1024 (o) or 4096 (down).  N a multiple of 16, ldo even.
struct Mx8GemmArgs {
    const uint16_t* X;         // [M][K] bf16 row-major
    const uint4* Wq;           // packed E4M3 octets (pack_weight_mx8)
    const unsigned char* Ws;   // their E8M0 scale bytes: Wq's bytes + rows * K, rows = N (EPI_SILU: 2 F)
    int M, K, N;
    void* out;                 // bf16 [M][ldo]; EPI_RESID: the residual stream, updated in place
    int ldo;
};
hipError_t launch_gemm_mx8(const Mx8GemmArgs& a, int epi, hipStream_t s);
hipError_t prepare_gemm_mx8();      // dynamic-LDS limits of its instantiations (before any stream capture)
// host: y = the stored value of w, blocks of 32 along a row (cols a multiple of 32) -- the quantiser pack_weight_mx8 runs, and its inverse
void mx8_roundtrip(const uint16_t* w, uint16_t* y, int rows, int cols);
size_t mx8_packed_bytes(int N, int K);                    // octets + scale bytes of an [N][K] matrix: 8.25 bits per weight
// host: [N][K] bf16 (N a multiple of 16, K of 64) -> out[mx8_packed_bytes(N, K)]; kbs = k-blocks of 32 per K segment of the form that reads it (8; o: 2)
void pack_weight_mx8(const uint16_t* W, int N, int K, int kbs, unsigned char* out);
void pack_gate_up_mx8(const uint16_t* Wg, const uint16_t* Wu, int Fdim, int K, unsigned char* out);      // tiles interleaved as pack_gate_up's

// Per-row record of a step (int32 words), built by the scheduler and uploaded once per step:
//   [0] stream  [1] position  [2] embed kind  [3] embed a  [4] embed b  [5] alignment frame  [6] alignment n_text  [7] unused  [8 ..] KV block ids of the row's stream
// One lookup gives a kernel everything it needs to address the row's paged KV (no stream -> block-table hop).
// [5], [6]: read by the alignment tap and the guard only (t3_alignment.hip, t3_guard.hip). frame = index of the token this row's logits produce, -1 = the row is not
// tapped; n_text = text ids of its prompt.
constexpr int ROW_HDR = 8;
constexpr int ROW_ALIGN_FRAME = 5, ROW_ALIGN_NTEXT = 6;
inline int row_stride_words(int max_blocks) { return ROW_HDR + ((max_blocks + 3) & ~3); }

struct EmbedArgs {
    const int* rowrec; int row_stride;   // row records
    const float* cond;         // [max_seqs][34][1024] fp32
    const uint16_t *text_emb, *text_pos, *speech_emb, *speech_pos;
    uint16_t* h;               // [rows][1024]
    int rows;
    const int* prev_tok;       // the sampler's output array of the previous step (EMB_SPEECH_PREV)
    // The step's metadata (selection arrays + row records) as the host wrote it, in pinned host memory: this launch reads its own row
    // records from there and leaves the device copy every later launch of the step reads (no copy kernel in front of the step).
    const int4* host_meta = nullptr; int4* dev_meta = nullptr; int meta_vec = 0;      // meta_vec 16-byte pieces
    const int* host_rowrec = nullptr;                                               // rowrec's twin inside host_meta
};
enum EmbedKind { EMB_COND = 0 /*a=slot,b=idx*/, EMB_TEXT = 1 /*a=id,b=pos*/, EMB_ZERO = 2, EMB_SPEECH = 3 /*a=id,b=pos*/,
                 EMB_SPEECH_PREV = 4 /*a=index into prev_tok,b=pos*/ };
hipError_t launch_embed(const EmbedArgs& a, hipStream_t s);

struct RopeArgs {
    const uint16_t* qkv;       // [rows][3072]
    uint16_t* q_out;           // [rows][1024]
    uint16_t* kv_layer;        // pool + layer*n_blocks*KV_BLOCK_ELEMS
    const int* rowrec; int row_stride;   // row records
    const float *cos_t, *sin_t;  // [max_pos][32]
    int rows;
};
hipError_t launch_rope_kv(const RopeArgs& a, hipStream_t s);

struct AttnArgs {
    const uint16_t* q;         // [rows][1024] rotated (unfused form)
    const uint16_t* kv_layer;
    const int* rowrec; int row_stride;   // row records
    uint16_t* out;             // [rows][1024]
    int rows;
    int max_chunks;            // LDS sizing: ceil(max_model_len/64)
    // fused decode form (every row is the newest position of its stream): RoPE of q,k + KV write happen here
    const uint16_t* qkv;       // [rows][3072] pre-RoPE, or null for the unfused form
    uint16_t* kv_layer_w;      // writable alias of kv_layer
    const float *cos_t, *sin_t;
    // unfused form: rows [tile_from, rows) are prefill rows and take the 16-rows-per-workgroup schedule (-1: none); tile_chunks =
    // ceil(longest context among them / 64) sizes its LDS (0: max_chunks)
    int tile_from = -1, tile_chunks = 0;
    int force_waves = 0;       // 4 / 8: waves per (row, head) workgroup of the per-row kernel (0: by row count; parity tests check both)
};
hipError_t launch_attention(const AttnArgs& a, hipStream_t s);
// parity hook: K (as stored, i.e. rotated) and V of every row's (stream, position) read back from the paged pool -> out [rows][2][1024]
hipError_t launch_kv_gather(const uint16_t* kv_layer, const int* rowrec, int row_stride, int rows, uint16_t* out, hipStream_t s);
// The same three over an FP8 (E4M3FN) pool, t3_attention_fp8.hip (T3EngineConfig.kv_cache_dtype = 1): same argument structs, but kv_layer /
// kv_layer_w point at ONE-byte elements (a layer of the pool is n_blocks * KV_BLOCK_ELEMS bytes); the gather dequantises to bf16.
hipError_t launch_rope_kv_fp8(const RopeArgs& a, hipStream_t s);
hipError_t launch_attention_fp8(const AttnArgs& a, hipStream_t s);
hipError_t launch_kv_gather_fp8(const uint16_t* kv_layer, const int* rowrec, int row_stride, int rows, uint16_t* out, hipStream_t s);
hipError_t launch_fp8_roundtrip(const float* x, float* y, int n, hipStream_t s);   // parity hook: y = dequantised q8(x)
// And over an MXFP4 pool, t3_attention_fp4.hip (kv_cache_dtype = 4): kv_layer / kv_layer_w point at bytes, a layer of the pool is
// n_blocks * KV4_BLOCK_BYTES of them.
hipError_t launch_rope_kv_fp4(const RopeArgs& a, hipStream_t s);
hipError_t launch_attention_fp4(const AttnArgs& a, hipStream_t s);
hipError_t launch_kv_gather_fp4(const uint16_t* kv_layer, const int* rowrec, int row_stride, int rows, uint16_t* out, hipStream_t s);
hipError_t launch_fp4_roundtrip(const float* x, float* y, int n, hipStream_t s);   // parity hook: y = the stored value of x, blocks of 32 (n a multiple of 32)

// The alignment tap (t3_alignment.hip): attention probabilities of ONE head over the span [lo, lo + n_text) of each tapped row's context,
// K only.  Workgroup i serves row sel_rows[2 i] (the conditional row of sampled utterance i; sel_rows null: row i) and leaves at once where
// the row record's frame word is -1.  Destination: out[((stream / 2) * frames_per_slot + frame) * ld + t].
struct AlignArgs {
    const uint16_t* qkv;       // [rows][3072] pre-RoPE: the step's qkv buffer
    const void* kv_layer;      // the layer's pool (bf16, one-byte E4M3 elements, or MXFP4 bytes), holding the rows' newest K already
    const int* rowrec; int row_stride;
    const int* sel_rows;       // nullable
    const float *cos_t, *sin_t;
    float* out;
    int n_wg;                  // workgroups: sampled utterances of the step (or rows)
    int head, lo, max_chunks;
    int frames_per_slot, ld;
    int tap, n_taps; float inv_taps;     // tap 0 stores, later taps add, tap n_taps - 1 scales by inv_taps
    uint16_t* q_rot_out = nullptr;       // nullable (parity hook): [rows][64] the rotated q the tap used
};
hipError_t launch_alignment(const AlignArgs& a, int kv_dtype, hipStream_t s);   // kv_dtype: T3EngineConfig.kv_cache_dtype (0, 1, 4)
hipError_t launch_alignment_clear(float* p, size_t n, hipStream_t s);   // p[0 .. n) = 0 by a kernel; n a multiple of 4, p 16-byte aligned

struct SampleArgs {
    const uint16_t* logits;    // [2*n][ldl] bf16: row 2i cond, 2i+1 uncond
    int ldl;
    const int4* sel;           // per sampled utterance {slot, step, 0, 0}
    uint16_t* counts;          // [max_seqs][VPAD]
    const T3Sampling* sp;      // [max_seqs], indexed by slot
    float cfg;
    int* out_tok;              // [n]
    float* dbg;                // nullable: [max_seqs][V]
    int n;
    int* hist = nullptr;       // nullable: [max_seqs][hist_cap] speech-space ids of every utterance, kept on the device (f4 hand-off)
    int hist_cap = 0;
    int* out_tok_host = nullptr;   // nullable: [n] in pinned host memory, written beside out_tok (no copy kernel behind the step)
    unsigned char* dbg_keep = nullptr;   // nullable (parity hook t3k_sample_support): [max_seqs][V] 1 where the draw can return the id
    const int* eos_ctl = nullptr;  // nullable: [max_seqs] guard control words (t3_guard.hip), obeyed for the slots whose sp.alignment is 2.  Non-null
                                   // launches the sampler's guarded instantiation; null launches the kernel as it was before the guard existed
    const uint32_t* proc = nullptr;    // nullable: [max_seqs][PROC_WORDS] logit-processor records (t3_logitproc.hip).  Non-null launches the sampler's third
                                       // instantiation (it obeys eos_ctl too, where that is set); a slot whose record is unmarked is sampled as without it
    float* dbg_proc = nullptr;         // nullable (parity hook t3k_sample_proc): [max_seqs][V] the logits behind the processors (allow, bias, min_tokens)
};
hipError_t launch_sampler(const SampleArgs& a, hipStream_t s);

// Logit processors (t3_logitproc.hip; the contract stands in include/t3_engine.h, "logit processors").  A slot's RECORD, PROC_WORDS 32-bit words in
// device memory, 16-byte aligned, is what the sampler reads:
//   [0, 264)    allow bitmask: bit v & 31 of word v >> 5 set = id v may be drawn (bits from 8194 on are clear)
//   [264, 328)  the biased ids, ascending, padded with INT32_MAX        [328, 392)  their fp32 biases, in the same order
//   [392] 1 = marked, 0 = unmarked (nothing else of the record is valid then)   [393] min_tokens   [394] n_stop   [395] n_bias   [396, 400) the stop ids
// The STAGING image of a request, PROC_STAGE_WORDS words in pinned host memory, is what the host writes and the build kernel reads:
//   [0] n_allowed, -1 = every id   [1] n_bias   [2] min_tokens   [3] n_stop   [4, 8) stop ids   [8, 72) bias ids, any order   [72, 136) their biases
//   [136, 136 + n_allowed) the allowed ids, any order, duplicates welcome
constexpr int PROC_ALLOW_WORDS = 264, PROC_MAX_BIAS = T3_MAX_LOGIT_BIAS, PROC_MAX_STOP = 4;
constexpr int PROC_IDS = PROC_ALLOW_WORDS, PROC_VALS = PROC_IDS + PROC_MAX_BIAS, PROC_HDR = PROC_VALS + PROC_MAX_BIAS, PROC_WORDS = PROC_HDR + 8;
constexpr int PROC_STAGE_IDS = 8, PROC_STAGE_VALS = PROC_STAGE_IDS + PROC_MAX_BIAS, PROC_STAGE_ALLOW = PROC_STAGE_VALS + PROC_MAX_BIAS;
constexpr int PROC_STAGE_WORDS = (PROC_STAGE_ALLOW + V + 3) & ~3;
static_assert(PROC_ALLOW_WORDS * 32 >= VPAD && PROC_WORDS % 4 == 0 && PROC_MAX_BIAS == 64, "logit-processor record layout");
// host: nullptr = well-formed, else what is malformed (t3_request_logit_processors' T3_E_INVALID cases); stop_token = T3Sampling.stop_token
const char* logitproc_check(const T3LogitProcessors* p);
// host: the staging image of a checked struct, PROC_STAGE_WORDS words; returns the request's stop list (stop_token first if it is one) in stops[4]
int logitproc_stage(const T3LogitProcessors* p, int stop_token, int32_t* words, int32_t* stops);
hipError_t launch_logitproc_build(const int32_t* stage, uint32_t* rec /*the slot's record*/, hipStream_t s);
hipError_t launch_logitproc_reset(uint32_t* rec /*the slot's record*/, hipStream_t s);      // the record's flag word = 0, by a kernel

// The alignment guard (t3_guard.hip): one wave per sampled utterance reads the frame the step's taps have just completed, moves the slot's
// state (include/t3_engine.h spells the rules out) and leaves the control word the step's sampler obeys.
constexpr int GUARD_NONE = 0, GUARD_SUPPRESS = 1, GUARD_FORCE = 2;
constexpr int GUARD_STATE_WORDS = 8;   // pos | complete + 256 reason | completed_at | forced_at + 1 | tail[3] (fp32) | rep (fp32): all zero = admitted
struct GuardArgs {
    const float* frames;       // [max_seqs][frames_per_slot][ld]: the alignment frames (AlignArgs.out)
    int frames_per_slot, ld;
    const int* rowrec; int row_stride;
    const int* sel_rows;       // nullable: wave u serves row sel_rows[2 u] (null: row u)
    const int4* sel;           // per sampled utterance {slot, step, 0, 0}
    const T3Sampling* sp;      // [max_seqs]: alignment == 2 marks a guarded slot, stop_token ends its utterance
    const int* hist; int hist_cap;      // the sampler's history (SampleArgs.hist)
    int* state;                // [max_seqs][GUARD_STATE_WORDS]
    int* ctl;                  // [max_seqs]
    int n_sel;
    T3GuardParams p;
};
hipError_t launch_guard(const GuardArgs& a, hipStream_t s);
hipError_t launch_guard_reset(int* state, int* ctl, int slot, hipStream_t s);   // the slot's state and control word = 0, by a kernel
void guard_unpack_state(const int* words, T3GuardState* out);                  // host: state words -> the ABI's struct
// Per-token log-probabilities (t3_logprobs.hip): workgroup u serves sampled utterance u directly behind the step's sampler -- the raw log-probability
// and rank of the id it drew and the k = lp_k[slot] most likely ids, over the post-CFG logits of the 8194 speech ids.  Destination: the record
// rec[(slot * rec_steps + step) * 2 (K + 1)] = {rank, lp_tok, (id, lp) x k}.  A workgroup whose slot is not marked (lp_k[slot] < 0) leaves at once.
struct LogprobArgs {
    const uint16_t* logits; int ldl;   // SampleArgs.logits / ldl (ldl a multiple of 8)
    const int4* sel;           // per sampled utterance {slot, step, 0, 0}
    const int* out_tok;        // [n]: what the sampler has just drawn
    const int* lp_k;           // [max_seqs]: -1 = not marked, else k in 0 .. K
    float cfg;
    int* rec;                  // [max_seqs][rec_steps][2 (K + 1)] 32-bit words
    int rec_steps, K;
    int n;
    // mode 1 = PROCESSED (t3_set_logprobs_mode): over z_v, the value the sampler draws from -- behind the slot's logit processors, the guard's
    // suppression, the penalties and the temperature.  It reads what the step's sampler read: counts / sp as SampleArgs has them (the drawn id's count
    // already raised), proc / eos_ctl nullable exactly where the sampler's launch left them null.  mode 0 reads none of the five.
    const uint16_t* counts = nullptr;      // [max_seqs][VPAD], 16-byte aligned
    const T3Sampling* sp = nullptr;        // [max_seqs]
    const uint32_t* proc = nullptr;        // nullable: [max_seqs][PROC_WORDS]
    const int* eos_ctl = nullptr;          // nullable: [max_seqs]
    int mode = 0;
};
hipError_t launch_logprobs(const LogprobArgs& a, hipStream_t s);
hipError_t launch_logprobs_mark(int* lp_k, int slot, int k, hipStream_t s);     // lp_k[slot] = k, by a kernel
// Token time spans (t3_align_path.hip): one wave per request runs the monotonic path search of DESIGN.md section 8 over a finished alignment
// matrix and leaves, per text id, the [start, end) frames the path spends on it.
struct AlignPathItem {
    const float* A;            // [n_frames][ld] fp32, columns >= n_text are never read into a result
    int n_frames, n_text, ld, _pad;
    unsigned long long* bp;    // workspace [n_frames][ceil(n_text / 64)]: bit l of word j of row k = cell (k, 64 j + l) came from t - 1
    int* path;                 // [n_frames]
    int* start; int* end;      // [span_ld] each: -1 beyond the path's last id
    int* res;                  // [2]: last, score
};
constexpr int ALIGN_PATH_MAX_TEXT = 2112, ALIGN_PATH_MAX_FRAMES = 8192;      // 33 slots of 64 ids; 8192 x 65536 stays below 2^30
hipError_t launch_align_path(const AlignPathItem* items /*device [n]*/, int n, int max_text /*over the items*/, int span_ld, hipStream_t s);
hipError_t launch_align_scores(const float* a, int* w, int n, hipStream_t s);
// Profile mode: the next single-kernel launch of this thread (decode GEMM forms, fused / per-row attention, embed, sampler) takes these as
// its start / stop events (hipExtLaunchKernelGGL); launch_events_armed() afterwards tells whether a launcher consumed them.
void arm_launch_events(hipEvent_t start, hipEvent_t stop);
bool launch_events_armed();
hipError_t prepare_kernels();   // one-time function attributes (must run before any stream capture)
hipError_t prepare_gemm2();     // its GEMM part (t3_gemm.hip)
void gemm_refresh_switches();   // re-reads the measurement switches of the GEMM launchers (per engine)
hipError_t launch_expf(const float* x, float* y, int n, hipStream_t s);

// f4: batched token hand-off to the vocoder.  One workgroup per utterance applies the reference's post-filter (tts.py:300-365 +
// alignment_stream_analyzer.py:111-201 + the range filter of tts.py:514 -- the same integer rules as t3_clean_tokens) to the
// utterance's device-resident ids and writes one padded row + length.
struct HandoffItem { const int* src; int n; int text_token_count; int _pad; };
hipError_t launch_handoff(const HandoffItem* items /*device [n_utt]*/, int n_utt, int flags, int* out /*device [n_utt][ld]*/, int ld, int* lens /*device [n_utt]*/, hipStream_t s);

void rope_tables(int max_pos, float* cos_t, float* sin_t);   // host, llama3 scaling, bf16-valued

}  // namespace t3
