/*
 * t3_engine.h -- C ABI of the MI355X-native T3 speech-token decode engine (libt3engine.so).
 *
 * This is the drop-in boundary for the ONE hot path of groxaxo/chatterbox-vllm2: everything that
 * happens between `LLM.generate(prompts, sampling_params)` and `output.token_ids`
 * (reference src/chatterbox_vllm/tts.py:445-465, 485) -- i.e. what the reference delegates to
 * vllm==0.10.0 plus its model plugin src/chatterbox_vllm/models/t3/t3.py.  The reference is pure
 * Python, so the "FFI" a maintainer binds is ctypes (see INTEGRATION.md for the stub).
 *
 * Conventions: every function returns 0 on success or a negative T3_E_* code; the message is
 * available from t3_last_error().  No exceptions cross the boundary.  The caller owns all host
 * buffers; the engine owns all device memory.  One handle per GPU; a handle is NOT thread-safe
 * (one driver thread per handle -- the reference's caller is a single blocking FastAPI handler,
 * api_server.py:265-271).  Token ids at this boundary are in the reference's OFFSET space
 * (speech id + 2500, t3.py:49,669-672) unless a function says "speech-space".
 */
#ifndef T3_ENGINE_H
#define T3_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define T3_OK 0
#define T3_E_INVALID (-1)   /* bad argument (maps to ValueError -> HTTP 400, api_server.py:323-326) */
#define T3_E_DEVICE (-2)    /* HIP error */
#define T3_E_NOMEM (-3)     /* KV pool / device memory exhausted */
#define T3_E_STATE (-4)     /* call not valid in this state (e.g. step before finalize_weights) */
#define T3_E_NOTFOUND (-5)  /* unknown request id / tensor name */

#define T3_SPEECH_TOKEN_OFFSET 2500 /* t3.py:49 */
#define T3_COND_ROWS 34             /* t3.py:42 */
#define T3_HIDDEN 1024
#define T3_SPEECH_VOCAB 8194        /* t3_config.py:10 */

typedef struct T3Engine* T3Handle;

/* Replaces the kwargs of `LLM(model=..., gpu_memory_utilization=, enforce_eager=, max_model_len=, **kw)`
 * (tts.py:150-171) and the env var CHATTERBOX_CFG_SCALE (t3.py:296). */
typedef struct {
    int32_t device_id;
    int32_t n_layers;          /* 30 for the real model (config.json:17); small values for tests */
    int32_t text_vocab;        /* 704 English / 2454 multilingual (t3.py:270) */
    int32_t max_model_len;     /* tts.py:164 */
    int32_t max_seqs;          /* utterance slots (vLLM max_num_seqs); each slot = 2 CFG streams */
    int32_t max_batched_rows;  /* rows (stream-tokens) per step budget, >= 2*max_seqs; 0 = default */
    int64_t kv_bytes;          /* KV pool size; 0 = derive from gpu_memory_utilization */
    float gpu_memory_utilization; /* fraction of total HBM the engine may use (tts.py:162) */
    float cfg_scale;           /* CHATTERBOX_CFG_SCALE, default 0.5 (t3.py:296) */
    int32_t enforce_eager;     /* 1: never use hipGraph replay (tts.py:163) */
    int32_t debug_logits;      /* 1: keep post-CFG logits of each sampled step for t3_debug_logits */
    int32_t n_groups;          /* utterance groups run concurrently on separate HIP streams; 0 = auto */
    int32_t kv_cache_dtype;    /* storage format of the paged KV pool: 0 = bf16 (default), 1 = FP8 E4M3FN with scale 1.0 (vLLM's
                                  kv_cache_dtype="fp8": half the bytes per token), 4 = MXFP4 (E2M1 elements, one E8M0 scale per 32 head
                                  dims of one token: 1088 bytes per token and layer against 4096); any other value, 2 and 3 included,
                                  is T3_E_INVALID.  This was padding: a C caller must zero it */
} T3EngineConfig;

/* Replaces vllm.SamplingParams as configured at tts.py:455-464 (+ the kwargs it forwards). */
typedef struct {
    float temperature;         /* < 1e-5 => greedy */
    float top_p;               /* 1.0 = off */
    float min_p;               /* 0.0 = off (reference accepts min_p but never forwards it, tts.py:415) */
    float repetition_penalty;  /* 1.0 = off; reference default 2.0 (tts.py:416) */
    float presence_penalty;
    float frequency_penalty;
    int32_t top_k;             /* <= 0 = off */
    int32_t max_tokens;        /* tts.py:459 */
    int32_t ignore_eos;        /* fixed-length generation for synthetic benchmarks */
    int32_t stop_token;        /* SPEECH-SPACE stop id, 6562 (= 9062 - 2500, tts.py:458); -1 none */
    uint64_t seed;
    uint64_t uid;              /* utterance id keying the RNG stream: results do not depend on batch
                                  composition or on data-parallel sharding */
    int32_t pos_policy;        /* 0: k-th generated token uses speech_pos_emb[k] (SURVEY.md 9 Q1 "exact");
                                  1: index 0 for every decode token (the literal fallback of t3.py:464) */
    int32_t alignment;         /* 1: keep the text-speech alignment matrix of this request (t3_get_alignment; needs t3_reserve_alignment);
                                  2: the same, and the alignment guard reads every frame and suppresses or forces stop_token (needs
                                  t3_set_alignment_guard, stop_token >= 0 and ignore_eos = 0); 0: off (default).  Any other value is
                                  T3_E_INVALID.  Token ids never depend on it unless it is 2.  This was padding: a C caller must zero it */
} T3Sampling;

typedef struct {
    int32_t n_rows;            /* rows processed this step */
    int32_t n_prefill_rows;
    int32_t n_sampled;         /* utterances that produced a token this step */
    int32_t n_finished;        /* finished this step */
    int32_t n_running;         /* after the step */
    int32_t n_waiting;
    int64_t finished_ids[64];  /* first min(n_finished, 64); every finished id, in order, is also queued for t3_pop_finished */
} T3StepResult;

typedef struct {
    int64_t steps;
    int64_t decode_steps;          /* steps with no prefill rows */
    int64_t tokens_generated;
    int64_t prefill_rows;
    int64_t decode_rows;
    double gpu_ms_total;           /* HIP-event time of all steps */
    double gpu_ms_decode;          /* ... of decode-only steps */
    double algo_bytes_decode;      /* SURVEY.md 8(d) formula summed over decode-only steps */
    double sum_ctx_decode;         /* sum over decode rows of context length */
    int64_t kv_blocks_total, kv_blocks_free;
    int64_t weight_bytes;
    int64_t finished_dropped;      /* ids t3_pop_finished will never return: the queue of finished ids holds 4 * max_seqs + 4096 entries and drops the oldest beyond that (a caller that never pops must not grow it) */
} T3Stats;

/* ---- lifecycle ------------------------------------------------------------------------- */
int t3_create(const T3EngineConfig* cfg, T3Handle* out);
int t3_destroy(T3Handle h);                      /* `del self.t3`, tts.py:527-529 */
const char* t3_last_error(T3Handle h);           /* h may be NULL for create() failures */

/* ---- weights: T3VllmModel.load_weights (t3.py:300-332) ---------------------------------
 * name: checkpoint tensor name ("tfmr.layers.3.self_attn.q_proj.weight", "speech_emb.weight",
 * "text_pos_emb.emb.weight", "speech_head.weight", ...).  Unknown prefixes (cond_enc.*, text_head.*)
 * return T3_E_NOTFOUND and may be ignored by the caller, as t3.py:316-319 does.
 * data: host or device pointer to bf16 ([rows][cols], row-major).                          */
int t3_load_tensor(T3Handle h, const char* name, const void* data_bf16, int32_t rows, int32_t cols);
int t3_finalize_weights(T3Handle h);             /* packs weights for the GEMM kernels, builds RoPE tables, allocates the KV pool */

/* ---- requests: LLM.generate (tts.py:445-465) -------------------------------------------
 * prompt_ids: the FINAL prompt [695, x*32, 696, text ids..., 697] of length T (t3.py:189-200);
 * cond_emb: fp32 [34][1024] host buffer (tts.py:286 hands the conditionals over on CPU).   */
int t3_add_request(T3Handle h, int64_t req_id, const int32_t* prompt_ids, int32_t T,
                   const float* cond_emb, const T3Sampling* sampling);
int t3_step(T3Handle h, T3StepResult* res);      /* admit -> prefill/decode rows -> sample, once */
int t3_run_until_done(T3Handle h);               /* C++ loop, no Python per step */
/* Runs at most n steps (stops early when nothing is left); *done = steps actually run. */
int t3_run_steps(T3Handle h, int32_t n, int32_t* done);
int t3_num_unfinished(T3Handle h);
/* Ids of the requests that finished since the previous call (any of t3_step / t3_run_steps / t3_run_until_done), oldest first:
 * up to `cap` of them are written to ids and leave the queue.  Returns how many were written (a step of 128 utterances can retire
 * more than the 64 that fit T3StepResult), or a negative T3_E_* code.  The queue keeps the most recent 4 * max_seqs + 4096 ids: a
 * serving loop pops after every step; a caller that reads outputs by request id need not pop at all.  vLLM hands finished RequestOutputs back from every
 * engine step (LLM.generate collects them, tts.py:445-465); this is that stream of ids. */
int t3_pop_finished(T3Handle h, int64_t* ids, int32_t cap);
/* ids: offset-space token ids (>= 2500), the stop id included when hit.
 * On entry *n = capacity; on exit *n = number of tokens.  finish_reason: 0 running, 1 stop, 2 length. */
int t3_get_output(T3Handle h, int64_t req_id, int32_t* ids, int32_t* n, int32_t* finish_reason);
/* Host wall-clock marks of a request, seconds since t3_create: out4 = {added (t3_add_request), admitted (slot + KV blocks
 * granted), first token read back, finished}; 0 where not reached yet.  The reference's clock is the wall time of its
 * `self.t3.generate` call (tts.py:444,466-467); per request, RTF = (finished - admitted) / (n_tokens / 25). */
int t3_get_timing(T3Handle h, int64_t req_id, double* out4);
int t3_release_request(T3Handle h, int64_t req_id);   /* forget a finished request */
/* Drop a request in any state -- vLLM's abort_request: a WAITING one leaves the queue, a running one gives its slot and KV
 * blocks back -- and forget it.  The host mirror uses it to roll back a generate() call whose later prompt was rejected
 * (api_server.py:323-326 turns that ValueError into HTTP 400 and the engine must be left empty).  Not valid while a step is
 * in flight (the engine is single-threaded: call it between t3_step / t3_run_* calls). */
int t3_abort_request(T3Handle h, int64_t req_id);

/* ---- token post-filter: ChatterboxTTS.analyze_and_clean_tokens (tts.py:300-365) driving the fork's
 * token-heuristic AlignmentStreamAnalyzer.step (models/t3/inference/alignment_stream_analyzer.py:111-201), plus the
 * range filter of tts.py:514.  Pure integer logic on the host (the reference does it with one CUDA tensor + .item()
 * sync per token).  speech_ids: speech-space ids (already un-offset, tts.py:492); text_token_count as tts.py:496.
 * The output is the prefix before the first token at which the analyzer forces EOS -- three identical tokens in a
 * row, or >= 10 frames after the estimated end of the text (frame/2 >= text_token_count - 3).
 * flags bit 0: also drop ids outside [0, 6561) (tts.py:514).  reason (nullable): 0 none, 1 repetition, 2 long tail.
 * Returns the number of tokens written to out (capacity n), or a negative T3_E_* code.                        */
int t3_clean_tokens(const int32_t* speech_ids, int32_t n, int32_t text_token_count, int32_t flags,
                    int32_t* out, int32_t* reason);

/* ---- T3 -> S3Gen hand-off --------------------------------------------------------------------------
 * Replaces the per-utterance loop of ChatterboxTTS.generate_with_conds after the engine call (tts.py:483-514): `token - 2500`,
 * analyze_and_clean_tokens (one CUDA tensor + .item() sync per token, tts.py:335-344), torch.tensor(ids, device="cuda")
 * (tts.py:365) and the [0, 6561) mask (tts.py:514), once per utterance.  Here the ids never leave the device: the sampler keeps
 * every utterance's ids in HBM, and this call filters, compacts and pads a whole batch in one launch, straight into the caller's
 * DEVICE buffers in the layout a batched vocoder front-end takes (speech_tokens [n][ld] int32, speech_token_lens [n]; the
 * reference's flow.inference asserts batch 1, flow.py:256, so today's caller slices row i to lens[i]).
 * req_ids: n FINISHED, not yet released requests; text_token_counts as tts.py:496; flags bit 0: range filter of tts.py:514.
 * dev_tokens: device int32 [n][ld], rows padded with 0 beyond lens; dev_lens: device int32 [n].  Returns when the buffers are
 * ready (the call synchronises its own stream).                                                                        */
int t3_handoff_tokens(T3Handle h, const int64_t* req_ids, int32_t n, const int32_t* text_token_counts, int32_t flags,
                      int32_t* dev_tokens, int32_t ld, int32_t* dev_lens);
/* Switches the retention of finished utterances' ids in device memory on (n_requests > 0) or off (0; the default: a caller
 * that reads ids with t3_get_output pays nothing for the hand-off), and makes sure buffers for n_requests finished-and-unreleased
 * utterances exist BEFORE the step loop runs (max_model_len int32 each).  If more than that finish unreleased, the pool grows inside
 * the loop and an allocation failure there is reported by the step call (T3_E_NOMEM), not by a later t3_handoff_tokens. */
int t3_reserve_handoff(T3Handle h, int32_t n_requests);

/* ---- text-speech alignment export -------------------------------------------------------------------------------------
 * What the upstream AlignmentStreamAnalyzer reads from its attention hooks (LLAMA_ALIGNED_HEADS) and the vLLM port lost
 * (alignment_stream_analyzer.py:139-141 falls back to frame // 2): for a request submitted with T3Sampling.alignment = 1, the fp32 matrix
 *   A[k][t] = mean over the configured (layer, head) taps of softmax_j(q_k . K_j / 8)[34 + t],   k < n_tokens, t < n_text
 * where q_k is the rotated query of the CONDITIONAL stream's row whose logits produced token k (position T - 1 + k; k = 0 is the BOS row of
 * the prefill), j runs over that row's whole causal context, 34 + t over the text span [34, T - 1) of the prompt, and K is the key as the
 * pool stores it (bf16, or the dequantised E4M3 value).  Row k is upstream's per-frame `A_chunk`.  With alignment = 0 a step launches exactly
 * what it launches without this feature.
 * t3_reserve_alignment: allocates (max_text_tokens > 0) or frees (0) the per-slot frame buffers, max_seqs x max_model_len x max_text_tokens
 * (rounded up to a multiple of 4) fp32; T3_E_NOMEM names the byte count.  Not valid while requests are queued or running.  A request with
 * alignment = 1 is T3_E_STATE before a reserve and T3_E_INVALID when its text is longer than the reserve.  A reserve and t3_set_alignment_heads
 * drop the captured decode-step graphs (they carry the buffer, its pitch and the taps); the next steps capture again.  The matrices of finished
 * requests live in pooled buffers of max_model_len x max_text_tokens fp32 that t3_release_request gives back for reuse. */
int t3_reserve_alignment(T3Handle h, int32_t max_text_tokens);
/* The taps: n (1..4) pairs (layer, head), layers strictly ascending and < n_layers, heads < 16.  Default: the reference's three heads in layer
 * order, (9, 2), (12, 15), (13, 11), restricted to the layers that exist; if none exists and none was set, an alignment = 1 request is
 * T3_E_STATE.  Valid only while no request is queued or running (T3_E_STATE otherwise). */
int t3_set_alignment_heads(T3Handle h, const int32_t* layer_head_pairs, int32_t n);
/* The matrix of a FINISHED, not yet released request, row-major [n_frames][n_text].  On entry *n_frames x *n_text is the capacity of out in
 * floats (out may be NULL to ask for the extents only); on exit they hold the real extents: n_frames = the number of tokens t3_get_output
 * returns, n_text = T - 35.  Unknown (or released) id: T3_E_NOTFOUND; a request submitted with alignment = 0 or a buffer too small:
 * T3_E_INVALID; not finished: T3_E_STATE. */
int t3_get_alignment(T3Handle h, int64_t req_id, float* out, int32_t* n_frames, int32_t* n_text);
/* Token time spans: WHEN each text token is spoken, from the matrices of n FINISHED, not yet released requests submitted with alignment >= 1,
 * by one kernel launch (t3_align_path.hip, one wave per request); only the spans cross to the host.  The path is Glow-TTS's monotonic
 * alignment search with a free end over integer cell scores (DESIGN.md section 8 states the contract):
 *   w[k][t] = rint(1024 log2 a'), a' = A[k][t] clamped into [2^-64, 2^64] (NaN, zero and negatives: 2^-64), log2 by exponent + a degree-5 polynomial;
 *   D[0][0] = w[0][0]; D[k][t] = w[k][t] + max(D[k-1][t], D[k-1][t-1]) for t <= k, the step from t - 1 taken only when strictly larger;
 *   last = the lowest t with the largest D[n_frames-1][t]; the path runs back from (n_frames - 1, last) to (0, 0) in steps of 0 or 1.
 * start / end: host arrays [n][ld]; row i holds, per text id t <= last[i], the first frame on t and one past its last frame, and -1 for every other
 * t < ld (beyond last, beyond the request's n_text).  Seconds = frame / 25.  n_text, last, score (= D at the end cell): [n] each, nullable.
 * ld smaller than some request's n_text: T3_E_INVALID; the other codes are t3_get_alignment's.  The call synchronises its own stream. */
int t3_get_token_spans(T3Handle h, const int64_t* req_ids, int32_t n, int32_t ld, int32_t* start, int32_t* end, int32_t* n_text, int32_t* last,
                       int32_t* score);

/* ---- alignment guard: EOS suppressed or forced on the device, from the alignment frames --------------------------------
 * The logits half of upstream's AlignmentStreamAnalyzer, as a kernel inside the step (t3_guard.hip) and a sampler that obeys it.  For a request
 * submitted with T3Sampling.alignment = 2, with S = n_text, a_k = row k of its alignment matrix and tok[k] the id drawn at step k, the state
 * {pos, complete, completed_at, tail[3], rep, reason, forced_at = -1}, all zero at admission, moves at step k, before that step's sampler:
 *   1. c = lowest index attaining max_t a_k[t], t < S.  -back < c - pos < fwd: pos = c; otherwise (a discontinuity) pos stays.
 *   2. !complete and pos >= S - end: complete = 1, completed_at = k.
 *   3. complete (this step included): tail[i] += a_k[S - 3 + i] for i < 3 with S - 3 + i >= 0;  rep += max(a_k[0 : S - skip]) (0 for an empty
 *      range).  One fp32 add each per step, in step order.
 *   4. long_tail = complete && max(tail) >= tail_thr;  align_rep = complete && rep > rep_thr;
 *      tok_rep_hit = tok_rep > 0 && k >= tok_rep && tok[k-1] == ... == tok[k-tok_rep].
 *   5. FORCE if one of them holds: reason = 1 token repetition, 2 long tail, 3 alignment repetition (the first in that order), forced_at = k;
 *      the state is frozen from then on and every later step of the slot is forced too.  Otherwise SUPPRESS if pos < S - end && S > skip.
 *      Otherwise nothing.
 * SUPPRESS: the stop id's post-CFG logit is -inf in front of penalties, temperature, min-p, top-k and top-p, as if the caller had handed in the
 * conditional logits with that column at -inf.  FORCE: the step's id is the stop id whatever the logits hold (NaN rows included); history and
 * counts are written as for any drawn id, the request finishes with reason 1 and the stop id as its last token.  A step scheduled behind the
 * one that drew the stop id (run-ahead, bursts) changes nothing: the state t3_get_guard returns is the state after the utterance's last step.
 * The defaults follow upstream's analyzer as its rules are known to the maintainers; they have NOT been validated against a real checkpoint
 * on this project, which is why every one of them is a parameter. */
typedef struct {
    int32_t struct_size;       /* sizeof(T3GuardParams).  Every other field 0: the defaults below; otherwise every field is taken as given */
    int32_t back, fwd;         /* 4, 7: the window -back < c - pos < fwd inside which the position follows the argmax (both >= 1) */
    int32_t end;               /* 3: the text counts as spoken once pos >= S - end (>= 0) */
    int32_t skip;              /* 5: repetition looks at the columns [0, S - skip) (>= 0); texts of S <= skip ids are never suppressed */
    float tail_thr, rep_thr;   /* 5.0, 5.0 (finite, >= 0) */
    int32_t tok_rep;           /* 3: this many equal ids in a row force the stop; 0 = off (0..16) */
} T3GuardParams;
typedef struct { int32_t pos, complete, completed_at, forced_at, reason; float tail[3]; float rep; } T3GuardState;
/* Non-NULL: allocates the per-slot state and control words and enables the guard with these parameters (again: replaces them).  NULL: frees
 * them and disables it.  Valid only while nothing is queued or running (T3_E_STATE); a parameter out of range is T3_E_INVALID.  Drops the captured
 * step graphs, as t3_set_alignment_heads does.  A request with alignment = 2 is T3_E_STATE while the guard is disabled and T3_E_INVALID with
 * stop_token outside [0, 8194) or ignore_eos = 1.  With no such request in a step, the step launches what it launches with the guard disabled. */
int t3_set_alignment_guard(T3Handle h, const T3GuardParams* params);
/* The final guard state of a FINISHED, not yet released request submitted with alignment = 2.  Error codes as t3_get_alignment. */
int t3_get_guard(T3Handle h, int64_t req_id, T3GuardState* out);

/* ---- per-token log-probabilities -----------------------------------------------------------------------------------------
 * vLLM's SamplingParams(logprobs=k), from a kernel directly behind the sampler (t3_logprobs.hip): the post-CFG logits live on the device for one
 * step only, so nothing outside the engine can compute these.  For a marked request and every token it draws, over the 8194 speech ids v:
 *   x_v    = the post-CFG logit as the sampler forms it, BEFORE penalties, temperature, min-p / top-k / top-p and the guard's suppression (what
 *            t3_debug_logits reports): vLLM's default "raw" log-probabilities.  A guard-forced stop id reports its raw value like any other id;
 *   lp_v   = (x_v - M) - logf(Z),  M = max_v x_v,  Z = sum_v exp(x_v - M) in fp32 in one fixed order;
 *   rank   = #{v : x_v >= x_tok}  (vLLM's definition: ties count);
 *   top[i] = the ids ordered by (x_v descending, v ascending), i < k, decided on the exact fp32 logits.
 * The numbers of a request are bit-identical between eager steps, captured graphs, bursts and batch compositions; token ids never depend on the
 * feature, bursts and run-ahead stay on, and a step that samples no marked request launches exactly what it launches without it.
 * t3_reserve_logprobs: max_k in 0..T3_MAX_LOGPROBS allocates the per-slot records, max_seqs x max_model_len x 2 (max_k + 1) 32-bit words, and the
 * per-slot k words; max_k < 0 frees them; max_k > T3_MAX_LOGPROBS is T3_E_INVALID; T3_E_NOMEM names the byte count.  Valid only while nothing is
 * queued or running (T3_E_STATE).  Drops the captured step graphs, as t3_reserve_alignment does.  The records of finished requests live in pooled
 * buffers that t3_release_request gives back for reuse. */
#define T3_MAX_LOGPROBS 20          /* vLLM's default max_logprobs */
int t3_reserve_logprobs(T3Handle h, int32_t max_k);
/* Marks a request that is still waiting (between t3_add_request and the next step call): k = 0 keeps the drawn id's log-probability and rank
 * only.  Unknown id: T3_E_NOTFOUND; before a reserve, or once the request is admitted: T3_E_STATE; k outside [0, max_k]: T3_E_INVALID. */
int t3_request_logprobs(T3Handle h, int64_t req_id, int32_t k);
/* The numbers of a FINISHED, not yet released, marked request.  On entry *n_tokens is the capacity of every array in tokens; on exit *n_tokens (the
 * number of tokens t3_get_output returns) and *k hold the real extents.  lp_tok / rank [n_tokens]; top_ids / top_lp row-major [n_tokens][k],
 * top_ids in OFFSET space (speech id + 2500) like t3_get_output.  All four arrays may be NULL to ask for the extents only (each may be NULL on its
 * own).  Error codes as t3_get_alignment. */
int t3_get_logprobs(T3Handle h, int64_t req_id, float* lp_tok, int32_t* rank, int32_t* top_ids, float* top_lp, int32_t* n_tokens, int32_t* k);
/* ---- processed log-probabilities: the distribution the sampler draws from -----------------------------------------------------
 * Mode 1 of t3_set_logprobs_mode.  The raw numbers above stand in front of everything the sampler kernel does to a logit; with the reference defaults
 * (repetition_penalty 2.0, temperature 0.8) they differ from what is drawn from by whole nats on repeated ids.  In processed mode the records of a
 * marked request hold, at step k (the step that draws token k) and over the 8194 speech ids v:
 *   1. x_v = the post-CFG fp32 logit as the sampler forms it (cfg_logit);
 *   2. steps 1-3 of "logit processors" below, if the request carries processors: allow list, ONE fp32 add per biased id, the stop ids at -inf while
 *      k < min_tokens;
 *   3. the guard's SUPPRESS of T3Sampling.stop_token, if the step's control word says so;
 *   4. the penalties, where cnt_v > 0, in the sampler's fp32 operations and order: x > 0 ? x / repetition_penalty : x * repetition_penalty (skipped at
 *      1.0), then x - frequency_penalty * cnt_v, then x - presence_penalty.  cnt_v is the count the step's sampler used for its own draw: the
 *      kernel runs behind it and takes the drawn id's increment back (a stored 65535 counts as saturated before the draw; the engine's counts stay
 *      below 8192, its largest max_model_len);
 *   5. z_v = x_v / T, T = temperature, or 1 where temperature < 1e-5 (greedy), as vLLM substitutes;
 *   6. lp_v = (z_v - M) - logf(Z),  M = max_v z_v,  Z = sum_v exp(z_v - M) in fp32, in the fixed order of the raw kernel;
 *   7. rank = #{v : z_v >= z_tok};
 *   8. top[i] = the ids ordered by (z_v descending, v ascending), decided on the exact fp32 z.
 * Ids at -inf have lp = -inf and enter the top list only when no finite id is left.  A guard-FORCEd stop id reports its z like any other id: -inf if
 * the processors had masked it.  min-p, top-k and top-p are NOT applied.  This is the project's own definition: vLLM is not part of the reference
 * tree and its versions disagree on where "processed" is captured.  With top_p = 1, top_k = 0, min_p = 0 it is exactly the distribution of the draw.
 * Token ids never depend on the mode; in mode 0 every record is what it was before the mode existed, and a step that samples no marked request
 * launches exactly what it launches without the feature.  The records keep the raw kernel's guarantees: bit-identical between eager steps, captured
 * graphs, bursts and batch compositions.
 * t3_set_logprobs_mode: mode 0 = raw (the default), 1 = processed; any other value is T3_E_INVALID.  Valid only while nothing is queued or running
 * (T3_E_STATE).  Drops the captured step graphs.  The mode holds for every request marked from then on. */
int t3_set_logprobs_mode(T3Handle h, int32_t mode);

/* ---- logit processors -------------------------------------------------------------------------------------------------------
 * vLLM's SamplingParams(allowed_token_ids=, logit_bias=, bad_words= (single ids), min_tokens=, stop_token_ids=) inside the sampler kernel: the
 * post-CFG logits exist on the device only, for one step, and a burst replays four steps with no host in between.  For a marked request at step k
 * (the step that draws token k), x_v = the post-CFG fp32 logit as the sampler forms it (cfg_logit).  In this order, in front of the guard's
 * suppression, the penalties, temperature, min-p, top-k and top-p:
 *   1. allowed_ids given and v not among them:  x_v = -inf;
 *   2. x_v = x_v + b_v for every (v, b_v) of the bias list: ONE fp32 add per listed id, none for the others.  b_v = -inf is allowed (bad_words);
 *   3. k < min_tokens:  x_s = -inf for every stop id s of the request;
 *   4. the guard's SUPPRESS applies as before; its FORCE draws T3Sampling.stop_token whatever the logits hold.
 * vLLM is not part of the reference tree: like the sampler's masks, this order is this project's restatement of vLLM 0.10's (allowed ids and bias
 * and min_tokens are its logits processors, which run in front of its penalties) and is not pinned by the reference.
 * Stop ids: T3Sampling.stop_token (when >= 0) and up to 3 extra ones.  The request finishes with reason 1 when it draws ANY of them; the guard forces
 * and suppresses the first only.  Raw log-probabilities, t3_debug_logits and the alignment export are defined in front of steps 1-3 and do not change.
 * A row whose every id ends at -inf draws the lowest id of the allow list (the lowest id, 0, without a list; id 0 too when the list is empty),
 * sampled or greedy alike; NaN decides nothing.
 * A step that samples no marked request launches exactly what it launches without the feature; an unmarked request's ids do not depend on it, and a
 * marked request's ids are bit-identical between eager steps, captured graphs, bursts and batch compositions. */
#define T3_MAX_LOGIT_BIAS 64
typedef struct {
    int32_t struct_size;           /* sizeof(T3LogitProcessors) */
    int32_t n_allowed;             /* 0..8194 entries of allowed_ids (ignored when that is NULL) */
    const int32_t* allowed_ids;    /* SPEECH-space, any order, duplicates allowed; NULL = every id */
    const int32_t* bias_ids;       /* SPEECH-space, any order, no duplicates */
    const float* bias_vals;        /* finite or -inf */
    int32_t n_bias;                /* 0..T3_MAX_LOGIT_BIAS */
    int32_t min_tokens;            /* >= 0 */
    int32_t extra_stop_ids[3];     /* SPEECH-space */
    int32_t n_extra_stop;          /* 0..3 */
} T3LogitProcessors;
/* on != 0 allocates the per-slot records (1600 bytes each) and the pinned staging area, 0 frees them.  Valid only while nothing is queued or
 * running (T3_E_STATE).  Drops the captured step graphs. */
int t3_reserve_logit_processors(T3Handle h, int32_t on);
/* Marks a request that is still waiting (between t3_add_request and the next step call).  Unknown id: T3_E_NOTFOUND; before a reserve, or once the
 * request is admitted: T3_E_STATE; T3_E_INVALID for a wrong struct_size, an id outside [0, 8194), n_allowed outside [0, 8194], n_bias outside
 * [0, 64], a bias id listed twice, a bias that is NaN or +inf, min_tokens < 0 or n_extra_stop outside [0, 3].  What is well-formed is accepted: a
 * stop id outside the allow list, or a min_tokens beyond max_tokens, only means that the request ends at its length limit. */
int t3_request_logit_processors(T3Handle h, int64_t req_id, const T3LogitProcessors* p);

/* ---- parity / measurement hooks --------------------------------------------------------- */
/* post-CFG logits [8194] (speech-space, before the 2500-wide -inf pad of t3.py:669-672) of the
 * most recent sampled step of req_id; needs cfg.debug_logits = 1. */
int t3_debug_logits(T3Handle h, int64_t req_id, float* out_8194);
/* The embedded input rows of the most recent step -- what get_input_embeddings (t3.py:424-647) hands to the Llama blocks: cond /
 * text + position / zero / speech + position rows, bf16 [rows][1024] -- with every row's stream (2 * slot for the conditional
 * half, 2 * slot + 1 for the unconditional half of the reference's [N, 2048] layout) and position; needs cfg.debug_logits = 1.
 * On entry *n = capacity in rows (out_bf16 / row_stream / row_pos may be NULL); on exit *n = rows of the step. */
int t3_debug_embeddings(T3Handle h, void* out_bf16, int32_t* row_stream, int32_t* row_pos, int32_t* n);
/* Durations (ms) of the most recent steps since t3_reset_stats, oldest first (at most cap, at most the last 16 384): the time each step
 * had the GPU to itself, i.e. from the completion of the step before it (or its own enqueue, if later) to its own completion as the host
 * sees it (the same clock gpu_ms_total sums).  rows (nullable): the step's row count, negative when it carried prefill rows.
 * Returns the number written.  For the p50 / p90 / p99 step latency SURVEY.md 8(d) asks for. */
int t3_step_times(T3Handle h, float* ms, int32_t* rows, int32_t cap);
int t3_stats(T3Handle h, T3Stats* out);
int t3_reset_stats(T3Handle h);
/* Average duration (ms) per launch of each kernel class over decode-only steps since the last reset,
 * measured with HIP events on the engine's stream when profiling is on (t3_set_profile).
 * names: "gemm_qkv","gemm_o","gemm_gateup","gemm_down","gemm_head","attention","rope_kv","embed","sampler".
 * Single-kernel launches (the decode GEMM forms, the fused / per-row attention, embed, sampler) are timed by the dispatch's own start / stop
 * events (what rocprofv3 reports); launchers that issue several kernels (prefill-sized GEMMs with their row-statistic pass, the tile attention
 * with its per-row head, rope_kv) are bracketed by two event records, ~2-3 us more per launch.  Only decode-only steps are accumulated, where every
 * class is of the first kind. */
int t3_set_profile(T3Handle h, int32_t on);
/* Restrict the events to ONE kernel class (name as above; NULL or "" = every class): the other launches of the step then run
 * undisturbed, so the class's average duration is not inflated by its neighbours' event packets. */
int t3_set_profile_kernel(T3Handle h, const char* name);
int t3_kernel_ms(T3Handle h, const char* name, double* avg_ms, int64_t* launches);

/* ---- conditioning encoder --------------------------------------------------
 * Replaces the reference's torch module `T3CondEnc` (models/t3/modules/cond_enc.py:57-123 with modules/perceiver.py:118-215),
 * as ChatterboxTTS uses it: `self.t3_cond_enc(T3Cond(speaker_emb, cond_prompt_speech_tokens, cond_prompt_speech_emb,
 * emotion_adv))` (tts.py:279-284) and `self.t3_cond_enc.emotion_adv_fc(exaggeration)` (tts.py:287-298).  fp32, on the device;
 * a handle of its own because the reference keeps this module outside the vLLM engine.  No CPU fallback.            */
typedef struct T3CondEncoder* T3CondHandle;
int t3_cond_create(int32_t device_id, T3CondHandle* out);
int t3_cond_destroy(T3CondHandle c);
const char* t3_cond_last_error(T3CondHandle c);          /* c may be NULL after a failed create */
/* fp32 parameters under their checkpoint names, with or without the "cond_enc." prefix (state_dict of T3CondEnc):
 * spkr_enc.{weight [1024][256], bias}, emotion_adv_fc.weight [1024][1], perceiver.pre_attention_query [1][32][1024],
 * perceiver.attn.norm.{weight,bias}, perceiver.attn.{to_q,to_k,to_v,proj_out}.{weight [1024][1024], bias}.
 * Other names return T3_E_NOTFOUND. */
int t3_cond_load_tensor(T3CondHandle c, const char* name, const float* data, int64_t numel);
/* T3CondEnc.forward: speaker_emb [256], cond_prompt_speech_emb [n][1024] (= speech_emb(tokens) + speech_pos_emb(tokens),
 * tts.py:277; 1 <= n <= 192, the reference uses 150), emotion_adv scalar -> out [34][1024] = [speaker; 32 perceiver rows; emotion]. */
int t3_cond_encode(T3CondHandle c, const float* speaker_emb, const float* prompt_emb, int32_t n, float emotion_adv, float* out);
/* emotion_adv_fc(exaggeration) -> out [1024] (the row ChatterboxTTS.update_exaggeration writes into cond_emb[-1]) */
int t3_cond_emotion_row(T3CondHandle c, float exaggeration, float* out);
/* kernel-level entry points of the encoder (host buffers), for the parity tests */
int t3k_ce_layernorm(const float* x /*[rows][1024]*/, const float* w, const float* b, float* y, int32_t rows);
int t3k_ce_linear(const float* x /*[M][K]*/, const float* W /*[N][K]*/, const float* bias /*nullable*/, const float* resid /*nullable [M][N]*/,
                  float* out /*[M][N]*/, int32_t M, int32_t K /*multiple of 32*/, int32_t N);
int t3k_ce_attention(const float* q /*[nq][1024]*/, const float* k /*[nk][1024]*/, const float* v, float* out /*[nq][1024]*/, int32_t nq, int32_t nk);

/* ---- kernel-level entry points (host buffers in, host buffers out; used by the parity tests) ----
 * Each runs exactly the kernel the engine uses, on the current device, and waits for it.
 * t3k_gemm: the engine's K only -- 1024 with 4 segments; 1024 or 4096 with 16 (N a multiple of 16 there); anything else is T3_E_INVALID. */
int t3k_gemm(const void* x_bf16 /*[M][K]*/, const void* w_bf16 /*[N][K]*/, int32_t M, int32_t K, int32_t N,
             float* out_f32 /*[M][N]*/, int32_t mt /*0 = auto*/, int32_t nw /*K segments: 4, or 16 = o_proj/down_proj form*/);
/* RMSNorm folded into the projection (qkv / gate-up / speech-head form): out[r] = rstd * GEMM(bf16(h[row_index[r]] * ln_w), W);
 * h [Mh][1024] bf16, row_index nullable (then M == Mh). */
int t3k_norm_gemm(const void* h_bf16, const void* ln_w_bf16, const void* w_bf16 /*[N][1024]*/, int32_t M, int32_t N,
                  float* out_f32, const int32_t* row_index, int32_t Mh);
/* the qkv projection as a step launches it (input RMSNorm folded): w [3072][1024] (q, k, v rows), out bf16 [M][3072] */
int t3k_qkv_gemm(const void* h_bf16, const void* ln_w_bf16, const void* w_bf16, int32_t M, void* out_bf16);
/* the speech head as a decode step launches it (final RMSNorm folded, rows gathered through row_index [M] into h [Mh][1024], t3.py:650-673
 * before the CFG): out bf16 [M][8208], columns >= 8194 unspecified */
int t3k_head_gemm(const void* h_bf16, const void* ln_w_bf16, const void* w_bf16 /*[8194][1024]*/, int32_t M, const int32_t* row_index, int32_t Mh, void* out_bf16);
/* residual epilogue (o_proj / down_proj form, 16 K-segments): h [M][N] bf16 updated in place, h = bf16(h + bf16(x W^T)) */
int t3k_gemm_resid(const void* x_bf16, const void* w_bf16, int32_t M, int32_t K, int32_t N, void* h_bf16);
/* gate/up form with folded RMSNorm and SiLU*mul epilogue */
int t3k_silu_mul_gemm(const void* h_bf16 /*[M][1024]*/, const void* ln_w_bf16, const void* wg_bf16 /*[F][1024]*/, const void* wu_bf16,
                      int32_t M, int32_t F, void* out_bf16 /*[M][F]*/);
/* RoPE + paged-KV write + paged attention for `rows` rows of ONE layer over a scratch pool:
 * qkv [rows][3072] bf16 (pre-RoPE), row_stream/row_pos int32 [rows]; rows are processed in the given
 * order in ONE launch sequence (all KV writes, then all attention), so rows of the same stream must
 * cover a prefix of positions.  out [rows][1024] bf16.                                        */
int t3k_rope_attention(const void* qkv_bf16, const int32_t* row_stream, const int32_t* row_pos, int32_t rows,
                       int32_t n_streams, int32_t max_pos, void* out_bf16);
/* The FUSED decode attention as a decode step launches it (RoPE of q / k + paged write of the newest K / V + attention over the
 * paged context in ONE kernel; what vLLM's rotary_embedding + reshape_and_cache + paged attention do per layer behind
 * t3.py:703-708), `steps` consecutive launches of `rows` rows over a scrambled scratch pool:
 *   stream r (= row r) holds ctx[r] - 1 context tokens, pre-RoPE qkv rows ctx_qkv[r % n_content][0 .. ctx[r] - 2] ([n_content][content_rows][3072]
 *   bf16), written through the prefill path; launch s takes new_qkv[s][r] ([steps][rows][3072]) at position ctx[r] - 1 + s, so launch
 *   s >= 1 reads what launch s - 1 wrote.  waves: 0 = as the engine picks (8 up to 8 rows, else 4), or 4 / 8.
 * out bf16 [steps][rows][1024]; kv_new (nullable) bf16 [steps][rows][2][1024] = K (rotated) and V of the written positions, read back. */
int t3k_decode_attention(const void* ctx_qkv_bf16, int32_t n_content, int32_t content_rows, const void* new_qkv_bf16, const int32_t* ctx,
                         int32_t rows, int32_t steps, int32_t max_pos, int32_t waves, void* out_bf16, void* kv_new_bf16);
/* CFG + sampler: logits bf16 [2][ldl] (cond row, uncond row), counts uint16 [8194] (updated). */
int t3k_sample(const void* logits2_bf16, int32_t ldl, uint16_t* counts, const T3Sampling* sp, float cfg,
               uint32_t step, int32_t* token_out, float* logits_out_8194 /*nullable*/);
/* t3k_sample plus the SUPPORT of its draw: keep_out [8194] = 1 where penalties -> /T -> min-p -> top-k -> top-p leave the id drawable
 * (greedy: the one id).  Parity hook of the randomized mask test (tests/vllm_masks.py). */
int t3k_sample_support(const void* logits2_bf16, int32_t ldl, uint16_t* counts, const T3Sampling* sp, float cfg,
                       uint32_t step, int32_t* token_out, uint8_t* keep_out_8194);
int t3k_expf(const float* x, float* y, int32_t n);
/* t3k_sample under a guard control word (0 nothing, 1 suppress sp->stop_token, 2 force it): the sampler's guarded instantiation. */
int t3k_sample_ctl(const void* logits2_bf16, int32_t ldl, uint16_t* counts, const T3Sampling* sp, float cfg,
                   uint32_t step, int32_t ctl, int32_t* token_out, float* logits_out_8194 /*nullable*/);
/* t3k_sample_support under logit processors: the build kernel makes the record from *lp (checked as t3_request_logit_processors checks it), then the
 * sampler's third instantiation draws token `step` (the k of the contract).  logits_out_8194 (nullable) = the logits behind step 3 of the contract,
 * in front of the penalties; keep_out_8194 (nullable) = the support of the draw. */
int t3k_sample_proc(const void* logits2_bf16, int32_t ldl, uint16_t* counts, const T3Sampling* sp, float cfg, uint32_t step,
                    const T3LogitProcessors* lp, int32_t* token_out, float* logits_out_8194, uint8_t* keep_out_8194);
/* The guard kernel (t3_guard.hip) over a host matrix A [n_frames][ld] (ld a multiple of 4, >= n_text; the columns from n_text on are never read
 * into a result) and the ids tok [n_frames] drawn at each frame: one launch per frame in frame order, as the engine's steps do it.
 * ctl_out [n_frames] = the control word of each frame, *final_state = the state behind the last one. */
int t3k_alignment_guard(const float* A, int32_t n_frames, int32_t n_text, int32_t ld, const int32_t* tok, const T3GuardParams* params,
                        int32_t* ctl_out, T3GuardState* final_state);
/* The path kernel of t3_get_token_spans on one host matrix A [n_frames][ld] (n_frames <= 8192, n_text <= 2112, ld >= n_text; the columns from n_text
 * on are never read into a result): path [n_frames], start / end [n_text], *last, *score. */
int t3k_align_path(const float* A, int32_t n_frames, int32_t n_text, int32_t ld, int32_t* path, int32_t* start, int32_t* end, int32_t* last,
                   int32_t* score);
/* Its cell score alone: w[i] = rint(1024 log2 a'[i]), |w| <= 65536. */
int t3k_align_scores(const float* a, int32_t* w, int32_t n);
/* The log-probability kernel (t3_logprobs.hip) for one utterance on host buffers: logits bf16 [2][ldl] as t3k_sample takes them (ldl a multiple of
 * 8), token = the drawn speech-space id, k in 0..T3_MAX_LOGPROBS.  top_ids (SPEECH-space) / top_lp [k], nullable when k = 0. */
int t3k_logprobs(const void* logits2_bf16, int32_t ldl, float cfg, int32_t token, int32_t k, int32_t* rank, float* lp_tok,
                 int32_t* top_ids, float* top_lp);
/* Its processed instantiation for one utterance at step `step` (< 8192).  counts uint16 [8194] = the counts the step's sampler USED for its draw (the
 * hook raises the drawn id's count on its device copy, as the sampler leaves it in the engine); lp nullable = no processors, else checked as
 * t3_request_logit_processors checks it; ctl = -1 no control word, 0 / 1 / 2 = the guard's word for a slot marked guarded (as t3k_sample_ctl). */
int t3k_logprobs_processed(const void* logits2_bf16, int32_t ldl, float cfg, const uint16_t* counts, const T3Sampling* sp, const T3LogitProcessors* lp,
                           int32_t ctl, uint32_t step, int32_t token, int32_t k, int32_t* rank, float* lp_tok, int32_t* top_ids, float* top_lp);
/* ---- the FP8 (E4M3FN) KV pool, kv_cache_dtype = 1 ----
 * y = dequantised q8(x) on the device, q8(x) = e4m3fn(round-to-nearest-even(clamp(x, -448, 448))): the stored format of the FP8 pool. */
int t3k_fp8_roundtrip(const float* x, float* y, int32_t n);
/* t3k_rope_attention over an FP8 pool; kv_bf16 (nullable) [rows][2][1024] = the stored K (rotated) and V of every row's position, dequantised. */
int t3k_rope_attention_fp8(const void* qkv_bf16, const int32_t* row_stream, const int32_t* row_pos, int32_t rows,
                           int32_t n_streams, int32_t max_pos, void* out_bf16, void* kv_bf16);
/* t3k_decode_attention over an FP8 pool: same arguments and meaning, kv_new read back dequantised. */
int t3k_decode_attention_fp8(const void* ctx_qkv_bf16, int32_t n_content, int32_t content_rows, const void* new_qkv_bf16, const int32_t* ctx,
                             int32_t rows, int32_t steps, int32_t max_pos, int32_t waves, void* out_bf16, void* kv_new_bf16);
/* ---- the MXFP4 KV pool, kv_cache_dtype = 4 ----
 * y = the stored value of x on the device, over blocks of 32 consecutive values (n a multiple of 32): with E the biased exponent field of the
 * block's max |x|, b = max(E - 2, 0) and X = 2^(b - 127), y = X * E2M1(round-to-nearest-even(x / X)), saturating at +-6. */
int t3k_fp4_roundtrip(const float* x, float* y, int32_t n);
/* t3k_rope_attention / t3k_decode_attention over an MXFP4 pool: the arguments and meaning of the FP8 pair above. */
int t3k_rope_attention_fp4(const void* qkv_bf16, const int32_t* row_stream, const int32_t* row_pos, int32_t rows,
                           int32_t n_streams, int32_t max_pos, void* out_bf16, void* kv_bf16);
int t3k_decode_attention_fp4(const void* ctx_qkv_bf16, int32_t n_content, int32_t content_rows, const void* new_qkv_bf16, const int32_t* ctx,
                             int32_t rows, int32_t steps, int32_t max_pos, int32_t waves, void* out_bf16, void* kv_new_bf16);
/* ---- MXFP8 weights for the four layer projections (qkv, o, gate/up, down), t3_set_weight_dtype = 1 ----
 * Storage format of t3_finalize_weights, applied behind the RMSNorm fold: blocks of 32 consecutive k of one output row; with E the biased exponent
 * field of the block's max |w|, b = max(E - 8, 0) is the block's E8M0 scale byte, X = 2^(b - 127), an element is q8(w / X) (q8 as above) and the
 * stored value is X * element: 8.25 bits per weight.  Every stored value of a block in bf16's normal range is a bf16 value, and the kernels
 * (t3_gemm_mx8.hip) rebuild it exactly in front of the bf16 matrix instruction, so a step computes bit for bit what the bf16 engine computes over
 * the stored values.  The speech head, the embeddings and the position tables stay bf16.  Audio quality under this format has NOT been
 * validated on a real checkpoint.
 * dtype: 0 = bf16 (default), 1 = MXFP8, anything else T3_E_INVALID; T3_E_STATE after t3_finalize_weights. */
int t3_set_weight_dtype(T3Handle h, int32_t dtype);
/* y = the stored value of w: the finalize quantiser and its inverse, on the host.  w, y bf16 [rows][cols], cols a multiple of 32. */
int t3k_mxfp8_roundtrip(const void* w_bf16, void* y_bf16, int32_t rows, int32_t cols);
/* t3k_qkv_gemm / t3k_gemm_resid (K = 1024 or 4096) / t3k_silu_mul_gemm over MXFP8 weights: the same arguments; each takes bf16 weights, folds the norm
 * weight where its twin does, quantises as t3_finalize_weights does and runs the kernel a step runs. */
int t3k_qkv_gemm_mx8(const void* h_bf16, const void* ln_w_bf16, const void* w_bf16, int32_t M, void* out_bf16);
int t3k_gemm_resid_mx8(const void* x_bf16, const void* w_bf16, int32_t M, int32_t K, int32_t N, void* h_bf16);
int t3k_silu_mul_gemm_mx8(const void* h_bf16 /*[M][1024]*/, const void* ln_w_bf16, const void* wg_bf16 /*[F][1024]*/, const void* wu_bf16,
                          int32_t M, int32_t F, void* out_bf16 /*[M][F]*/);
/* The alignment tap kernel (t3_alignment.hip) on host buffers.  Every row is written through the prefill path (RoPE + paged write, as
 * t3k_rope_attention / t3k_rope_attention_fp8 / _fp4 do; kv_dtype 0 = bf16 pool, 1 = FP8, 4 = MXFP4), then the tap runs for EVERY row over the span [lo, hi) of
 * its stream: out [rows][hi - lo] = softmax over the row's context 0 .. row_pos of head `head`; positions at or beyond the row's own context
 * length come back as 0.  q_rot (nullable) bf16 [rows][64] = the rotated q the tap used; kv (nullable) bf16 [rows][2][1024] = the stored K / V
 * of every row's position (dequantised for the FP8 pool). */
int t3k_attention_probs(const void* qkv_bf16, const int32_t* row_stream, const int32_t* row_pos, int32_t rows, int32_t n_streams, int32_t max_pos,
                        int32_t head, int32_t lo, int32_t hi, int32_t kv_dtype, float* out_f32, void* q_rot_bf16, void* kv_bf16);
/* the hand-off kernel on host buffers (one utterance): out [ld] padded with 0, *len = kept tokens */
int t3k_handoff(const int32_t* speech_ids, int32_t n, int32_t text_token_count, int32_t flags, int32_t* out, int32_t ld, int32_t* len);
/* Row count from which the GEMM launcher switches to its prefill schedule (same numbers, LDS-tiled); process-wide.
 * < 0 restores the default (per form, 448-1600 rows).  For the parity tests, which check the prefill schedule at small row counts. */
int t3k_set_prefill_rows(int32_t rows);
/* Row count from which the 4-segment forms of that schedule take 128 x 128 workgroup tiles instead of 128 x 64 (0 = never,
 * < 0 = default 2048).  Same purpose. */
int t3k_set_prefill_wide_rows(int32_t rows);

#ifdef __cplusplus
}
#endif
#endif /* T3_ENGINE_H */
