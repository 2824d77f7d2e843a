"""vLLM-shaped surface of the T3 engine: ``LLM`` / ``SamplingParams`` / ``RequestOutput``.

Drop-in for what src/chatterbox_vllm/tts.py uses of vLLM (reference lines):
  * construction  ``LLM(model=dir, task="generate", tokenizer="EnTokenizer"|"MtlTokenizer",
                        tokenizer_mode="custom", gpu_memory_utilization=f, enforce_eager=b,
                        max_model_len=n, **kwargs)``                              tts.py:150-171
  * generation    ``llm.generate([{"prompt": str, "multi_modal_data": {"conditionals": [Tensor[34,1024]]}}, ...],
                                 sampling_params=SamplingParams(temperature=, stop_token_ids=[9062],
                                 max_tokens=, top_p=, repetition_penalty=, **kw))``        tts.py:445-465
  * results       ``for r in results: for o in r.outputs: o.token_ids``  (ids >= 2500)     tts.py:474-492
Errors: bad input -> ValueError (HTTP 400 in api_server.py:323-326), anything else -> RuntimeError (500).
"""
from __future__ import annotations

import os
import warnings
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from . import constants as C
from .engine import LOGPROBS_MODES, MAX_LOGIT_BIAS, T3Engine, kv_cache_dtype_code, weight_dtype_code, make_guard_params, make_logit_processors, make_sampling
from .prompt import TextTokenizer, assemble_prompt_ids, find_tokenizer_file
from .weights import iter_safetensors, synthetic_tensors


MAX_LOGPROBS = 20      # vLLM's default max_logprobs; T3_MAX_LOGPROBS of include/t3_engine.h


@dataclass
class Logprob:
    """vLLM's Logprob: the log-probability of an id (raw or processed: LLM(logprobs_mode=...)), its rank among the 8194 speech ids (1 = most likely; ties count for the drawn id)."""
    logprob: float
    rank: Optional[int] = None
    decoded_token: Optional[str] = None


class SamplingParams:
    """The subset of vllm.SamplingParams that reaches the sampler on this path (tts.py:455-464),
    with vLLM's names and defaults.  Unknown keyword arguments are rejected like vLLM does."""

    _IGNORED = {"prompt_logprobs", "detokenize", "skip_special_tokens", "spaces_between_special_tokens",
                "include_stop_str_in_output", "output_kind", "stop",
                "truncate_prompt_tokens", "guided_decoding", "extra_args", "best_of", "logits_processors"}

    def __init__(self, n: int = 1, temperature: float = 1.0, top_p: float = 1.0, top_k: int = 0, min_p: float = 0.0,
                 repetition_penalty: float = 1.0, presence_penalty: float = 0.0, frequency_penalty: float = 0.0,
                 seed: Optional[int] = None, stop_token_ids: Optional[List[int]] = None, max_tokens: Optional[int] = 16,
                 ignore_eos: bool = False, pos_policy: int = 0, alignment: bool = False,
                 alignment_guard: Union[bool, dict, None] = False, logprobs: Optional[int] = None, timestamps: bool = False,
                 logit_bias: Optional[Dict[int, float]] = None, allowed_token_ids: Optional[List[int]] = None,
                 bad_words: Optional[list] = None, min_tokens: int = 0, **kwargs):
        for k, v in kwargs.items():
            if k not in self._IGNORED:
                raise TypeError(f"SamplingParams got an unexpected keyword argument {k!r}")
            if v not in (None, 0, False, [], {}, True) and k not in ("detokenize", "skip_special_tokens"):
                warnings.warn(f"SamplingParams.{k} is not supported on the T3 path and is ignored")
        if n != 1:
            raise ValueError("n must be 1 on the T3 path")
        if temperature < 0:
            raise ValueError(f"temperature must be non-negative, got {temperature}")
        if not 0 < top_p <= 1:
            raise ValueError(f"top_p must be in (0, 1], got {top_p}")
        if top_k < -1:
            raise ValueError(f"top_k must be -1/0 (disable) or positive, got {top_k}")
        if not 0 <= min_p <= 1:
            raise ValueError(f"min_p must be in [0, 1], got {min_p}")
        if not 0 < repetition_penalty <= 2 + 1e-6 and repetition_penalty <= 0:
            raise ValueError(f"repetition_penalty must be positive, got {repetition_penalty}")
        if max_tokens is not None and max_tokens < 1:
            raise ValueError(f"max_tokens must be at least 1, got {max_tokens}")
        self.n, self.temperature, self.top_p, self.top_k, self.min_p = n, temperature, top_p, top_k, min_p
        self.repetition_penalty, self.presence_penalty, self.frequency_penalty = repetition_penalty, presence_penalty, frequency_penalty
        self.seed, self.stop_token_ids, self.max_tokens, self.ignore_eos = seed, list(stop_token_ids or []), max_tokens, ignore_eos
        self.pos_policy = pos_policy
        # vLLM's logits processors, run inside the sampler kernel (csrc/t3_logitproc.hip; include/t3_engine.h "logit processors" has the order).
        # Every id is in OFFSET space (speech id + 2500), as stop_token_ids and the output ids are.  logit_bias values are passed on as given:
        # vLLM 0.10 clamps them to [-100, 100] only in SamplingParams.from_optional (its OpenAI server's path), not in the constructor this class
        # stands for.  bad_words has no detokenizer to go through here: an entry is one offset-space id, bare or as a list of one, and becomes a
        # bias of -inf.  At most 64 ids may carry a bias, bad_words included, and at most 4 stop ids end a request.
        lo, hi = C.SPEECH_TOKEN_OFFSET, C.SPEECH_TOKEN_OFFSET + C.SPEECH_VOCAB

        def speech_id(v, what):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"{what}: {v!r} is not a token id")
            if not lo <= int(v) < hi:
                raise ValueError(f"{what}: id {v} is outside the speech range [{lo}, {hi}) -- ids at this surface carry the +{lo} offset")
            return int(v) - lo

        self.logit_bias, self.allowed_token_ids, self.bad_words, self.min_tokens = logit_bias, allowed_token_ids, bad_words, int(min_tokens)
        bias = {}
        for k, v in (logit_bias or {}).items():
            v = float(v)
            if v != v or v == float("inf"):
                raise ValueError(f"logit_bias[{k}] = {v}: a bias must be finite or -inf")
            bias[speech_id(k, "logit_bias")] = v
        for w in bad_words or []:
            if isinstance(w, (list, tuple)):
                if len(w) != 1:
                    raise ValueError(f"bad_words entry {w!r}: only single-token entries are supported (there is no detokenizer on the T3 path)")
                w = w[0]
            if isinstance(w, str):
                raise ValueError(f"bad_words entry {w!r}: give the offset-space token id, there is no detokenizer on the T3 path")
            bias[speech_id(w, "bad_words")] = float("-inf")
        if len(bias) > MAX_LOGIT_BIAS:
            raise ValueError(f"{len(bias)} biased ids (logit_bias and bad_words together): at most {MAX_LOGIT_BIAS}")
        if allowed_token_ids is not None and len(allowed_token_ids) == 0:
            raise ValueError("allowed_token_ids must not be empty")
        allowed = None if allowed_token_ids is None else sorted({speech_id(v, "allowed_token_ids") for v in allowed_token_ids})
        if self.min_tokens < 0:
            raise ValueError(f"min_tokens must be non-negative, got {min_tokens}")
        if max_tokens is not None and self.min_tokens > max_tokens:
            raise ValueError(f"min_tokens must be at most max_tokens = {max_tokens}, got {min_tokens}")
        if len(self.stop_token_ids) > 4:
            raise ValueError(f"at most 4 stop_token_ids, got {len(self.stop_token_ids)}")
        stops = [speech_id(v, "stop_token_ids") for v in self.stop_token_ids]
        # what LLM.generate marks the request with (speech-space), None when there is nothing to do
        self.processors = None
        if bias or allowed is not None or self.min_tokens > 0 or len(stops) > 1:
            self.processors = dict(allowed_ids=allowed, bias=bias, min_tokens=self.min_tokens, extra_stop_ids=stops[1:])
        # vLLM's logprobs: None = off; k in 0..20 = the log-probability and rank of every drawn id plus the k most likely ids per token
        # (CompletionOutput.logprobs / cumulative_logprob), from a kernel behind the sampler (csrc/t3_logprobs.hip).  Which numbers is the engine's
        # LLM(logprobs_mode=...): "raw_logprobs" (vLLM's default: the post-CFG logits -- processors, penalties, temperature and the alignment guard's
        # suppression do not enter) or "processed_logprobs" (what the draw is taken from; top-k / top-p / min-p enter neither).  prompt_logprobs
        # stays ignored.
        if logprobs is not None and not 0 <= int(logprobs) <= MAX_LOGPROBS:
            raise ValueError(f"logprobs must be in [0, {MAX_LOGPROBS}], got {logprobs}")
        self.logprobs = None if logprobs is None else int(logprobs)
        # extension: keep the text-speech alignment matrix of the request (CompletionOutput.alignment) -- what upstream's
        # AlignmentStreamAnalyzer reads from its attention hooks and a vLLM engine cannot hand out
        self.alignment = bool(alignment)
        # extension: the on-device alignment guard (csrc/t3_guard.hip) holds the stop token back until the text is spoken and forces it once
        # the model lingers on, or goes back over, spoken text.  True = the default parameters, a dict overrides some (engine.GUARD_DEFAULTS;
        # not validated against a real checkpoint).  Implies alignment=True; CompletionOutput.guard reports the final state.
        self.alignment_guard = None
        if alignment_guard not in (None, False):
            make_guard_params(alignment_guard)        # ValueError for an unknown name or a wrong type
            if ignore_eos:
                raise ValueError("alignment_guard cannot be combined with ignore_eos: the guard works by drawing the stop token")
            if not stop_token_ids:
                raise ValueError("alignment_guard needs stop_token_ids: the token the guard suppresses or forces")
            self.alignment_guard = dict(alignment_guard) if isinstance(alignment_guard, dict) else {}
            self.alignment = True

        # extension: when each text token is spoken (CompletionOutput.timestamps), from a path search over the alignment matrix on the device
        # (csrc/t3_align_path.hip).  The request runs with the alignment tap on; the matrix itself is fetched only with alignment=True.
        self.timestamps = bool(timestamps)

    def __repr__(self):
        return ("SamplingParams(" + ", ".join(f"{k}={getattr(self, k)!r}" for k in (
            "temperature", "top_p", "top_k", "min_p", "repetition_penalty", "seed", "stop_token_ids", "max_tokens", "ignore_eos")) + ")")


@dataclass
class CompletionOutput:
    index: int
    text: str
    token_ids: List[int]
    cumulative_logprob: Optional[float] = None    # SamplingParams(logprobs=k): the float64 sum of the drawn ids' log-probabilities (in the engine's logprobs_mode), in token order
    logprobs: Optional[List[Dict[int, Logprob]]] = None      # ... and per token {offset-space id: Logprob} for the drawn id and the k most likely ids
    finish_reason: Optional[str] = None
    stop_reason: Union[int, str, None] = None
    alignment: Optional[torch.Tensor] = None      # SamplingParams(alignment=True): CPU float32 [n_tokens, n_text], row k = frame k's attention over the text
    timestamps: Optional[torch.Tensor] = None     # SamplingParams(timestamps=True): CPU int32 [n_text, 2], [start, end) frames of every text id (25 frames / s), -1 = not reached
    guard: Optional[dict] = None                  # SamplingParams(alignment_guard=...): the guard's final state (T3Engine.get_guard); reason None = never forced


@dataclass
class RequestOutput:
    request_id: str
    prompt: Optional[str]
    prompt_token_ids: List[int]
    outputs: List[CompletionOutput]
    finished: bool = True
    metrics: Dict[str, float] = field(default_factory=dict)


PromptType = Union[str, Dict[str, Any]]


class LLM:
    def __init__(self, model: str, task: str = "generate", tokenizer: Optional[str] = None,
                 tokenizer_mode: Optional[str] = None, gpu_memory_utilization: float = 0.9,
                 enforce_eager: bool = True, max_model_len: int = 1000, max_num_seqs: int = 256,
                 max_num_batched_tokens: int = 0, seed: int = 0, load_format: str = "auto", dtype: str = "bfloat16",
                 device_id: Optional[int] = None, tokenizer_file: Optional[str] = None, num_hidden_layers: Optional[int] = None,
                 kv_cache_bytes: int = 0, debug_logits: bool = False, honor_enforce_eager: Optional[bool] = None,
                 kv_cache_dtype: Optional[str] = None, alignment_max_text: int = 0,
                 alignment_guard: Union[bool, dict, None] = None, logprobs_mode: str = "raw_logprobs",
                 quantization: Optional[str] = None, **kwargs):
        if task != "generate":
            raise ValueError("only task='generate' exists on the T3 path")
        # vLLM's logprobs_mode: what SamplingParams(logprobs=k) reports.  "raw_logprobs" (default) or "processed_logprobs" (the distribution the
        # sampler draws from, include/t3_engine.h); vLLM's "raw_logits" / "processed_logits" are not built and, like any other string, a ValueError.
        if logprobs_mode not in LOGPROBS_MODES:
            raise ValueError(f"logprobs_mode {logprobs_mode!r}: the T3 engine builds {sorted(LOGPROBS_MODES)}")
        if dtype not in ("bfloat16", "auto", torch.bfloat16):
            raise ValueError("the T3 engine computes in bf16 storage / fp32 accumulation only")
        # vLLM's switch for the storage format of the KV cache ("auto" / "bfloat16": bf16; "fp8" / "fp8_e4m3": E4M3 with scale 1.0, half
        # the bytes per token; "mxfp4" / "fp4": E2M1 with one power-of-two scale per 32 head dims of a token, 1088 bytes per token and layer
        # against 4096; anything else, "fp8_e5m2" included, is a ValueError).  None: the T3_KV_CACHE_DTYPE environment variable.
        kv_cache_dtype_code(kv_cache_dtype)
        # vLLM's switch for quantised weights.  "mxfp8": the qkv / o / gate-up / down matrices of every layer are quantised to OCP MXFP8 while the
        # checkpoint loads (E4M3 elements, one power-of-two scale per 32 weights of a row: 8.25 bits per weight); the speech head and the embeddings
        # stay bf16.  Audio quality under it has not been validated on a real checkpoint.  None: the T3_WEIGHT_DTYPE environment variable
        # ("bf16" / "mxfp8"), else bf16.  Any other method ("awq", "gptq", "fp8", ...) is not built: a ValueError.
        if quantization is not None and quantization != "mxfp8":
            raise ValueError(f"quantization {quantization!r}: the T3 engine builds 'mxfp8' only (None = bf16 weights)")
        weight_dtype_code(quantization)
        for k in kwargs:
            warnings.warn(f"LLM(...) keyword {k!r} has no meaning for the T3 engine and is ignored")
        self.model_dir = model
        self.tokenizer_kind = tokenizer or "EnTokenizer"
        text_vocab = C.TEXT_VOCAB_EN if self.tokenizer_kind == "EnTokenizer" else C.TEXT_VOCAB_MTL   # t3.py:270
        n_layers = num_hidden_layers or C.N_LAYERS
        self.max_model_len, self.seed = int(max_model_len), int(seed)
        if device_id is None:
            device_id = int(os.environ.get("LOCAL_RANK", "0")) if torch.cuda.device_count() > 1 else 0
        if torch.cuda.is_available():
            torch.cuda.set_device(device_id)      # torch-side work of this process (RCCL collectives of dp.py, hand-off tensors) runs on the engine's GPU
        # enforce_eager: in vLLM it switches off CUDA-graph capture and torch.compile (start-up time and memory knobs; the
        # reference server always passes True, api_server.py:157 -> tts.py:156,163).  Here a decode step is replayed from a
        # hipGraph captured on first use -- no compile step, a few MB -- and token ids do not depend on it, so by default the
        # flag is accepted and NOT applied.  `honor_enforce_eager=True` (a kwarg of this class, forwarded by tts.py:171's **kwargs;
        # default: the T3_HONOR_ENFORCE_EAGER environment variable, else False) makes enforce_eager=True mean launch-by-launch
        # steps, as in vLLM (debugging, profiling: +43 % step time at B = 1).
        if honor_enforce_eager is None:
            honor_enforce_eager = os.environ.get("T3_HONOR_ENFORCE_EAGER", "0") == "1"
        self.honor_enforce_eager = bool(honor_enforce_eager)
        eager = bool(enforce_eager) and self.honor_enforce_eager
        self.engine = T3Engine(n_layers=n_layers, text_vocab=text_vocab, max_model_len=max_model_len, max_seqs=max_num_seqs,
                               device_id=device_id, kv_bytes=kv_cache_bytes, gpu_memory_utilization=gpu_memory_utilization,
                               enforce_eager=eager, debug_logits=debug_logits, max_batched_rows=max_num_batched_tokens,
                               kv_cache_dtype=kv_cache_dtype, weight_dtype=quantization)
        ckpt = os.path.join(model, "model.safetensors") if model and os.path.isdir(model) else model
        if load_format == "dummy" or not (ckpt and os.path.exists(ckpt)):
            if load_format != "dummy":
                raise ValueError(f"no checkpoint at {ckpt!r}: pass load_format='dummy' for seeded synthetic weights")
            self.engine.load_tensors(synthetic_tensors(n_layers, text_vocab, seed=1234))
        else:
            self.engine.load_tensors(iter_safetensors(ckpt))
        self.engine.finalize()
        # alignment export: frame buffers for texts of up to alignment_max_text ids are made now; 0 = the first generate() with a tapped
        # request reserves for the longest text of that call
        if alignment_max_text > 0:
            self.engine.reserve_alignment(alignment_max_text)
        # alignment guard: enabled now with these parameters (True = defaults); None = the first generate() with a guarded request enables it
        # with that call's parameters
        if alignment_guard not in (None, False):
            self.engine.set_alignment_guard(alignment_guard)
        if logprobs_mode != "raw_logprobs":
            self.engine.set_logprobs_mode(logprobs_mode)
        tf = find_tokenizer_file(self.tokenizer_kind, model if model and os.path.isdir(model) else None, tokenizer_file)
        self.tokenizer = TextTokenizer(self.tokenizer_kind, tf) if tf else None
        self._next_id = 0
        self._next_uid = 0            # RNG stream of the next unseeded request (see generate)

    # -- vLLM API -------------------------------------------------------------------------------
    def get_tokenizer(self):
        return self.tokenizer

    def _text_ids(self, p: PromptType) -> (Optional[str], List[int], torch.Tensor):
        if isinstance(p, str):
            raise ValueError("T3 prompts need multi_modal_data={'conditionals': [Tensor[34,1024]]} (t3.py:207-210)")
        conds = (p.get("multi_modal_data") or {}).get("conditionals")
        if conds is None or len(conds) != 1:
            raise ValueError("exactly one conditional embedding is required for prefill (t3.py:208-209)")
        cond = conds[0]
        if cond.shape[0] != C.CONDITIONING_SIZE:
            raise ValueError("Conditionals must be CONDITIONING_SIZE tokens long (t3.py:210)")
        if "prompt_token_ids" in p:
            return p.get("prompt"), [int(t) for t in p["prompt_token_ids"]], cond
        if self.tokenizer is None:
            raise ValueError("no tokenizer file found: pass tokenizer_file=... / CHATTERBOX_TOKENIZER_DIR, or give prompt_token_ids")
        return p["prompt"], self.tokenizer.encode(p["prompt"]), cond

    def generate(self, prompts: Union[PromptType, Sequence[PromptType]], sampling_params: Optional[Union[SamplingParams, Sequence[SamplingParams]]] = None,
                 use_tqdm: bool = False, uid_base: Optional[int] = None, uids: Optional[Sequence[int]] = None,
                 keep_for_handoff: bool = False) -> List[RequestOutput]:
        """Randomness (the sampler draws from Philox keyed by (seed, uid, step), include/t3_engine.h):
          * no SamplingParams.seed (what tts.py:455-464 does): every request takes the next RNG stream of this LLM object, so the
            same text submitted twice gives two different utterances, while a fresh process replays the same sequence -- vLLM's
            behaviour with its global `seed=0` default;
          * SamplingParams.seed given: that request is reproducible wherever it sits -- alone, in a batch, in a data-parallel shard
            (vLLM's per-request generator): it draws from (seed, stream 0) whatever uids / uid_base say;
          * uids (one per prompt) or uid_base (request i uses uid_base + i) given -- the data-parallel launcher, dp.py: the stream
            of an UNSEEDED request is the utterance's GLOBAL index, so a sharded run emits the ids of the one-GPU run.
        keep_for_handoff: the requests stay in the engine (finished) until `handoff_tokens(outputs, ...)` hands their ids to the
        vocoder from device memory; without it they are released here, as the reference's flow expects."""
        if isinstance(prompts, (str, dict)):
            prompts = [prompts]
        if sampling_params is None:
            sampling_params = SamplingParams()
        sps = list(sampling_params) if isinstance(sampling_params, (list, tuple)) else [sampling_params] * len(prompts)
        if len(sps) != len(prompts):
            raise ValueError("The lengths of prompts and sampling_params must be the same.")
        if uids is not None and len(uids) != len(prompts):
            raise ValueError("The lengths of prompts and uids must be the same.")
        if uids is None and uid_base is not None:
            uids = [int(uid_base) + i for i in range(len(prompts))]
        metas = []
        queued: List[int] = []
        uid0 = self._next_uid
        # ids stay in device memory for the hand-off only when asked for; free buffers for this call's requests are made now, outside
        # the step loop (requests kept by an earlier call hold theirs until handoff_tokens releases them).  A caller that switched the
        # retention on itself (T3Engine.reserve_handoff) keeps it: this call touches the flag only when it needs it and puts it back.
        kept_before = getattr(self.engine, "keeps_device_ids", False)
        if keep_for_handoff:
            self.engine.reserve_handoff(len(prompts))
        try:
            self._queue(prompts, sps, uids, metas, queued)
        except Exception:
            for rid in queued:             # nothing of this call has run yet: leave the engine as it was found
                self.engine.abort(rid)
            self._next_uid = uid0
            raise
        try:
            self.engine.run_until_done()
        except Exception:
            for rid in queued:             # e.g. a request that can never be admitted (KV pool too small): drop the whole call
                try:
                    self.engine.abort(rid)
                except Exception:
                    pass
            raise
        finally:
            if keep_for_handoff and not kept_before:
                self.engine.reserve_handoff(0)      # finished requests keep the buffers they hold; no new ones are made
        outs = []
        stamped = [m[0] for m in metas if m[6]]
        spans = dict(zip(stamped, self.engine.get_token_spans(stamped)))      # one launch for all of the call's marked requests, before any is released
        for rid, text, final, tap, guarded, want_lp, _ in metas:
            toks, fr = self.engine.get_output(rid)
            align = self.engine.get_alignment(rid) if tap else None
            guard = self.engine.get_guard(rid) if guarded else None
            lps = cum = None
            if want_lp:
                lp, rank, ids, tlp = self.engine.get_logprobs(rid)
                lps = []
                for t, tok in enumerate(toks):
                    d = {int(i): Logprob(float(v), n + 1) for n, (i, v) in enumerate(zip(ids[t], tlp[t]))}
                    d[tok] = Logprob(float(lp[t]), int(rank[t]))
                    lps.append(d)
                cum = float(lp.astype("float64").sum())
            if not keep_for_handoff:
                self.engine.release(rid)
            reason = {1: "stop", 2: "length"}.get(fr)
            outs.append(RequestOutput(request_id=str(rid), prompt=text, prompt_token_ids=final,
                                      outputs=[CompletionOutput(index=0, text="", token_ids=toks, finish_reason=reason,
                                                                stop_reason=(toks[-1] if fr == 1 else None), alignment=align, guard=guard,
                                                                timestamps=spans[rid][0] if rid in spans else None,
                                                                logprobs=lps, cumulative_logprob=cum)]))
        return outs

    def handoff_tokens(self, outputs: Sequence[RequestOutput], text_token_counts: Sequence[int], range_filter: bool = True):
        """The T3 -> S3Gen hand-off for a whole batch (replaces the loop of tts.py:483-514): for outputs of
        `generate(..., keep_for_handoff=True)` returns (speech_tokens int32 [n, L], speech_token_lens int32 [n]) CUDA tensors --
        ids already un-offset, cut where the reference's AlignmentStreamAnalyzer would force EOS (text_token_counts as tts.py:496:
        `len(prompt.split()) * 2`), filtered to [0, 6561) -- and releases the requests."""
        rids = [int(o.request_id) for o in outputs]
        try:
            return self.engine.handoff_tokens(rids, text_token_counts, range_filter)
        finally:
            for r in rids:
                try:
                    self.engine.release(r)
                except Exception:
                    pass

    def _queue(self, prompts, sps, uids, metas, queued):
        texts = [self._text_ids(p) for p in prompts]
        tapped = [len(t[1]) for t, sp in zip(texts, sps) if sp.alignment or sp.timestamps]      # text ids per tapped request
        if tapped and max(tapped) > self.engine.alignment_max_text:
            self.engine.reserve_alignment(max(tapped))
        guards = [sp.alignment_guard for sp in sps if sp.alignment_guard is not None]
        if guards:
            if any(g != guards[0] for g in guards):
                raise ValueError("the guarded requests of one generate() call must share their alignment_guard parameters (one set per engine)")
            if self.engine.guard_params is None:
                self.engine.set_alignment_guard(guards[0])       # the first guarded call enables the guard with its parameters
            elif any(self.engine.guard_params[k] != getattr(make_guard_params(guards[0]), k) for k in guards[0]):      # as the C struct rounds them
                raise ValueError(f"alignment_guard {guards[0]} differs from the engine's enabled guard {self.engine.guard_params}")
        asked = [sp.logprobs for sp in sps if sp.logprobs is not None]
        if asked and max(asked) > self.engine.logprobs_max_k:
            self.engine.reserve_logprobs(max(asked))         # once for the call's largest k, before anything of it is queued
        if any(sp.processors for sp in sps) and not self.engine.logit_processors_reserved:
            self.engine.reserve_logit_processors(True)       # on first use, before anything of the call is queued
        for i, ((text, tids, cond), sp) in enumerate(zip(texts, sps)):
            final = assemble_prompt_ids(tids)
            stop = -1
            if sp.stop_token_ids:       # the first is T3Sampling.stop_token (the guard's), the others ride in the request's processors
                stop = int(sp.stop_token_ids[0]) - C.SPEECH_TOKEN_OFFSET          # 9062 -> 6562 (tts.py:458)
            max_tokens = sp.max_tokens if sp.max_tokens is not None else self.max_model_len
            if sp.seed is not None:
                uid = 0                    # a seeded request draws from (seed, 0) wherever it runs: alone, in a batch or in a data-parallel shard
            elif uids is not None:
                uid = int(uids[i])
            else:
                uid = self._next_uid; self._next_uid += 1
            esp = make_sampling(temperature=sp.temperature, top_p=sp.top_p, min_p=sp.min_p, repetition_penalty=sp.repetition_penalty,
                                presence_penalty=sp.presence_penalty, frequency_penalty=sp.frequency_penalty,
                                top_k=max(0, sp.top_k), max_tokens=max_tokens, ignore_eos=sp.ignore_eos, stop_token=stop,
                                seed=self.seed if sp.seed is None else sp.seed, uid=uid, pos_policy=sp.pos_policy, alignment=sp.alignment or sp.timestamps,
                                alignment_guard=sp.alignment_guard is not None)
            rid = self._next_id; self._next_id += 1
            self.engine.add_request(rid, final, cond, esp)
            queued.append(rid)
            if sp.logprobs is not None:
                self.engine.request_logprobs(rid, sp.logprobs)
            if sp.processors:
                self.engine.request_logit_processors(rid, make_logit_processors(**sp.processors))
            metas.append((rid, text, final, sp.alignment, sp.alignment_guard is not None, sp.logprobs is not None, sp.timestamps))

    def shutdown(self):
        self.engine.close()

    def __del__(self):
        try:
            self.engine.close()
        except Exception:
            pass
