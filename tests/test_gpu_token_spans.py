"""Token time spans (csrc/t3_align_path.hip): the cell score and the monotonic path kernel against a plain numpy restatement of DESIGN.md
section 8 -- the score steps in float32, the dynamic programme in int64 -- and the engine path that serves a generate() call with one launch.
Everything behind the score is integer arithmetic, so every comparison of paths, spans and scores is exact."""
import ctypes as ct

import numpy as np
import pytest
import torch

from util import make_prompt

pytestmark = pytest.mark.gpu
f32 = np.float32
COEF = [f32(c) for c in (1.4426814317703247, -0.7203587889671326, 0.4686588644981384, -0.30163800716400146, 0.14447109401226044, -0.03382204473018646)]
NEG = -(1 << 30)


@pytest.fixture(scope="module")
def E():
    from chatterbox_vllm2_amd import engine
    engine.load_library()
    return engine


def clamp(a):
    lo, hi = f32(2.0 ** -64), f32(2.0 ** 64)
    with np.errstate(invalid="ignore"):
        a = np.where(np.asarray(a, f32) > lo, a, lo).astype(f32)
        return np.where(a < hi, a, hi).astype(f32)


def ref_scores(a):
    u = clamp(a).view(np.uint32)
    e = (u >> 23).astype(np.int32) - 127
    f = ((u & 0x7fffff) | 0x3f800000).view(f32) - f32(1.0)
    p = COEF[5]
    for c in COEF[4::-1]:
        p = c + f * p                    # float32 arrays: every product and sum rounded on its own
    return np.rint((e.astype(f32) + f * p) * f32(1024.0)).astype(np.int32)


def ref_path(A):
    """A [n, S] -> (path, start, end, last, score)"""
    n, S = A.shape
    w = ref_scores(A.reshape(-1)).reshape(n, S).astype(np.int64)
    D = np.full(S, NEG, np.int64); D[0] = w[0, 0]
    came = np.zeros((n, S), bool)
    for k in range(1, n):
        left = np.concatenate([[NEG], D[:-1]])
        came[k] = left > D
        D = np.where(np.arange(S) <= k, w[k] + np.maximum(D, left), NEG)
    last = int(np.argmax(D))             # the lowest index among equal maxima
    path = np.zeros(n, np.int32); t = last
    for k in range(n - 1, -1, -1):
        path[k] = t
        t -= int(came[k, t]) if k else 0
    start = np.full(S, -1, np.int32); end = np.full(S, -1, np.int32)
    for k in range(n - 1, -1, -1):
        start[path[k]] = k
    for k in range(n):
        end[path[k]] = k + 1
    return path, start, end, last, int(D[last])


def test_score_pin(E):
    xs = [v for q in range(-70, 3) for v in (f32(2.0 ** q), np.nextafter(f32(2.0 ** q), f32(0)), np.nextafter(f32(2.0 ** q), f32(np.inf)))]
    xs += [0.0, -1.0, 1e-40, np.nan, 1.0]
    a = np.concatenate([np.array(xs, f32), np.exp2(np.random.default_rng(0).uniform(-40, 0, 4096)).astype(f32)])
    w = E.k_align_scores(a)
    assert np.array_equal(w, ref_scores(a))
    err = np.abs(w - 1024 * np.log2(clamp(a).astype(np.float64))).max()
    print(f"score: max |w - 1024 log2 a'| = {err:.4f}")
    assert err <= 1


def matrix(kind, n, S, rng):
    if kind == "diagonal":               # a noisy diagonal softmax
        centre = np.arange(n)[:, None] * (S / n)
        z = -0.5 * (np.arange(S)[None] - centre) ** 2 / 4 + rng.normal(0, 1, (n, S))
        return (np.exp(z - z.max(1, keepdims=True)) / np.exp(z - z.max(1, keepdims=True)).sum(1, keepdims=True)).astype(f32)
    if kind == "ties":                   # two values only: ties at predecessors and at the end cell everywhere
        return rng.choice(np.array([0.25, 0.5], f32), (n, S))
    A = rng.uniform(0.01, 1, (n, S)).astype(f32)      # two columns of zeros (the clamp) that the path must cross to reach the large entries behind them
    A[:, S // 3 + 2:] *= f32(2.0 ** 20)
    A[:, S // 3: S // 3 + 2] = 0
    return A


SHAPES = [(1, 1), (1, 5), (5, 1), (3, 5), (64, 64), (65, 65), (130, 63), (130, 64), (130, 65), (130, 128), (130, 129), (200, 512), (200, 513),
          (63, 40), (64, 40), (65, 40), (129, 40), (40, 2050),
          (70, 256), (70, 257), (40, 1024), (40, 1025)]      # the two further boundaries between instantiations


@pytest.mark.parametrize("kind", ["diagonal", "ties", "zeros"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_path_parity(E, shape, kind):
    n, S = shape
    A = matrix(kind, n, S, np.random.default_rng(n * 4099 + S))
    padded = np.full((n, S + 5), 1e30, f32); padded[:, :S] = A      # pad columns: large values that must never be read into a result
    want = ref_path(A)
    for M in (A, padded):
        got = E.k_align_path(torch.from_numpy(M), S)
        for name, g, w in zip(("path", "start", "end", "last", "score"), got, want):
            assert np.array_equal(g, w), f"{name}: {g} vs {w}"


def test_engine_token_spans(E):
    from chatterbox_vllm2_amd import LLM, SamplingParams
    from chatterbox_vllm2_amd.weights import synthetic_cond_emb
    cond = synthetic_cond_emb(1)
    llm = LLM(model="", tokenizer="EnTokenizer", load_format="dummy", num_hidden_layers=2, max_model_len=200, max_num_seqs=3, kv_cache_bytes=1 << 28)
    llm.engine.set_alignment_heads([(0, 3), (1, 15)])
    prompts = [{"prompt_token_ids": make_prompt(5 + 4 * i, seed=80 + i)[34:-1], "multi_modal_data": {"conditionals": [cond]}} for i in range(3)]
    kw = dict(temperature=0.8, top_p=0.8, repetition_penalty=2.0, max_tokens=70, ignore_eos=True)
    marks = [dict(timestamps=True), dict(timestamps=True, alignment=True), {}]
    outs = llm.generate(prompts, [SamplingParams(seed=3 + i, **kw, **m) for i, m in enumerate(marks)], keep_for_handoff=True)
    c = [o.outputs[0] for o in outs]
    mats = [llm.engine.get_alignment(int(outs[0].request_id)), c[1].alignment]      # the first request's matrix: fetched here, before release
    assert c[0].alignment is None and c[2].timestamps is None and c[2].alignment is None
    for co, A in zip(c, mats):
        _, start, end, _, _ = ref_path(A.numpy())
        assert co.timestamps.dtype == torch.int32 and np.array_equal(co.timestamps.numpy(), np.stack([start, end], 1))
    # error codes: ld too small, untapped, unknown id, unfinished
    lib, h, buf = llm.engine.lib, llm.engine.h, np.zeros(64, np.int32)
    call = lambda rid, ld: lib.t3_get_token_spans(h, ct.byref(ct.c_int64(rid)), 1, ld, buf.ctypes.data, buf.ctypes.data, None, None, None)
    assert call(int(outs[0].request_id), 4) == E.T3_E_INVALID
    assert call(int(outs[2].request_id), 64) == E.T3_E_INVALID
    assert call(12345, 64) == -5
    for o in outs:
        llm.engine.release(int(o.request_id))
    llm.engine.add_request(777, make_prompt(5, seed=1), cond, E.make_sampling(alignment=True, max_tokens=3))
    assert call(777, 64) == -4
    llm.engine.abort(777)
    plain = llm.generate(prompts, [SamplingParams(seed=3 + i, **kw) for i in range(3)])
    assert [o.outputs[0].token_ids for o in plain] == [co.token_ids for co in c]
    llm.shutdown()
