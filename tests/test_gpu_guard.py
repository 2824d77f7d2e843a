"""The alignment guard: the kernel (t3_guard.hip) and the guarded sampler against a plain numpy restatement of the contract in
include/t3_engine.h, and the engine path that runs both inside every step.  argmax and max are exact and the two running sums are float32
adds in step order -- the kernel's own arithmetic -- so every comparison is for equality."""
import numpy as np
import pytest
import torch

from util import make_prompt, rand_bf16

REASONS = ["token_repetition", "long_tail", "alignment_repetition"]


@pytest.fixture(scope="module")
def E():
    from chatterbox_vllm2_amd import engine
    engine.load_library()
    return engine


def guard_reference(A, S, tok, back=4, fwd=7, end=3, skip=5, tail_thr=5.0, rep_thr=5.0, tok_rep=3):
    """-> (control word per frame: 0 nothing, 1 suppress, 2 force; final state)"""
    st = dict(pos=0, complete=False, completed_at=0, forced_at=-1, reason=None, tail=[np.float32(0)] * 3, rep=np.float32(0))
    ctl = []
    for k in range(len(A)):
        if st["forced_at"] >= 0:
            ctl.append(2)
            continue
        a = np.asarray(A[k], dtype=np.float32)[:S]
        c = int(np.argmax(a))
        if -back < c - st["pos"] < fwd:
            st["pos"] = c
        if not st["complete"] and st["pos"] >= S - end:
            st["complete"], st["completed_at"] = True, k
        if st["complete"]:
            for i in range(3):
                if S - 3 + i >= 0:
                    st["tail"][i] = np.float32(st["tail"][i] + a[S - 3 + i])
            if S - skip > 0:
                st["rep"] = np.float32(st["rep"] + a[:S - skip].max())
        hits = [tok_rep > 0 and k >= tok_rep and len(set(tok[k - tok_rep:k])) == 1,
                st["complete"] and max(st["tail"]) >= np.float32(tail_thr), st["complete"] and st["rep"] > np.float32(rep_thr)]
        if any(hits):
            st["reason"], st["forced_at"] = REASONS[hits.index(True)], k
        ctl.append(2 if any(hits) else 1 if st["pos"] < S - end and S > skip else 0)
    st["tail"] = [float(x) for x in st["tail"]]; st["rep"] = float(st["rep"])
    return ctl, st


PEAK = 48 / 64


def scenario(name, S):
    """-> (A [frames, ld] with 1e9 in the padding columns, ids, parameter overrides): noise of 0..3/64 with one peak per frame"""
    walk = list(range(0, S, 6)) + [S - 1]                      # forward steps below fwd = 7, so the position follows
    p = dict(tail_thr=2.0, rep_thr=2.0)
    peaks = {"tail": walk + [S - 1] * 6,                       # lingers on the last column
             "back": walk + [0] * 6,                           # spoken to the end, then back to column 0: discontinuities, mass over spoken text
             "jump": [0, 1, min(S - 1, 9)] + [min(S - 1, 9)] * 5,    # a step of fwd or more is not followed
             "never": [0] * 8,                                 # suppressed to the end
             "tie": [0, 1, 2] + [2] * 5,
             "tokens": [0] * 12, "tok_rep0": [0] * 12}[name]
    F, ld = len(peaks), (S + 3) // 4 * 4 + 4
    A = np.full((F, ld), 1e9, dtype=np.float32)
    A[:, :S] = np.random.RandomState(S).randint(0, 4, size=(F, S)) / 64
    for k, c in enumerate(peaks):
        A[k, min(c, S - 1)] = PEAK
    if name == "tie":
        A[3:, S - 1] = PEAK                                    # as high as column 2 (or the same column): the lower index must win
    tok = [100 + k for k in range(F)]
    if name in ("tokens", "tok_rep0"):
        tok[5] = tok[6] = tok[7] = 7
        p["tok_rep"] = 3 if name == "tokens" else 0
    return A, tok, p


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tail", "back", "jump", "never", "tie", "tokens", "tok_rep0"])
@pytest.mark.parametrize("S", [3, 5, 6, 7, 64, 255, 256, 257, 600])
def test_guard_kernel_against_reference(E, S, name):
    A, tok, p = scenario(name, S)
    want_ctl, want = guard_reference(A, S, tok, **p)
    got_ctl, got = E.k_alignment_guard(torch.from_numpy(A), S, tok, p)
    assert got_ctl == want_ctl
    assert got == want


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(temperature=0.0), dict(temperature=0.8, top_p=0.8, top_k=50, min_p=0.02, repetition_penalty=1.2, seed=3)],
                         ids=["greedy", "stochastic"])
def test_sampler_obeys_the_control_word(E, kw):
    STOP = 6562
    sp = E.make_sampling(stop_token=STOP, uid=1, **kw)
    lg = rand_bf16(2, 8208, seed=11)
    lg[0, STOP] = 30.0                                         # the stop id is the top logit
    held = lg.clone(); held[0, STOP] = float("-inf")
    fresh = lambda: torch.zeros(8194, dtype=torch.uint16)
    plain, without = E.k_sample(lg, fresh(), sp, 0.5, 4)[0], E.k_sample(held, fresh(), sp, 0.5, 4)[0]
    assert plain == STOP and without != STOP
    assert E.k_sample_ctl(lg, fresh(), sp, 0.5, 4, 0) == plain
    assert E.k_sample_ctl(lg, fresh(), sp, 0.5, 4, 1) == without
    counts = fresh()
    assert E.k_sample_ctl(held, counts, sp, 0.5, 4, 2) == STOP and counts.view(torch.int16)[STOP].item() == 1
    assert E.k_sample_ctl(torch.full_like(lg, float("nan")), fresh(), sp, 0.5, 4, 2) == STOP


TAPS, STOP = [(0, 3), (1, 15)], 6562
# Synthetic weights attend almost evenly (a frame's largest entry is about 0.02), so the thresholds come down to where forcing happens within
# two dozen steps.  Picked from an UNGUARDED run of these four requests (the guard changes no id before it forces, as no stop id is drawn on
# its own): replaying guard_reference over its matrices forces request 1 by alignment repetition (step 14 on the bf16 pool, 19 on FP8) and
# request 5 by a long tail (14 / 17), each behind several suppressed steps.
GP = dict(tail_thr=0.2, rep_thr=0.25)
REQS = [(1, 12, True), (2, 20, False), (5, 9, True), (6, 16, False)]      # (id, n_text, guarded)
_unguarded = {}


def run_engine(E, weights, dtype, eager, guard):
    from chatterbox_vllm2_amd.weights import synthetic_cond_emb
    eng = E.T3Engine(n_layers=2, text_vocab=704, max_model_len=128, max_seqs=4, kv_bytes=1 << 28, enforce_eager=eager, kv_cache_dtype=dtype)
    eng.load_tensors(weights); eng.finalize()
    eng.set_alignment_heads(TAPS); eng.reserve_alignment(20); eng.set_alignment_guard(GP)
    for i, n_text, g in REQS:
        eng.add_request(i, make_prompt(n_text, seed=60 + i), synthetic_cond_emb(1),
                        E.make_sampling(uid=i, temperature=0.0, repetition_penalty=2.0, max_tokens=32, stop_token=STOP, alignment_guard=guard and g))
    eng.run_until_done()
    out = {i: eng.get_output(i) + ((eng.get_alignment(i), eng.get_guard(i)) if guard and g else ()) for i, _, g in REQS}
    eng.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("mode", ["eager", "graph", "burst"])
def test_engine_guard(E, tiny_weights, mode, dtype, monkeypatch):
    if mode == "graph":
        monkeypatch.setenv("T3_STEPS_PER_GRAPH", "1")
    if dtype not in _unguarded:
        _unguarded[dtype] = run_engine(E, tiny_weights, dtype, False, False)
    got = run_engine(E, tiny_weights, dtype, mode == "eager", True)
    reasons = []
    for i, S, guarded in REQS:
        if not guarded:
            assert got[i] == _unguarded[dtype][i], "an unguarded request's ids must not depend on guarded neighbours"
            continue
        ids, finish, A, state = got[i]
        tok = [t - 2500 for t in ids]
        ctl, want = guard_reference(A.numpy(), S, tok, **GP)
        print(f"{dtype} {mode} request {i}: {state}")
        assert state == want
        assert state["forced_at"] == len(tok) - 1 and tok[-1] == STOP and finish == 1
        assert all(t != STOP for t, c in zip(tok, ctl) if c == 1), "a stop id at a suppressed step"
        reasons.append(state["reason"])
    assert set(reasons) & {"long_tail", "alignment_repetition"}


def test_guard_parameter_errors():
    from chatterbox_vllm2_amd.llm import SamplingParams
    assert SamplingParams(alignment_guard=dict(tail_thr=1.0), stop_token_ids=[9062]).alignment
    for bad in (dict(alignment_guard=True), dict(alignment_guard=True, stop_token_ids=[9062], ignore_eos=True),
                dict(alignment_guard=dict(tail=1.0), stop_token_ids=[9062]), dict(alignment_guard=3, stop_token_ids=[9062])):
        with pytest.raises(ValueError):
            SamplingParams(**bad)
