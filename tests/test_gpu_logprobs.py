"""Per-token log-probabilities: the kernel behind the sampler (t3_logprobs.hip) and the engine path against a float64 log-softmax.
Bound, |lp - ref| <= 2e-5 + 2.4e-7 |ref|: t3_expf is pinned below 3e-7 relative (test_gpu_kernels.py); the fp32 sum of <= 8194 non-negative
terms by per-thread partials of 33, a butterfly and four waves stays below 3e-6 relative on Z; logf is a few ulp; x - M and the final
subtraction round once each, 2^-23 |lp| together.  rank and the top ids are exact.  Measured: max 9.0e-7 (profiles/NOTES.md).
The row of case "minus-inf" at cfg = 0 holds NaN (0 * inf in the CFG mix), outside the numeric contract: there the call returns in bounds."""
import numpy as np
import pytest

from chatterbox_vllm2_amd import engine as E
from test_logprobs_host import CASES, V, logits_case, ref64
from util import make_prompt

pytestmark = pytest.mark.gpu


def check(x, token, rank, lp_tok, ids, tlp, what):
    lp, order = ref64(x)
    assert rank == int((x >= x[token]).sum()), what
    assert list(ids) == order[:len(ids)].tolist(), what
    for got, want in [(lp_tok, lp[token])] + list(zip(tlp, lp[np.asarray(ids, dtype=int)])):
        print(f"{what}: |lp - ref| = {abs(got - want):.3e} at ref = {want:.4f}")
        assert abs(got - want) <= 2e-5 + 2.4e-7 * abs(want), what


@pytest.fixture(scope="module")
def post_cfg():
    """(case, cfg) -> the exact fp32 post-CFG logits, from one greedy k_sample each"""
    import torch
    greedy = E.make_sampling(temperature=0.0, repetition_penalty=1.0)
    return {(c, cfg): E.k_sample(logits_case(c)[0], torch.zeros(V, dtype=torch.uint16), greedy, cfg, 0)[1].numpy() for c in CASES for cfg in (0.0, 0.5)}


@pytest.mark.parametrize("k", [0, 1, 20])
@pytest.mark.parametrize("cfg", [0.0, 0.5])
@pytest.mark.parametrize("case", CASES)
def test_kernel_against_float64(post_cfg, case, cfg, k):
    l2, token = logits_case(case)
    rank, lp_tok, ids, tlp = E.k_logprobs(l2, cfg, token, k)
    x = post_cfg[case, cfg]
    if np.isnan(x).any():
        assert (case, cfg) == ("minus-inf", 0.0) and 0 <= rank <= V and ((ids >= 0) & (ids < V)).all()
        return
    check(x, token, rank, lp_tok, ids, tlp, f"{case} cfg {cfg} k {k}")


REQS = [(0, 5, 3), (1, 12, 20), (2, 9, None)]          # id, text ids, k (None: not marked)
KW = dict(temperature=0.8, repetition_penalty=2.0, seed=5, ignore_eos=True)


def start(weights, reqs, reserve=20, max_tokens=10, max_seqs=4, **kw):
    from chatterbox_vllm2_amd.weights import synthetic_cond_emb
    eng = E.T3Engine(n_layers=2, text_vocab=704, max_model_len=128, max_seqs=max_seqs, kv_bytes=1 << 28, enforce_eager=False, **kw)
    eng.load_tensors(weights); eng.finalize()
    if reserve is not None:
        eng.reserve_logprobs(reserve)
    for i, n_text, k in reqs:
        eng.add_request(i, make_prompt(n_text, seed=60 + i), synthetic_cond_emb(1), E.make_sampling(uid=i, max_tokens=max_tokens, **KW))
        if reserve is not None and k is not None:
            eng.request_logprobs(i, k)
    return eng


def test_engine_against_its_debug_logits(tiny_weights):
    """A: step by step with debug logits (its finishing step releases the slot, so it runs an 11th token to leave the logits of ten readable);
    B: graphs, bursts and run-ahead; C: nothing reserved.  A's numbers meet the kernel's bounds, B's records are A's bit for bit, ids are equal."""
    a = start(tiny_weights, REQS, debug_logits=True, max_tokens=11)
    rows = {i: [] for i, _, _ in REQS}
    while a.num_unfinished():
        a.step()
        for i in rows:
            toks, fr = a.get_output(i)
            if len(toks) > len(rows[i]) and fr == 0:
                rows[i].append(a.debug_logits(i).numpy())
    b = start(tiny_weights, REQS); b.run_until_done()
    c = start(tiny_weights, REQS, reserve=None); c.run_until_done()
    for i, _, k in REQS:
        toks = b.get_output(i)[0]
        assert len(toks) == 10 and toks == a.get_output(i)[0][:10] == c.get_output(i)[0]
        if k is None:
            with pytest.raises(ValueError):          # T3_E_INVALID: not marked
                a.get_logprobs(i)
            continue
        got_a, got_b = a.get_logprobs(i), b.get_logprobs(i)
        assert [len(g) for g in got_a] == [11] * 4 and got_b[2].shape == (10, k)
        for ga, gb in zip(got_a, got_b):
            assert ga[:10].tobytes() == gb.tobytes(), f"request {i}: graphs / bursts vs eager steps"
        for t in range(10):
            check(rows[i][t], toks[t] - 2500, got_b[1][t], got_b[0][t], got_b[2][t] - 2500, got_b[3][t], f"request {i} token {t}")
    a.close(); b.close(); c.close()


@pytest.mark.parametrize("case, err", [("mark-before-reserve", -4), ("k-above-max", -1), ("mark-after-step", -4), ("reserve-while-queued", -4),
                                       ("get-unfinished", -4), ("get-released", -5)])
def test_state_errors(tiny_weights, case, err):
    eng = start(tiny_weights, [(0, 5, 1 if case.startswith("get") else None)], reserve=None if case == "mark-before-reserve" else 3, max_seqs=1)
    if case in ("mark-after-step", "get-unfinished"):
        eng.step()
    if case == "get-released":
        eng.run_until_done(); eng.release(0)
    call = (eng.get_logprobs if case.startswith("get") else (lambda i: eng.reserve_logprobs(5)) if case.startswith("reserve")
            else (lambda i: eng.request_logprobs(i, 4 if case == "k-above-max" else 1)))
    with (pytest.raises(ValueError) if err == -1 else pytest.raises(E.T3Error, match=rf"\[{err}\]")):          # T3_E_INVALID surfaces as ValueError
        call(0)
    eng.close()


def test_slot_reuse(tiny_weights):
    """One slot, two marked requests one after the other: the second returns its own records, those of a run alone in a fresh slot."""
    both = start(tiny_weights, REQS[:2], max_seqs=1); both.run_until_done()
    alone = start(tiny_weights, REQS[1:2], max_seqs=1); alone.run_until_done()
    assert both.get_output(1)[0] == alone.get_output(1)[0]
    for x, y in zip(both.get_logprobs(1), alone.get_logprobs(1)):
        assert x.shape == y.shape and x.tobytes() == y.tobytes()
    both.close(); alone.close()
