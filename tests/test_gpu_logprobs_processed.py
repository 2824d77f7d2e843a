"""Processed log-probabilities: the second instantiation of the kernel behind the sampler (t3_logprobs.hip) and the engine path, against the numpy
restatement of the contract (test_logprobs_processed_host.ref_z, fp32 operation by operation) followed by a float64 log-softmax.
Bound: the raw kernel's, |lp - ref| <= 2e-5 + 2.4e-7 |ref| (test_gpu_logprobs.py derives it): the reference forms z with the kernel's own fp32
operations, so z is the same number on both sides and only the softmax differs, as in raw mode.  rank and the top ids are exact.  Measured: max
1.5e-6 at lp = -26, 7.0e-4 at lp = -21865 (profiles/NOTES.md).  The head rows are multiples of 1/4, so the post-CFG logits tie in droves."""
import numpy as np
import pytest
import torch

from chatterbox_vllm2_amd import engine as E
from test_logprobs_host import ref64
from test_logprobs_processed_host import V, ref_z
from util import make_prompt

pytestmark = pytest.mark.gpu
CFG, STOP = 0.5, 6562
DEF, ZERO = (2.0, 0.0, 0.0, 0.8), np.zeros(V, dtype=np.uint16)          # the reference defaults: repetition, frequency, presence, temperature
RNG = np.random.default_rng(3)
IDS = RNG.choice(V, 200, replace=False)                                  # the ids that carry a count; the first one a saturated count
COUNTS = ZERO.copy(); COUNTS[IDS] = RNG.integers(1, 6, 200); COUNTS[IDS[0]] = 65535
FREE = int(np.setdiff1d(np.arange(V), IDS)[50])                          # no count: the sampler's increment is all the kernel meets there
RUN = [0, 4000, 4001, 4002, 4007, 8193]                                  # biased: four ids of one run of eight, the first id, a tail lane's
BIAS = dict(zip(RUN + RNG.choice(np.setdiff1d(np.arange(V), RUN), 58, replace=False).tolist(), (RNG.standard_normal(64) * 3).astype(np.float32).tolist()))
BIAS[4002] = BIAS[list(BIAS)[10]] = float("-inf")
PROC = dict(allowed_ids=sorted(set(RNG.choice(V, 6550, replace=False).tolist()) | set(RUN) | {8192, STOP}), bias=BIAS, min_tokens=5, extra_stop_ids=[8192])
CASES = {       # (repetition, frequency, presence, temperature), counts, drawn id (None: what t3k_sample draws), step, processors, control word
    "plain": ((1.0, 0.0, 0.0, 1.0), COUNTS, int(IDS[3]), 0, None, -1),
    "defaults": (DEF, COUNTS, FREE, 0, None, -1),
    "presence-frequency": ((1.3, 0.3, 0.7, 0.9), COUNTS, int(IDS[0]), 0, None, -1),
    "greedy": ((2.0, 0.0, 0.0, 0.0), COUNTS, None, 0, None, -1),
    "processors": (DEF, COUNTS, 4001, 3, PROC, -1),
    "suppress": (DEF, COUNTS, int(IDS[5]), 7, None, 1),
    "force-held": (DEF, COUNTS, STOP, 3, dict(min_tokens=5), 2),
}


def check(z, token, rank, lp_tok, ids, tlp, what):
    lp, order = ref64(z)
    assert rank == int((z >= z[token]).sum()) and list(ids) == order[:len(ids)].tolist(), what
    for got, want in [(lp_tok, lp[token])] + list(zip(tlp, lp[np.asarray(ids, dtype=int)])):
        print(f"{what}: |lp - ref| = {abs(got - want) if np.isfinite(want) else 0.0:.3e} at ref = {want:.4f}")
        assert got == want if np.isinf(want) else abs(got - want) <= 2e-5 + 2.4e-7 * abs(want), what


@pytest.fixture(scope="module")
def logits():
    """(logits2 bf16 [2, 8208], the exact fp32 post-CFG logits from one greedy k_sample)"""
    g = torch.Generator().manual_seed(11)
    l2 = torch.full((2, 8208), 3e38)
    l2[0, :V], l2[1, :V] = ((torch.randn(V, generator=g) * 8).round() / 4 for _ in range(2))
    l2 = l2.to(torch.bfloat16)
    x = E.k_sample(l2, torch.from_numpy(ZERO.copy()), E.make_sampling(temperature=0.0, repetition_penalty=1.0), CFG, 0)[1].numpy()
    assert (x[IDS] > 0).any() and (x[IDS] < 0).any() and len(np.unique(x)) < V // 8
    return l2, x


@pytest.mark.parametrize("k", [0, 1, 20])
@pytest.mark.parametrize("case", list(CASES))
def test_kernel_against_the_contract(logits, case, k):
    (l2, x), (pen, counts, token, step, proc, ctl) = logits, CASES[case]
    sp = E.make_sampling(stop_token=STOP, repetition_penalty=pen[0], frequency_penalty=pen[1], presence_penalty=pen[2], temperature=pen[3])
    if token is None:       # greedy: the id sampler_kernel draws from the same counts pins the two restatements of the penalties against each other
        token = E.k_sample(l2, torch.from_numpy(counts.copy()), sp, CFG, step)[0]
    got = E.k_logprobs_processed(l2, CFG, torch.from_numpy(counts.copy()), sp, token, k, step, ctl, E.make_logit_processors(**proc) if proc else None)
    check(ref_z(x, counts, pen, step, proc, [STOP] + (proc or {}).get("extra_stop_ids", []), STOP if ctl == 1 else None), token, *got, f"{case} k {k}")
    if case == "plain":
        assert [np.asarray(g).tobytes() for g in got] == [np.asarray(r).tobytes() for r in E.k_logprobs(l2, CFG, token, k)], "raw hook, bit for bit"
    assert case != "greedy" or not k or got[2][0] == token
    assert case != "force-held" or (got[1] == -np.inf and got[0] == V)


EPROC = dict(allowed_ids=list(range(100, 124)), bias={101: 1.5, 110: float("-inf")}, min_tokens=4)          # 23 ids for 24 tokens: counts rise
REQS = [(0, 5, 3, None), (1, 12, 20, EPROC), (2, 9, 0, None)]          # id, text ids, k, processors
N, RAW, PRO = 24, "raw_logprobs", "processed_logprobs"


def start(weights, reqs, modes=(), reserve=20, max_tokens=N, max_seqs=4, **kw):
    from chatterbox_vllm2_amd.weights import synthetic_cond_emb
    eng = E.T3Engine(n_layers=2, text_vocab=704, max_model_len=128, max_seqs=max_seqs, kv_bytes=1 << 28, **kw)
    eng.load_tensors(weights); eng.finalize(); eng.reserve_logit_processors(True); eng.reserve_logprobs(reserve)
    for m in modes:
        eng.set_logprobs_mode(m)
    for i, n_text, k, proc in reqs:
        eng.add_request(i, make_prompt(n_text, seed=60 + i), synthetic_cond_emb(1),
                        E.make_sampling(uid=i, max_tokens=max_tokens, seed=5, ignore_eos=True, temperature=0.8, repetition_penalty=2.0))
        if proc:
            eng.request_logit_processors(i, E.make_logit_processors(**proc))
        if reserve >= 0:
            eng.request_logprobs(i, k)
    return eng


def test_engine_modes_paths_and_batches(tiny_weights):
    """a: eager steps with debug logits, processed (one token more: the finishing step releases the slot and its logits); b: graphs and bursts,
    processed; alone: request 1 in a batch of one; raw / today: mode 0 set back from 1, and never touched; off: nothing reserved."""
    a = start(tiny_weights, REQS, [PRO], debug_logits=True, max_tokens=N + 1, enforce_eager=True)
    assert a.lib.t3_set_logprobs_mode(a.h, 0) == -4 and a.lib.t3_set_logprobs_mode(a.h, 2) == -1          # T3_E_STATE: requests are queued; T3_E_INVALID
    rows = {i: [] for i, *_ in REQS}
    while a.num_unfinished():
        a.step()
        for i in rows:
            toks, fr = a.get_output(i)
            if len(toks) > len(rows[i]) and fr == 0:
                rows[i].append(a.debug_logits(i).numpy())
    b, alone, raw, today, off = (start(tiny_weights, r, m, enforce_eager=False, **kw) for r, m, kw in
                                 [(REQS, [PRO], {}), (REQS[1:2], [PRO], dict(max_seqs=1)), (REQS, [PRO, RAW], {}), (REQS, [], {}), (REQS, [], dict(reserve=-1))])
    for eng in (b, alone, raw, today, off):
        eng.run_until_done()
    same = lambda p, q, n=None: all(u[:n].tobytes() == v.tobytes() for u, v in zip(p, q))
    for i, _, k, proc in REQS:
        toks, got = b.get_output(i)[0], b.get_logprobs(i)
        assert len(toks) == N and all(toks == e.get_output(i)[0][:N] for e in (a, raw, today, off)), f"request {i}: ids"
        assert same(a.get_logprobs(i), got, N), f"request {i}: graphs / bursts vs eager steps"
        assert same(raw.get_logprobs(i), today.get_logprobs(i)), f"request {i}: raw mode vs the engine whose mode was never set"
        assert i != 1 or (toks == alone.get_output(i)[0] and same(got, alone.get_logprobs(i))), "a batch of three vs a batch of one"
        counts = np.zeros(V, dtype=np.int64)
        for t in range(N):
            check(ref_z(rows[i][t], counts, DEF, t, proc, [STOP]), toks[t] - 2500, got[1][t], got[0][t], got[2][t] - 2500, got[3][t], f"request {i} token {t}")
            counts[toks[t] - 2500] += 1
        assert not proc or counts.max() > 1
    for eng in (a, b, alone, raw, today, off):
        eng.close()
