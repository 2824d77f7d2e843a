"""Logit processors inside the sampler kernel (t3_kernels.hip PROC instantiation, t3_logitproc.hip): allow list, biases, min_tokens, stop lists.
The kernel checks are exact: a bias is ONE fp32 add, a mask is -inf, so logits compare bit for bit against numpy on the sampler's own raw
logits, and a masked draw must equal the unprocessed sampler's draw on logits whose conditional row is -inf at the masked ids."""
import numpy as np
import pytest
import torch

from chatterbox_vllm2_amd import engine as E
from chatterbox_vllm2_amd.llm import LLM, SamplingParams
from chatterbox_vllm2_amd.weights import synthetic_cond_emb
from util import make_prompt

pytestmark = pytest.mark.gpu
V, CFG, STOP = 8194, 0.5, 6562
EDGE = [0, 63, 64, 8191, 8192, 8193]          # word boundaries of the bitmask, the last vector, the two ids that go element by element
PARAMS = dict(greedy=dict(temperature=0.0), top_k=dict(temperature=0.9, top_k=40), top_p=dict(temperature=0.8, top_p=0.8),
              min_p=dict(temperature=1.0, min_p=0.05))


def logits2(seed):
    g = torch.Generator().manual_seed(seed)
    l2 = torch.full((2, 8208), 3e38)
    l2[:, :V] = torch.randn(2, V, generator=g) * 3
    return l2.to(torch.bfloat16)


@pytest.fixture(scope="module")
def raw():          # seed -> the sampler's own fp32 post-CFG logits
    greedy = E.make_sampling(temperature=0.0, repetition_penalty=1.0)
    return {s: E.k_sample(logits2(s), torch.zeros(V, dtype=torch.uint16), greedy, CFG, 0)[1].numpy() for s in range(3)}


@pytest.mark.parametrize("n_bias", [0, 1, 64])
@pytest.mark.parametrize("seed", range(3))
def test_processed_logits_bit_for_bit(raw, seed, n_bias):
    rs = np.random.RandomState(seed)
    ids = (EDGE + [i for i in rs.permutation(V).tolist() if i not in EDGE])[:n_bias] if n_bias > 1 else [EDGE[seed * 2 + 1]][:n_bias]
    vals = (rs.randn(n_bias) * 5).astype(np.float32)
    vals[3::7] = -np.inf
    order = rs.permutation(n_bias)
    masked = [5, 62, 8192, 4097] if n_bias != 1 else []          # 8192 is biased AND masked at n_bias = 64
    lp = E.make_logit_processors(allowed_ids=[i for i in rs.permutation(V).tolist() if i not in masked] if masked else None,
                                 bias=[(ids[i], vals[i]) for i in order])
    _, got, _ = E.k_sample_proc(logits2(seed), torch.zeros(V, dtype=torch.uint16), E.make_sampling(temperature=0.0, repetition_penalty=1.0), CFG, 0, lp)
    want = raw[seed].copy()
    ids = np.asarray(ids, dtype=int)
    want[ids] = want[ids] + vals
    want[masked] = -np.inf
    assert got.numpy().tobytes() == want.tobytes()


@pytest.mark.parametrize("n_allow", [1, 2, 6562, 8194])
@pytest.mark.parametrize("name", PARAMS)
def test_mask_equals_minus_inf_in_the_conditional_row(name, n_allow):
    rs = np.random.RandomState(n_allow)
    allowed = {1: [8193], 2: [8192, 31], 6562: list(range(6561)) + [STOP], 8194: list(range(V))}[n_allow]
    sp = E.make_sampling(repetition_penalty=1.2, seed=11, uid=4, **PARAMS[name])
    cnt = torch.from_numpy((rs.rand(V) < 0.01).astype(np.uint16))
    l2 = logits2(1)
    tok, _, keep = E.k_sample_proc(l2, cnt.clone(), sp, CFG, 3, E.make_logit_processors(allowed_ids=rs.permutation(allowed).tolist()))
    ref = l2.clone()
    ref[0, np.setdiff1d(np.arange(V), allowed)] = float("-inf")
    want_tok, want_keep = E.k_sample_support(ref, cnt.clone(), sp, CFG, 3)
    assert tok == want_tok and tok in allowed and torch.equal(keep, want_keep)


@pytest.mark.parametrize("n_stop", [1, 4])
def test_min_tokens(raw, n_stop):
    stops = np.argsort(-raw[0])[:n_stop].tolist()          # the most likely ids: inside every unprocessed support
    sp = E.make_sampling(temperature=1.0, top_k=50, repetition_penalty=1.0, stop_token=stops[0], seed=2)
    lp = E.make_logit_processors(min_tokens=6, extra_stop_ids=stops[1:])
    _, _, held = E.k_sample_proc(logits2(0), torch.zeros(V, dtype=torch.uint16), sp, CFG, 5, lp)
    _, _, free = E.k_sample_proc(logits2(0), torch.zeros(V, dtype=torch.uint16), sp, CFG, 6, lp)
    _, plain = E.k_sample_support(logits2(0), torch.zeros(V, dtype=torch.uint16), sp, CFG, 6)
    assert not held[stops].any() and held.any() and free[stops].all() and torch.equal(free, plain)


@pytest.mark.parametrize("name", ["greedy", "top_p"])
@pytest.mark.parametrize("allowed, want", [([900, 7], 7), ([], 0), (None, 0)])
def test_row_without_a_finite_logit_draws_the_lowest_allowed_id(name, allowed, want):
    bias = {i: -np.inf for i in (allowed or [])} if allowed is not None else {}
    l2 = logits2(2)
    if allowed is None:
        l2[0, :V] = float("-inf")
    tok, got, keep = E.k_sample_proc(l2, torch.zeros(V, dtype=torch.uint16), E.make_sampling(repetition_penalty=1.0, **PARAMS[name]), CFG, 0,
                                     E.make_logit_processors(allowed_ids=allowed, bias=bias))
    assert tok == want and np.isneginf(got.numpy()).all() and keep.nonzero().flatten().tolist() == [want]


SPEECH = list(range(2500, 2500 + 6561)) + [2500 + STOP]


@pytest.fixture(scope="module")
def llms():
    kw = dict(model="", load_format="dummy", num_hidden_layers=2, max_model_len=160, max_num_seqs=4, kv_cache_bytes=1 << 28)
    both = LLM(**kw), LLM(honor_enforce_eager=True, enforce_eager=True, **kw)          # graphs + bursts, eager steps
    yield both
    for m in both:
        m.shutdown()


def run(llm, sps):
    prompts = [dict(prompt_token_ids=make_prompt(5 + 3 * i, seed=80 + i)[34:-1], multi_modal_data=dict(conditionals=[synthetic_cond_emb(1)])) for i in range(len(sps))]
    return [o.outputs[0] for o in llm.generate(prompts, sps)]


def test_engine(llms):
    fast, eager = llms
    kw = dict(temperature=1.0, repetition_penalty=1.2, max_tokens=64, ignore_eos=True)
    plain = [SamplingParams(seed=7 + i, logprobs=2, **kw) for i in range(3)]
    before = run(fast, plain)                                     # nothing reserved yet
    assert any(t not in SPEECH for o in before for t in o.token_ids), "the seeds must draw an id outside the speech range unconstrained"
    marked = [SamplingParams(seed=7 + i, logprobs=2, allowed_token_ids=SPEECH, **kw) for i in range(2)] + plain[2:]
    got, got_eager = run(fast, marked), run(eager, marked)
    assert all(len(o.token_ids) == 64 and all(t in SPEECH for t in o.token_ids) for o in got[:2])
    assert [o.token_ids for o in got] == [o.token_ids for o in got_eager]                  # graphs and bursts against eager steps
    assert got[2].token_ids == before[2].token_ids                                         # the unmarked request of the shared batch
    top2 = [{i: lp.logprob for i, lp in o.logprobs[0].items() if lp.rank <= 2} for o in (got[0], before[0])]
    assert top2[0] and top2[0] == top2[1]                                        # raw log-probabilities of token 0: in front of the processors
    stop = 2500 + STOP
    o = run(fast, [SamplingParams(seed=3, temperature=1.0, max_tokens=40, stop_token_ids=[stop], logit_bias={stop: 100.0}, min_tokens=5)])[0]
    assert len(o.token_ids) == 6 and o.token_ids[-1] == stop and stop not in o.token_ids[:5] and o.finish_reason == "stop"
    second = before[0].token_ids[4]                               # an id the unconstrained request draws as its fifth token
    o = run(fast, [SamplingParams(seed=7, temperature=1.0, repetition_penalty=1.2, max_tokens=64, stop_token_ids=[stop, second])])[0]
    cut = min(i for i, t in enumerate(before[0].token_ids) if t in (stop, second))
    assert o.token_ids == before[0].token_ids[:cut + 1] and o.finish_reason == "stop"


def test_state_and_argument_errors(tiny_weights):
    eng = E.T3Engine(n_layers=2, text_vocab=704, max_model_len=128, max_seqs=1, kv_bytes=1 << 28)
    eng.load_tensors(tiny_weights); eng.finalize()
    eng.add_request(0, make_prompt(5, seed=1), synthetic_cond_emb(1), E.make_sampling(max_tokens=4, ignore_eos=True))
    with pytest.raises(E.T3Error, match=r"\[-4\]"):              # before a reserve: T3_E_STATE, even for a malformed struct
        eng.request_logit_processors(0, E.make_logit_processors(min_tokens=-1))
    eng.run_until_done(); eng.release(0)
    eng.reserve_logit_processors(True)
    eng.add_request(1, make_prompt(5, seed=1), synthetic_cond_emb(1), E.make_sampling(max_tokens=4, ignore_eos=True))
    for bad in (dict(bias=[(3, 1.0), (3, 2.0)]), dict(bias={V: 0.0}), dict(bias={1: float("nan")}), dict(min_tokens=-1), dict(allowed_ids=[V])):
        with pytest.raises(ValueError):
            eng.request_logit_processors(1, E.make_logit_processors(**bad))
    eng.request_logit_processors(1, E.make_logit_processors(allowed_ids=[STOP], min_tokens=99))      # legal: it ends at its length limit
    eng.step()
    with pytest.raises(E.T3Error, match=r"\[-4\]"):              # admitted
        eng.request_logit_processors(1, E.make_logit_processors())
    eng.run_until_done()
    assert eng.get_output(1) == ([2500 + STOP] * 4, 2)            # whatever the hold leaves, the one allowed id is drawn; the length limit ends it
    eng.close()
