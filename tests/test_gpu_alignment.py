"""The text-speech alignment export: the tap kernel (t3_alignment.hip) against a plain float64 softmax, and the engine path that collects
one fp32 matrix [n_tokens, n_text] per tapped request.

Tolerance of the kernel test, 4e-6 absolute against float64: an fp32 torch restatement of softmax(K q / 8) measured at most 2.8e-7 on the CPU
for these lengths and sigma = 3; 4e-6 is about 16x that, for the different summation order and the polynomial t3_expf.  Measured on the
MI355X over all cases below: max |error| 9.6e-7 on the bf16 pool, 4.7e-7 on the FP8 pool (profiles/NOTES.md)."""
import pytest
import torch

from util import assert_bit_equal, make_prompt, rand_bf16

pytestmark = pytest.mark.gpu
TOL = 4e-6


@pytest.fixture(scope="module")
def E():
    from chatterbox_vllm2_amd import engine
    engine.load_library()
    return engine


def seeded_qkv(L):
    qkv = rand_bf16(L, 3072, seed=L)
    qkv[:, :2048] = rand_bf16(L, 2048, seed=L + 1, scale=3.0)      # sigma = 3 for q and k: peaked and flat rows
    return qkv


@pytest.mark.parametrize("full", [True, False], ids=["whole-context", "text-span"])
@pytest.mark.parametrize("L", [35, 64, 65, 257, 321])      # partial first chunk, the chunk edge on both sides, the 256-token block edge, more chunks than waves
@pytest.mark.parametrize("head", [0, 15])
@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_probabilities_against_float64(E, kv_dtype, head, L, full):
    lo, hi = (0, L) if full else (34, min(L, 34 + 70))
    got, q_rot, kv = E.k_attention_probs(seeded_qkv(L), [0] * L, list(range(L)), 1, L + 3, head, lo, hi, kv_dtype)
    K = kv[:, 0, head * 64:(head + 1) * 64].double()
    s = q_rot.double() @ K.T / 8                                    # [row, position]; no RoPE here: q and K are what the kernel used / stored
    causal = torch.ones(L, L, dtype=torch.bool).tril()
    want = torch.softmax(s.masked_fill(~causal, float("-inf")), dim=1)[:, lo:hi]
    err = (got.double() - want).abs().max().item()
    print(f"alignment tap {kv_dtype} head {head} L {L} span [{lo}, {hi}): max |err| = {err:.3e}")
    assert err <= TOL
    assert (got[~causal[:, lo:hi]] == 0).all(), "positions beyond a row's context must be 0"
    if full:
        assert (got.double().sum(1) - 1).abs().max().item() <= TOL * L


def test_tap_rotates_q_with_the_rows_own_position(E):
    """q slice = k slice: the q the tap rotated for row r must be the K rope_kv stored for position r, bit for bit."""
    L, head = 70, 5
    qkv = seeded_qkv(L)
    qkv[:, head * 64:(head + 1) * 64] = qkv[:, 1024 + head * 64:1024 + (head + 1) * 64]
    _, q_rot, kv = E.k_attention_probs(qkv, [0] * L, list(range(L)), 1, L + 3, head, 0, L, "bf16")
    assert_bit_equal(q_rot, kv[:, 0, head * 64:(head + 1) * 64].contiguous(), "rotated q vs stored K")


TAPS = [(0, 3), (1, 15)]
KW = dict(temperature=0.8, top_p=0.8, repetition_penalty=2.0, seed=5, max_tokens=6, ignore_eos=True)


def run(E, weights, dtype, batches, tap=True, eager=False, max_seqs=4, taps=TAPS, text=70, between=None):
    """Batches of (id, n_text, tapped) run one after the other on one engine (between(eng) after the first) -> {id: (token ids, matrix or None)}"""
    from chatterbox_vllm2_amd.weights import synthetic_cond_emb
    eng = E.T3Engine(n_layers=2, text_vocab=704, max_model_len=128, max_seqs=max_seqs, kv_bytes=1 << 28, enforce_eager=eager, kv_cache_dtype=dtype)
    eng.load_tensors(weights); eng.finalize()
    eng.set_alignment_heads(taps); eng.reserve_alignment(text)
    out = {}
    for n, batch in enumerate(batches):
        if n == 1 and between:
            between(eng)
        for i, n_text, tapped in batch:
            eng.add_request(i, make_prompt(n_text, seed=60 + i), synthetic_cond_emb(1), E.make_sampling(uid=i, alignment=tap and tapped, **KW))
        eng.run_until_done()
        for i, n_text, tapped in batch:
            out[i] = (eng.get_output(i)[0], eng.get_alignment(i) if tap and tapped else None)
            eng.release(i)
    eng.close()
    return out


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_engine_alignment(E, tiny_weights, dtype, monkeypatch):
    """Text lengths 5, 70 (its span crosses a chunk edge; untapped) and 12: ids do not depend on the flag, every frame is written, and the
    matrices are bit-identical between eager steps, one-step graphs, bursts, the request alone in a fresh slot and in a reused one."""
    reqs = [(0, 5, True), (1, 70, False), (2, 12, True)]
    burst = run(E, tiny_weights, dtype, [reqs])
    off = run(E, tiny_weights, dtype, [reqs], tap=False)
    for i, n_text, tapped in reqs:
        ids, A = burst[i]
        assert ids == off[i][0], "token ids must not depend on the alignment flag"
        if not tapped:
            assert A is None
            continue
        assert tuple(A.shape) == (6, n_text) and torch.isfinite(A).all() and (A >= 0).all() and (A <= 1).all()
        sums = A.double().sum(1)
        assert (sums > 0).all() and (sums <= 1 + 1e-5).all(), f"a zero row is a frame nobody wrote: {sums.tolist()}"
    others = {"eager": run(E, tiny_weights, dtype, [reqs], eager=True),
              "alone in a fresh slot": run(E, tiny_weights, dtype, [[reqs[0]]], max_seqs=1),
              "in a reused slot": run(E, tiny_weights, dtype, [[reqs[2]], [reqs[0]]], max_seqs=1)}
    monkeypatch.setenv("T3_STEPS_PER_GRAPH", "1")
    others["one-step graphs"] = run(E, tiny_weights, dtype, [reqs])
    for what, res in others.items():
        for i in res:
            if burst[i][1] is not None:
                assert res[i][0] == burst[i][0]
                assert_bit_equal(res[i][1], burst[i][1], f"request {i}, {what} vs bursts")


def test_reserve_and_heads_change_between_requests(E, tiny_weights):
    """A larger reserve (another buffer and pitch) and other heads between two tapped requests of one batch shape: the second request's
    decode steps must not replay graphs captured for the first configuration -- its matrix is a fresh engine's, bit for bit."""
    other = [(0, 7), (1, 2)]
    got = run(E, tiny_weights, "bf16", [[(0, 5, True)], [(2, 12, True)]], max_seqs=1, text=8,
              between=lambda eng: (eng.reserve_alignment(70), eng.set_alignment_heads(other)))
    want = run(E, tiny_weights, "bf16", [[(2, 12, True)]], max_seqs=1, taps=other)
    assert got[2][0] == want[2][0]
    assert_bit_equal(got[2][1], want[2][1], "request 2 after a re-reserve and new heads vs a fresh engine")


def test_alignment_error_codes(E, tiny_weights):
    from chatterbox_vllm2_amd.weights import synthetic_cond_emb
    eng = E.T3Engine(n_layers=2, text_vocab=704, max_model_len=128, max_seqs=2, kv_bytes=1 << 28)
    eng.load_tensors(tiny_weights); eng.finalize()
    add = lambda i, n_text, tap: eng.add_request(i, make_prompt(n_text, seed=i), synthetic_cond_emb(1), E.make_sampling(uid=i, alignment=tap, **KW))
    with pytest.raises(E.T3Error, match=r"\[-4\].*t3_reserve_alignment"):        # T3_E_STATE: no reserve yet
        add(0, 5, True)
    eng.reserve_alignment(8)
    with pytest.raises(E.T3Error, match=r"\[-4\].*no alignment head"):           # T3_E_STATE: none of the default taps' layers (9, 12, 13) exists here
        add(0, 5, True)
    eng.set_alignment_heads(TAPS)
    with pytest.raises(ValueError):                         # text longer than the reserve
        add(0, 9, True)
    add(0, 8, True); add(1, 8, False)
    eng.run_until_done()
    assert tuple(eng.get_alignment(0).shape) == (6, 8)
    with pytest.raises(ValueError):                         # T3_E_INVALID: not tapped
        eng.get_alignment(1)
    eng.release(0)
    with pytest.raises(E.T3Error, match=r"\[-5\]"):        # T3_E_NOTFOUND: released
        eng.get_alignment(0)
    eng.close()
