"""The layer projections over MXFP8 weights (t3_gemm_mx8.hip) against the oracle over the dequantised matrix mx8(bf16(W * ln)).  Bar: BIT-EXACT --
every stored value is a bf16 value and the numerics contract is the bf16 forms'."""
import pytest
import torch

from test_weights_mxfp8_host import mx8
from util import assert_bit_equal, make_prompt, rand_bf16

pytestmark = pytest.mark.gpu
MS = [1, 2, 16, 17, 64, 65, 130, 545]      # a ragged last group, several groups per workgroup, well past one workgroup's loop
MMAX = max(MS)


@pytest.fixture(scope="module")
def E():
    from chatterbox_vllm2_amd import engine
    engine.load_library()
    return engine


def weights(N, K, seed, scale):
    W = rand_bf16(N, K, seed=seed, scale=scale)
    blk = W.view(-1, 32)
    blk[::3] *= 1000; blk[1::3] /= 512
    return W


def folded(W, ln):
    return mx8((W.float() * ln.float()).to(torch.bfloat16))


@pytest.fixture(scope="module")
def qkv_case(oracle):
    h = rand_bf16(MMAX, 1024, seed=11, scale=2.0); ln = (rand_bf16(1024, seed=9) + 1.0).to(torch.bfloat16); W = weights(3072, 1024, 21, 0.05)
    return h, ln, W, oracle.norm_gemm(h, torch.ones_like(ln), folded(W, ln)).to(torch.bfloat16)


@pytest.mark.parametrize("M", MS)
def test_qkv_form(E, qkv_case, M):
    h, ln, W, want = qkv_case
    assert_bit_equal(E.k_qkv_gemm_mx8(h[:M], ln, W), want[:M], f"qkv over mxfp8 M={M}")


@pytest.fixture(scope="module")
def resid_cases(oracle):
    out = {}
    for K, N in [(1024, 1024), (1024, 48), (4096, 1024), (4096, 48)]:
        x = rand_bf16(MMAX, K, seed=K + 3); W = weights(N, K, N + 4, 0.05); h = rand_bf16(MMAX, N, seed=5, scale=2.0)
        y = oracle.gemm(x, mx8(W), K // 16).to(torch.bfloat16)
        out[K, N] = x, W, h, (h.float() + y.float()).to(torch.bfloat16)
    return out


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("K,N", [(1024, 1024), (1024, 48), (4096, 1024), (4096, 48)])
def test_residual_forms(E, resid_cases, K, N, M):
    x, W, h, want = resid_cases[K, N]
    assert_bit_equal(E.k_gemm_resid_mx8(x[:M], W, h[:M]), want[:M], f"h + bf16(x mx8(W)^T) K={K} N={N} M={M}")


@pytest.fixture(scope="module")
def gate_up_cases(oracle):
    out = {}
    for Fd, rows in [(48, MMAX), (4096, 130)]:
        h = rand_bf16(rows, 1024, seed=Fd, scale=2.0); ln = (rand_bf16(1024, seed=8) + 1.0).to(torch.bfloat16)
        Wg = weights(Fd, 1024, 2, 0.1); Wu = weights(Fd, 1024, 3, 0.1)
        g, u = (oracle.norm_gemm(h, torch.ones_like(ln), folded(W, ln)).to(torch.bfloat16) for W in (Wg, Wu))
        out[Fd] = h, ln, Wg, Wu, oracle.silu_mul(g, u)
    return out


@pytest.mark.parametrize("Fd,M", [(48, M) for M in MS] + [(4096, 130)])
def test_gate_up_form(E, gate_up_cases, Fd, M):
    h, ln, Wg, Wu, want = gate_up_cases[Fd]
    assert_bit_equal(E.k_silu_mul_gemm_mx8(h[:M], ln, Wg, Wu), want[:M], f"silu(gate) * up over mxfp8 F={Fd} M={M}")


def test_engine_mxfp8_equals_bf16_engine_over_the_stored_values(E, tiny_weights):
    """2 layers, both RMSNorm weights ones (the fold is then the identity): an MXFP8 engine loaded with W against a bf16 engine loaded with mx8(W)."""
    from chatterbox_vllm2_amd.weights import synthetic_cond_emb
    proj = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
    W = [(n, torch.ones_like(t) if "layernorm" in n else t) for n, t in tiny_weights]
    Wq = [(n, mx8(t) if n.startswith("tfmr.layers.") and any(p in n for p in proj) else t) for n, t in W]
    cond = synthetic_cond_emb(1)
    reqs = [(i, make_prompt(n_text, seed=60 + i), dict(temperature=0.8, top_p=0.8, repetition_penalty=2.0, seed=3, uid=i, max_tokens=n, ignore_eos=True))
            for i, (n_text, n) in enumerate([(20, 40), (45, 25), (8, 12)])]

    def run(tensors, dtype, eager):
        eng = E.T3Engine(n_layers=2, text_vocab=704, max_model_len=192, max_seqs=4, kv_bytes=1 << 27, enforce_eager=eager, debug_logits=True, weight_dtype=dtype)
        eng.load_tensors(tensors); eng.finalize()
        for i, prompt, kw in reqs:
            eng.add_request(i, prompt, cond, E.make_sampling(**kw))
        eng.step()                                                   # prefill + first token
        first = [eng.debug_logits(i) for i, _, _ in reqs]
        for _ in range(6):
            eng.step()
        later = [eng.debug_logits(i) for i, _, _ in reqs]           # a decode step (replayed from the graph where the engine captures one)
        eng.run_until_done()
        ids = [eng.get_output(i)[0] for i, _, _ in reqs]
        nbytes = int(eng.stats().weight_bytes)
        eng.close()
        return ids, first + later, nbytes

    ids, lg, nbytes = run(W, "mxfp8", True)
    ids_g, lg_g, _ = run(W, "mxfp8", False)
    ids_b, lg_b, nbytes_b = run(Wq, "bf16", True)
    assert ids == ids_b and ids_g == ids_b and all(len(t) == kw["max_tokens"] for t, (_, _, kw) in zip(ids, reqs))
    for a, g, b in zip(lg, lg_g, lg_b):
        assert_bit_equal(a, b, "logits, launch by launch"); assert_bit_equal(g, b, "logits, graph replay")
    mat = 4 * 1024 * 1024 + 3 * 4096 * 1024                          # per layer: 2 bytes per weight -> 1 byte + a scale byte per 32
    assert nbytes == nbytes_b - 2 * (2 * mat) + 2 * (mat + mat // 32) and nbytes < nbytes_b
