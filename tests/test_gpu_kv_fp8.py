"""The FP8 (E4M3FN) KV pool against the oracle, BIT-EXACT: the pool stores q8(x) = e4m3fn(rne(clamp(x, -448, 448))) of what the bf16 pool
would store, and the kernels run the bf16 chain on the dequantised values (DESIGN.md "Attention"), so the reference is the oracle's own
rope / attn_row over K / V that went through torch's CPU e4m3fn cast."""
import numpy as np
import pytest
import torch

from util import assert_bit_equal, make_prompt, rand_bf16

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    from chatterbox_vllm2_amd import engine
    engine.load_library()
    return engine


def dq8(t):
    """what the FP8 pool hands back for a stored tensor: torch's CPU cast there and back"""
    return t.float().clamp(-448, 448).to(torch.float8_e4m3fn).to(t.dtype)


def test_format_pin(E):
    """The hardware convert is torch's CPU e4m3fn cast: every bf16 value up to |x| = 1024 (subnormals, ties, both zeros, saturation
    beyond 448) and fp32 halfway points between neighbouring e4m3 values (normal, subnormal, the tie at half the smallest subnormal)."""
    allbf = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).float()
    half = torch.tensor([1.0625, 1.1875, 1.0625 + 2 ** -20, 1.0625 - 2 ** -20, 2.0 ** -10, 3 * 2.0 ** -10, 5 * 2.0 ** -10, 2.0 ** -10 + 2.0 ** -30,
                         0.0166015625, 432.0, 447.999, 464.0, 0.0068359375])
    x = torch.cat([allbf[allbf.abs() <= 1024], half, -half])
    assert_bit_equal(E.k_fp8_roundtrip(x), dq8(x), "q8 round trip")


CTX = [1, 16, 17, 33, 63, 64, 65, 255, 256, 257, 300]


@pytest.mark.parametrize("rows,waves,ctxs", [(2, 8, [CTX[j:j + 2] for j in range(0, 10, 2)] + [[300, 1]]), (2, 4, [CTX[j:j + 2] for j in range(0, 10, 2)] + [[300, 1]]),
                                             (9, 4, [CTX[:9], CTX[2:]]), (2, 4, [[1000, 937]])],
                         ids=["2rows-8waves", "2rows-4waves", "9rows-4waves", "long-2rows"])
def test_fused_decode_attention_fp8_bit_exact(E, oracle, rows, waves, ctxs):
    """Three consecutive fused launches per case (launch s reads what s - 1 wrote, positions 62 -> 64 among them): newest token only, piece
    and half-piece edges, a chunk that holds only the newest token, the block boundary; the long case runs the two-tiles-in-flight loop
    beyond four chunks per wave.  One head of K and of V is scaled x1000 (saturation), another x1/512 (fp8 subnormals)."""
    steps, n_max = 3, max(max(c) for c in ctxs)
    max_pos = n_max + steps + 1
    cos_t, sin_t = oracle.rope_table(max_pos)
    ctx_qkv = rand_bf16(2, n_max, 3072, seed=rows + waves)
    for t in (ctx_qkv[..., 1024:2048], ctx_qkv[..., 2048:]):
        t[..., 64:128] *= 1000; t[..., 192:256] /= 512
    pos_all = torch.arange(n_max, dtype=torch.int32)
    Kc = [dq8(oracle.rope(ctx_qkv[c, :, 1024:2048], pos_all, cos_t, sin_t)) for c in range(2)]
    Vc = [dq8(ctx_qkv[c, :, 2048:].contiguous()) for c in range(2)]
    for j, ctx in enumerate(ctxs):
        new_qkv = rand_bf16(steps, rows, 3072, seed=100 * rows + j)
        for t in (new_qkv[..., 1024:2048], new_qkv[..., 2048:]):
            t[..., 64:128] *= 1000; t[..., 192:256] /= 512
        got, kv_got = E.k_decode_attention_fp8(ctx_qkv, new_qkv, ctx, max_pos, waves)
        want = torch.empty_like(got); kv_want = torch.empty_like(kv_got)
        for r in range(rows):
            n = ctx[r] - 1
            K = torch.cat([Kc[r % 2][:n], torch.zeros(steps, 1024, dtype=torch.bfloat16)]); V = torch.cat([Vc[r % 2][:n], torch.zeros(steps, 1024, dtype=torch.bfloat16)])
            for s in range(steps):
                p = torch.tensor([n + s], dtype=torch.int32)
                q = oracle.rope(new_qkv[s, r:r + 1, :1024], p, cos_t, sin_t)[0]
                K[n + s] = dq8(oracle.rope(new_qkv[s, r:r + 1, 1024:2048], p, cos_t, sin_t)[0]); V[n + s] = dq8(new_qkv[s, r, 2048:])
                kv_want[s, r, 0] = K[n + s]; kv_want[s, r, 1] = V[n + s]
                for h in range(16):
                    sl = slice(h * 64, (h + 1) * 64)
                    want[s, r, sl] = oracle.attn_row(q[sl], K[:n + s + 1, sl], V[:n + s + 1, sl])
        assert_bit_equal(kv_got, kv_want, f"stored newest K / V, contexts {ctx}")
        assert_bit_equal(got, want, f"fused fp8 decode attention, contexts {ctx}")


@pytest.mark.parametrize("lens", [[1], [65], [5, 130, 63, 200], [300, 2]])
def test_rope_paged_attention_fp8_bit_exact(E, oracle, lens):
    """Prefill path: RoPE + quantise + paged write (aligned 8-row V transposes and ragged single-byte rows), the 16-rows-per-workgroup
    attention over the FP8 pool, and the stored K / V of every position read back."""
    row_stream = [s for s, L in enumerate(lens) for _ in range(L)]; row_pos = [p for L in lens for p in range(L)]
    qkv = rand_bf16(len(row_pos), 3072, seed=sum(lens))
    for t in (qkv[:, 1024:2048], qkv[:, 2048:]):
        t[:, 64:128] *= 1000; t[:, 192:256] /= 512
    max_pos = max(lens) + 3
    got, kv_got = E.k_rope_attention_fp8(qkv, row_stream, row_pos, len(lens), max_pos)
    cos_t, sin_t = oracle.rope_table(max_pos)
    pos = torch.tensor(row_pos, dtype=torch.int32)
    q = oracle.rope(qkv[:, :1024], pos, cos_t, sin_t)
    k = dq8(oracle.rope(qkv[:, 1024:2048], pos, cos_t, sin_t)); v = dq8(qkv[:, 2048:].contiguous())
    assert_bit_equal(kv_got, torch.stack([k, v], dim=1), f"stored K / V lens={lens}")
    want = torch.empty_like(got)
    start = np.cumsum([0] + lens)
    for r, (s, p) in enumerate(zip(row_stream, row_pos)):
        ctx = slice(start[s], start[s] + p + 1)
        for h in range(16):
            sl = slice(h * 64, (h + 1) * 64)
            want[r, sl] = oracle.attn_row(q[r, sl], k[ctx, sl], v[ctx, sl])
    assert_bit_equal(got, want, f"fp8 prefill attention lens={lens}")


def test_engine_fp8_pool(E, tiny_weights):
    """2 layers, 3 utterances of different lengths generating across position 256 on an FP8 pool: ids do not depend on graph replay vs
    launch-by-launch steps nor on batch composition, the pool holds twice the blocks of a bf16 pool of the same bytes and gives them all
    back; a bf16 engine in the same process still produces its own ids, replayed or launch by launch."""
    from chatterbox_vllm2_amd.weights import synthetic_cond_emb
    cond = synthetic_cond_emb(1)
    reqs = [(i, make_prompt(n_text, seed=40 + i), dict(temperature=0.8, top_p=0.8, repetition_penalty=2.0, seed=7, uid=i, max_tokens=n, ignore_eos=True))
            for i, (n_text, n) in enumerate([(20, 215), (45, 190), (8, 60)])]

    def run(dtype, eager, subset):
        eng = E.T3Engine(n_layers=2, text_vocab=704, max_model_len=320, max_seqs=4, kv_bytes=1 << 28, enforce_eager=eager, kv_cache_dtype=dtype)
        eng.load_tensors(tiny_weights); eng.finalize()
        for i, prompt, kw in subset:
            eng.add_request(i, prompt, cond, E.make_sampling(**kw))
        eng.run_until_done()
        ids = {i: eng.get_output(i)[0] for i, _, _ in subset}
        for i in ids:
            eng.release(i)
        st = eng.stats()
        eng.close()
        assert st.kv_blocks_free == st.kv_blocks_total
        return ids, int(st.kv_blocks_total)

    fp8, blocks8 = run("fp8", False, reqs)
    assert all(len(fp8[i]) == kw["max_tokens"] for i, _, kw in reqs)
    assert run("fp8", True, reqs)[0] == fp8, "graph replay vs enforce_eager"
    for rq in reqs:
        assert run("fp8", False, [rq])[0][rq[0]] == fp8[rq[0]], f"utterance {rq[0]} alone vs in the batch"
    bf16, blocks16 = run("bf16", False, reqs)
    assert abs(blocks8 - 2 * blocks16) <= 1
    assert bf16 == run("auto", True, reqs)[0]
