"""The MXFP4 KV pool against the oracle, BIT-EXACT: the pool stores dq4(x) of what the bf16 pool would store (DESIGN.md "Attention", MXFP4
pool: blocks of 32 head dims of one token, E8M0 scale 2^(max(E - 2, 0) - 127), E2M1 elements, round to nearest even, saturating), and the
kernels run the bf16 chain on the dequantised values, so the reference is the oracle's own rope / attn_row over dq4 of K and V."""
import numpy as np
import pytest
import torch

from util import assert_bit_equal, make_prompt, rand_bf16

pytestmark = pytest.mark.gpu
E2M1 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]


@pytest.fixture(scope="module")
def E():
    from chatterbox_vllm2_amd import engine
    engine.load_library()
    return engine


def dq4(t):
    """the stored value of t over its last axis in blocks of 32, in float64 arithmetic (every step is exact there)"""
    x = t.double().reshape(-1, 32)
    amax = x.abs().amax(1, keepdim=True)
    b = (((amax.float().view(torch.int32) >> 23) & 0xff) - 2).clamp(min=0)
    X = torch.ldexp(torch.ones_like(amax), b - 127)
    grid = torch.tensor(E2M1, dtype=torch.float64)
    dist = ((x.abs() / X).unsqueeze(-1) - grid).abs() + torch.tensor([0, 1, 0, 1, 0, 1, 0, 1]) * 1e-12      # a tie goes to the even code
    y = torch.copysign(grid[dist.argmin(-1)] * X, x)
    return y.reshape(t.shape).to(t.dtype)


def block(head, fill=0.0):
    return torch.tensor(list(head) + [fill] * (32 - len(head)), dtype=torch.float32)


def test_format_pin(E):
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    mids = f32([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])
    ties = torch.cat([mids, torch.nextafter(mids, f32(9.0)), torch.nextafter(mids, f32(0.0)), f32([4.0])]).tolist()      # 4.0 pins the scale at 1
    rows = []
    for s in (1.0, 2.0 ** -9, 2.0 ** 10, 2.0 ** -120):
        rows.append(block([v * s for v in E2M1] + [-v * s for v in E2M1]))               # every value, both signs, -0.0 among them
        rows.append(block([v * s for v in ties])); rows.append(block([-v * s for v in ties]))
    others = [0.3, -0.7, 1.1, 0.05, -1.6, 0.9]
    for amax in (1.9921875, 2.0, 1.75, 1.875, -1.9921875 * 2.0 ** -7, 1.75 * 2.0 ** 9):      # below / at a power of two, saturation after rounding
        rows.append(block([amax] + [o * abs(amax) / 2 for o in others]))
    rows.append(block([]))                                                                   # all zero
    rows.append(block([m * 2.0 ** -133 for m in (127, 1, -64, 96, 33, -5, 16, 8)]))          # amax is a bf16 subnormal
    rows.append(block([-0.0, 0.0, 1.0, -1e-30]))
    rows.append(block([2.0 ** 127, -2.0 ** 126, 1.5 * 2.0 ** 125, 0.9 * 2.0 ** 124, 1.25 * 2.0 ** 125, -2.0 ** 127, 1.0]))      # top of the scale range
    x = torch.stack(rows)
    assert_bit_equal(E.k_fp4_roundtrip(x), dq4(x), "MXFP4 round trip")


CTX = [1, 16, 17, 33, 63, 64, 65, 255, 256, 257, 300]


def scale_heads(t):
    """head 1 x1000, head 3 /512, head 5: dims 0..31 a factor 2^10 above dims 32..63 (two very different scales inside one head)"""
    t[..., 64:128] *= 1000; t[..., 192:256] /= 512; t[..., 320:352] *= 1024


@pytest.mark.parametrize("rows,waves,ctxs", [(2, 8, [CTX[j:j + 2] for j in range(0, 10, 2)] + [[300, 1]]), (2, 4, [CTX[j:j + 2] for j in range(0, 10, 2)] + [[300, 1]]),
                                             (9, 4, [CTX[:9], CTX[2:]]), (2, 4, [[1000, 937]])],
                         ids=["2rows-8waves", "2rows-4waves", "9rows-4waves", "long-2rows"])
def test_fused_decode_attention_fp4_bit_exact(E, oracle, rows, waves, ctxs):
    """Three consecutive fused launches per case (launch s reads what s - 1 wrote, positions 62 -> 64 and the block boundary among them):
    newest token only, word and piece edges, a chunk that holds only the newest token; the long case runs the two-tiles-in-flight loop."""
    steps, n_max = 3, max(max(c) for c in ctxs)
    max_pos = n_max + steps + 1
    cos_t, sin_t = oracle.rope_table(max_pos)
    ctx_qkv = rand_bf16(2, n_max, 3072, seed=rows + waves)
    scale_heads(ctx_qkv[..., 1024:2048]); scale_heads(ctx_qkv[..., 2048:])
    pos_all = torch.arange(n_max, dtype=torch.int32)
    Kc = [dq4(oracle.rope(ctx_qkv[c, :, 1024:2048], pos_all, cos_t, sin_t)) for c in range(2)]
    Vc = [dq4(ctx_qkv[c, :, 2048:].contiguous()) for c in range(2)]
    for j, ctx in enumerate(ctxs):
        new_qkv = rand_bf16(steps, rows, 3072, seed=100 * rows + j)
        scale_heads(new_qkv[..., 1024:2048]); scale_heads(new_qkv[..., 2048:])
        got, kv_got = E.k_decode_attention_fp4(ctx_qkv, new_qkv, ctx, max_pos, waves)
        want = torch.empty_like(got); kv_want = torch.empty_like(kv_got)
        for r in range(rows):
            n = ctx[r] - 1
            K = torch.cat([Kc[r % 2][:n], torch.zeros(steps, 1024, dtype=torch.bfloat16)]); V = torch.cat([Vc[r % 2][:n], torch.zeros(steps, 1024, dtype=torch.bfloat16)])
            for s in range(steps):
                p = torch.tensor([n + s], dtype=torch.int32)
                q = oracle.rope(new_qkv[s, r:r + 1, :1024], p, cos_t, sin_t)[0]
                K[n + s] = dq4(oracle.rope(new_qkv[s, r:r + 1, 1024:2048], p, cos_t, sin_t)[0]); V[n + s] = dq4(new_qkv[s, r, 2048:])
                kv_want[s, r, 0] = K[n + s]; kv_want[s, r, 1] = V[n + s]
                for h in range(16):
                    sl = slice(h * 64, (h + 1) * 64)
                    want[s, r, sl] = oracle.attn_row(q[sl], K[:n + s + 1, sl], V[:n + s + 1, sl])
        assert_bit_equal(kv_got, kv_want, f"stored newest K / V, contexts {ctx}")
        assert_bit_equal(got, want, f"fused mxfp4 decode attention, contexts {ctx}")


@pytest.mark.parametrize("lens", [[1], [65], [5, 130, 63, 200], [300, 2]])
def test_rope_paged_attention_fp4_bit_exact(E, oracle, lens):
    """Prefill path: RoPE + quantise + paged write (whole and ragged groups of eight V tokens), the 16-rows-per-workgroup attention over the
    MXFP4 pool, and the stored K / V of every position read back."""
    row_stream = [s for s, L in enumerate(lens) for _ in range(L)]; row_pos = [p for L in lens for p in range(L)]
    qkv = rand_bf16(len(row_pos), 3072, seed=sum(lens))
    scale_heads(qkv[:, 1024:2048]); scale_heads(qkv[:, 2048:])
    max_pos = max(lens) + 3
    got, kv_got = E.k_rope_attention_fp4(qkv, row_stream, row_pos, len(lens), max_pos)
    cos_t, sin_t = oracle.rope_table(max_pos)
    pos = torch.tensor(row_pos, dtype=torch.int32)
    q = oracle.rope(qkv[:, :1024], pos, cos_t, sin_t)
    k = dq4(oracle.rope(qkv[:, 1024:2048], pos, cos_t, sin_t)); v = dq4(qkv[:, 2048:].contiguous())
    assert_bit_equal(kv_got, torch.stack([k, v], dim=1), f"stored K / V lens={lens}")
    want = torch.empty_like(got)
    start = np.cumsum([0] + lens)
    for r, (s, p) in enumerate(zip(row_stream, row_pos)):
        ctx = slice(start[s], start[s] + p + 1)
        for h in range(16):
            sl = slice(h * 64, (h + 1) * 64)
            want[r, sl] = oracle.attn_row(q[r, sl], k[ctx, sl], v[ctx, sl])
    assert_bit_equal(got, want, f"mxfp4 prefill attention lens={lens}")


def test_alignment_tap_over_the_fp4_pool(E, oracle):
    """One ragged shape (two chunks and a part, a text span that crosses a chunk edge): the stored K is dq4 of the rotated K, and the tap's
    probabilities are the float64 softmax over it to the tolerance tests/test_gpu_alignment.py holds the bf16 and FP8 pools to."""
    L, head, lo, hi, TOL = 150, 7, 34, 104, 4e-6
    qkv = rand_bf16(L, 3072, seed=L)
    qkv[:, :2048] = rand_bf16(L, 2048, seed=L + 1, scale=3.0)
    got, q_rot, kv = E.k_attention_probs(qkv, [0] * L, list(range(L)), 1, L + 3, head, lo, hi, "mxfp4")
    cos_t, sin_t = oracle.rope_table(L + 3)
    assert_bit_equal(kv[:, 0].contiguous(), dq4(oracle.rope(qkv[:, 1024:2048], torch.arange(L, dtype=torch.int32), cos_t, sin_t)), "stored K")
    s = q_rot.double() @ kv[:, 0, head * 64:(head + 1) * 64].double().T / 8
    causal = torch.ones(L, L, dtype=torch.bool).tril()
    want = torch.softmax(s.masked_fill(~causal, float("-inf")), dim=1)[:, lo:hi]
    err = (got.double() - want).abs().max().item()
    print(f"alignment tap mxfp4: max |err| = {err:.3e}")
    assert err <= TOL
    assert (got[~causal[:, lo:hi]] == 0).all(), "positions beyond a row's context must be 0"


def test_engine_fp4_pool(E, tiny_weights):
    """2 layers, 3 utterances of different lengths generating across position 256 on an MXFP4 pool: ids do not depend on graph replay vs
    launch-by-launch steps nor on batch composition; the pool holds floor(kv_bytes / block bytes) blocks, at least 3.7 x (4096 / 1088 = 3.76,
    the bytes of a token in the two formats) those of a bf16 pool of the same bytes, and gives them all back; a bf16 engine in the same
    process still produces its own ids, replayed or launch by launch."""
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

    fp4, blocks4 = run("mxfp4", False, reqs)
    assert all(len(fp4[i]) == kw["max_tokens"] for i, _, kw in reqs)
    assert run("fp4", True, reqs)[0] == fp4, "graph replay vs enforce_eager"
    for rq in reqs:
        assert run("mxfp4", False, [rq])[0][rq[0]] == fp4[rq[0]], f"utterance {rq[0]} alone vs in the batch"
    bf16, blocks16 = run("bf16", False, reqs)
    block_bytes = 2 * 16 * (4 * (64 * 32 + 128) + 256)      # per layer: K and V, 16 heads, 4 chunks of nibbles + scales, the head padding
    assert blocks4 == (1 << 28) // (2 * block_bytes) and blocks4 >= 3.7 * blocks16
    assert bf16 == run("auto", True, reqs)[0]
