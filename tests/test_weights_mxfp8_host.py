"""Host side of the MXFP8 weight option (no GPU): the finalize quantiser against a torch restatement of the format, the names, the new symbols."""
import pytest
import torch


def mx8(W: torch.Tensor) -> torch.Tensor:
    """The stored value of every weight: blocks of 32 along a row, scale byte b = max(E - 8, 0) from the block max's exponent field, E4M3 elements."""
    w = W.to(torch.bfloat16).float().reshape(-1, 32)
    b = (((w.abs().amax(1, keepdim=True).view(torch.int32) >> 23) & 0xff) - 8).clamp(min=0)
    X = torch.where(b > 0, (b << 23).view(torch.float32), torch.tensor(2.0 ** -127))
    q = (w / X).clamp(-448, 448).to(torch.float8_e4m3fn)
    return (q.float() * X).to(torch.bfloat16).reshape(W.shape)


def blocks_under_scale(vals: torch.Tensor, X: float) -> torch.Tensor:
    """vals * X in blocks of 31 values plus the anchor 448 X, which pins the block's scale to X"""
    v = torch.cat([vals, vals.new_zeros(-len(vals) % 31)]).reshape(-1, 31)
    return torch.cat([v, torch.full((len(v), 1), 448.0)], dim=1) * X


def test_roundtrip_equals_the_format_bit_for_bit():
    from chatterbox_vllm2_amd import engine
    from util import assert_bit_equal, rand_bf16
    e4 = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float()
    pos = e4[:127]                                                   # 0 .. 448, ascending
    grid = torch.cat([pos, (pos[:-1] + pos[1:]) / 2])                # every value and every halfway point (four mantissa bits: bf16 values)
    rnd = rand_bf16(64, 32, seed=1).float()
    below = rnd[:8].clamp(-200, 200).clone(); below[:, 0] = 255.0    # block max just below a power of two ...
    at = below.clone(); at[:, 0] = 256.0                             # ... and at it
    sat = blocks_under_scale(torch.tensor([449.0, 464.0, 480.0, 496.0, 510.0, -464.0, -510.0]), 1.0)
    sat[:, -1] = 496.0                                               # elements between 448 and 512: saturation behind the rounding
    zero = torch.zeros(2, 32); zero[0, ::3] = -0.0
    rows = torch.cat([blocks_under_scale(torch.cat([grid, -grid]), 2.0 ** -5), blocks_under_scale(grid, 2.0 ** 9), below, at, sat, zero,
                      rnd[8:24] * 1000, rnd[24:40] / 512, rnd[40:]]).to(torch.bfloat16)
    assert_bit_equal(engine.k_mxfp8_roundtrip(rows), mx8(rows), "mxfp8 round trip")
    wide = rows[: len(rows) // 4 * 4].reshape(-1, 128)               # several blocks per row
    assert_bit_equal(engine.k_mxfp8_roundtrip(wide), mx8(wide), "mxfp8 round trip, 4 blocks per row")


def test_new_symbols_are_part_of_the_abi():
    from chatterbox_vllm2_amd import engine
    lib = engine.load_library()
    for name in ("t3_set_weight_dtype", "t3k_mxfp8_roundtrip", "t3k_qkv_gemm_mx8", "t3k_silu_mul_gemm_mx8", "t3k_gemm_resid_mx8"):
        assert name in engine.ABI_SYMBOLS and hasattr(lib, name)
    assert lib.t3_set_weight_dtype(None, 1) == engine.T3_E_INVALID


def test_weight_dtype_names(monkeypatch):
    from chatterbox_vllm2_amd import engine
    from chatterbox_vllm2_amd.llm import LLM
    monkeypatch.delenv("T3_WEIGHT_DTYPE", raising=False)
    assert engine.weight_dtype_code(None) == 0 and engine.weight_dtype_code("bf16") == 0 and engine.weight_dtype_code("mxfp8") == 1
    monkeypatch.setenv("T3_WEIGHT_DTYPE", "mxfp8")
    assert engine.weight_dtype_code(None) == 1 and engine.weight_dtype_code("bf16") == 0
    for bad in ("fp8", "mxfp4", ""):
        with pytest.raises(ValueError, match="mxfp8"):
            engine.weight_dtype_code(bad)
    for bad in ("awq", "bf16"):
        with pytest.raises(ValueError, match="mxfp8"):
            LLM(model="", quantization=bad)
