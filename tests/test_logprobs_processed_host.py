"""Host side of the processed log-probabilities (no GPU): the ABI names, LLM(logprobs_mode=...), the error codes reachable without a device, and the
numpy restatement of the contract (include/t3_engine.h, "processed log-probabilities") that test_gpu_logprobs_processed.py holds the kernel to."""
import numpy as np
import pytest

from chatterbox_vllm2_amd import engine as E

V = 8194
f32 = np.float32


def ref_z(x, counts, sp, step=0, proc=None, stops=(), suppress=None):
    """Steps 2-5 of the contract in np.float32, one rounding per operation: x fp32 [8194] post-CFG, counts = what the step's sampler used, sp =
    (repetition_penalty, frequency_penalty, presence_penalty, temperature), proc = the make_logit_processors() keywords or None, stops = every stop
    id of the request, suppress = the id the guard holds at -inf or None."""
    x = np.array(x, dtype=f32)
    if proc:
        if proc.get("allowed_ids") is not None:
            x[np.setdiff1d(np.arange(V), proc["allowed_ids"])] = -np.inf
        for v, b in dict(proc.get("bias") or {}).items():
            x[v] = x[v] + f32(b)
        if step < proc.get("min_tokens", 0):
            x[list(stops)] = -np.inf
    if suppress is not None:
        x[suppress] = -np.inf
    rp, fp, pp, T = (f32(v) for v in sp)
    pos = np.asarray(counts) > 0
    y = x[pos] if rp == 1 else np.where(x[pos] > 0, x[pos] / rp, x[pos] * rp)
    y = y - fp * np.asarray(counts)[pos].astype(f32)
    x[pos] = y - pp
    return x / (T if T >= f32(1e-5) else f32(1))


def test_abi_and_mode_strings():
    assert {"t3_set_logprobs_mode", "t3k_logprobs_processed"} <= set(E.ABI_SYMBOLS)
    lib = E.load_library()
    assert lib.t3_set_logprobs_mode(None, 1) == -1 and lib.t3_set_logprobs_mode(None, 7) == -1          # T3_E_INVALID: no handle
    # the hook checks its arguments before it looks for a device: malformed is T3_E_INVALID everywhere
    assert lib.t3k_logprobs_processed(None, 8208, 0.5, None, None, None, -1, 8192, 0, 0, None, None, None, None) == -1


@pytest.mark.parametrize("mode", ["processed", "raw_logits", "processed_logits", None])
def test_llm_rejects_an_unknown_logprobs_mode(mode):
    from chatterbox_vllm2_amd import LLM
    with pytest.raises(ValueError, match="logprobs_mode"):
        LLM(model="", load_format="dummy", logprobs_mode=mode)
