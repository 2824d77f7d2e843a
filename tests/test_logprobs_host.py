"""Host side of the per-token log-probabilities (no GPU): the SamplingParams parameter, the ABI names, and the inputs and the float64 reference
the GPU test (test_gpu_logprobs.py) holds the kernel to."""
import warnings

import numpy as np
import pytest
import torch

V = 8194
CASES = ["normal-id0", "normal-tail", "five-values", "dominant", "minus-inf"]


def logits_case(case):
    """-> (logits2 bf16 [2, 8208] with a large finite junk value in the pad columns, the id taken as drawn)"""
    g = torch.Generator().manual_seed(CASES.index(case))
    cond, unc = torch.randn(V, generator=g) * 2, torch.randn(V, generator=g) * 2          # N(0, 4)
    token = {"normal-id0": 0, "normal-tail": V - 1}.get(case)
    if case == "five-values":          # x takes 5 values at either cfg (uncond = cond): ~1600 ids tie at the top, the top-20 sits inside that group
        cond = torch.randint(-2, 3, (V,), generator=g).float()
        unc = cond.clone()
        token = int((cond == 2).nonzero()[30])          # inside the top group, behind its first 20 ids
    elif case == "dominant":           # id 4000 at 0, the rest 80 +- 3 below: exp(x - M) underflows, some terms below the contract exp's cutoff of -87
        cond = -80 + torch.randn(V, generator=g) * 3
        cond[4000] = 0
        unc, token = cond.clone(), 17
    elif case == "minus-inf":          # cond -inf on 100 ids, uncond finite: x = -inf there at cfg 0.5 (and NaN at cfg 0: 0 * inf)
        cond[torch.randperm(V, generator=g)[:100]] = float("-inf")
        token = int(torch.isfinite(cond).nonzero()[7])
    l2 = torch.full((2, 8208), 3e38)
    l2[0, :V], l2[1, :V] = cond, unc
    return l2.to(torch.bfloat16), token


def ref64(x):
    """The reference: x fp32 [8194] -> (log-softmax in float64, the ids ordered by (x descending, id ascending))"""
    x64 = np.asarray(x, dtype=np.float64)
    m = x64.max()
    return x64 - (m + np.log(np.exp(x64 - m).sum())), np.lexsort((np.arange(len(x64)), -x64))


@pytest.mark.parametrize("cfg", [0.0, 0.5])
@pytest.mark.parametrize("case", CASES)
def test_reference_top_ids_are_unique_under_the_tie_rule(case, cfg):
    l2, token = logits_case(case)
    c, u = l2[0, :V], l2[1, :V]
    x = (c + (cfg * (c - u))).float().numpy()          # bf16 tensor arithmetic, one rounding per operation: what the sampler forms
    if case == "minus-inf" and cfg == 0.0:
        assert np.isnan(x).sum() == 100                  # outside the numeric contract: no reference
        return
    order = ref64(x)[1]
    a, b = order[:20], order[1:21]
    assert sorted(order.tolist()) == list(range(V)) and np.isfinite(x[token]) and ((x[a] > x[b]) | ((x[a] == x[b]) & (a < b))).all()


def test_sampling_params_logprobs():
    from chatterbox_vllm2_amd import engine
    from chatterbox_vllm2_amd.llm import SamplingParams
    with pytest.raises(ValueError):
        SamplingParams(logprobs=21)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert SamplingParams(logprobs=5).logprobs == 5 and SamplingParams().logprobs is None
    assert {"t3_reserve_logprobs", "t3_request_logprobs", "t3_get_logprobs", "t3k_logprobs"} <= set(engine.ABI_SYMBOLS)
