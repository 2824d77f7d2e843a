"""Host side of the logit processors (no GPU): what SamplingParams accepts and rejects, the ABI names, and the error order of the C call."""
import ctypes as ct
import warnings

import pytest

from chatterbox_vllm2_amd import engine as E
from chatterbox_vllm2_amd.llm import SamplingParams

OFF, STOP = 2500, 9062


@pytest.mark.parametrize("kw", [
    dict(logit_bias={5: 1.0}), dict(allowed_token_ids=[2499]), dict(bad_words=[[100]]), dict(stop_token_ids=[STOP, 12]),      # ids below 2500
    dict(allowed_token_ids=[OFF + 8194]), dict(allowed_token_ids=[]),
    dict(bad_words=["word"]), dict(bad_words=[[OFF, OFF + 1]]),                                                                # no detokenizer
    dict(logit_bias={OFF + i: 1.0 for i in range(60)}, bad_words=[OFF + 100 + i for i in range(5)]),                           # 65 biased ids
    dict(logit_bias={OFF: float("inf")}), dict(logit_bias={OFF: float("nan")}),
    dict(min_tokens=-1), dict(min_tokens=17, max_tokens=16), dict(stop_token_ids=[STOP - i for i in range(5)]),
])
def test_rejected(kw):
    with pytest.raises(ValueError):
        SamplingParams(**kw)


def test_accepted_without_a_warning():
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert SamplingParams().processors is None and SamplingParams(stop_token_ids=[STOP]).processors is None
        sp = SamplingParams(logit_bias={STOP: 100.0, OFF + 3: -2.5}, bad_words=[[OFF + 1], OFF + 2], allowed_token_ids=[OFF + 9, OFF, STOP, OFF],
                            min_tokens=5, stop_token_ids=[STOP, OFF + 7], max_tokens=9)
    assert sp.processors == dict(allowed_ids=[0, 9, 6562], bias={6562: 100.0, 3: -2.5, 1: float("-inf"), 2: float("-inf")}, min_tokens=5,
                                 extra_stop_ids=[7])
    assert SamplingParams(logit_bias={OFF: 1e4}).processors["bias"] == {0: 1e4}          # not clamped: vLLM's constructor does not either
    lp = E.make_logit_processors(**sp.processors)
    assert (lp.struct_size, lp.n_allowed, lp.n_bias, lp.min_tokens, lp.n_extra_stop, lp.extra_stop_ids[0]) == (56, 3, 4, 5, 1, 7)


def test_abi():
    assert {"t3_reserve_logit_processors", "t3_request_logit_processors", "t3k_sample_proc"} <= set(E.ABI_SYMBOLS)
    lib = E.load_library()
    lp = E.make_logit_processors(bias={0: 1.0})
    assert lib.t3_request_logit_processors(None, 0, ct.byref(lp)) == -1 and lib.t3_reserve_logit_processors(None, 1) == -1      # T3_E_INVALID: no handle
    # the kernel hook checks the struct before it looks for a device: malformed is T3_E_INVALID everywhere
    for bad in (dict(bias=[(3, 1.0), (3, 2.0)]), dict(bias={8194: 0.0}), dict(bias={1: float("inf")}), dict(allowed_ids=[-1]), dict(min_tokens=-1),
                dict(extra_stop_ids=[9000])):
        assert lib.t3k_sample_proc(None, 8208, None, None, 0.5, 0, ct.byref(E.make_logit_processors(**bad)), None, None, None) == -1, bad
