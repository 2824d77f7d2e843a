"""Token time spans without a GPU: the ABI names, the kernel entry point's "no HIP device" error, and the SamplingParams keyword."""
import ctypes as ct

import pytest
import torch


def test_symbols_declared_and_exported():
    from chatterbox_vllm2_amd import engine
    lib = ct.CDLL(engine.LIB_PATH)
    for name in ("t3_get_token_spans", "t3k_align_path", "t3k_align_scores"):
        assert name in engine.ABI_SYMBOLS and hasattr(lib, name)


@pytest.mark.skipif(torch.cuda.is_available(), reason="needs a machine without a GPU")
def test_kernel_entry_point_has_no_cpu_fallback():
    from chatterbox_vllm2_amd import engine
    with pytest.raises(engine.T3Error, match="no usable HIP device"):
        engine.k_align_path(torch.full((4, 3), 0.5), 3)


def test_sampling_params_timestamps():
    from chatterbox_vllm2_amd.llm import CompletionOutput, SamplingParams
    sp = SamplingParams(timestamps=True)
    assert sp.timestamps and not sp.alignment and sp.alignment_guard is None
    assert not SamplingParams().timestamps and SamplingParams(alignment=True, timestamps=True).alignment
    assert SamplingParams(timestamps=True, alignment_guard=True, stop_token_ids=[9062], logprobs=2).alignment_guard == {}
    assert CompletionOutput(index=0, text="", token_ids=[]).timestamps is None
