"""Host side of the alignment export (no GPU): the flag travels from SamplingParams into T3Sampling.alignment."""
import torch


def test_make_sampling_alignment_word():
    from chatterbox_vllm2_amd import engine as E
    assert E.T3Sampling.alignment.offset == 60
    assert E.make_sampling().alignment == 0 and E.make_sampling(alignment=True).alignment == 1


def test_sampling_params_alignment_reaches_the_engine():
    from chatterbox_vllm2_amd.llm import LLM, CompletionOutput, SamplingParams

    class Recorder:                                  # stands in for T3Engine: what LLM._queue hands over
        def __init__(self):
            self.sps, self.reserved, self.alignment_max_text = [], [], 0

        def add_request(self, rid, ids, cond, sp):
            self.sps.append(sp)

        def reserve_alignment(self, n):
            self.reserved.append(n); self.alignment_max_text = n

    assert SamplingParams().alignment is False and CompletionOutput(0, "", []).alignment is None
    llm = LLM.__new__(LLM)
    llm.engine, llm.seed, llm._next_id, llm._next_uid, llm.max_model_len, llm.tokenizer = Recorder(), 0, 0, 0, 1000, None
    prompt = {"prompt_token_ids": [255, 5, 0], "multi_modal_data": {"conditionals": [torch.zeros(34, 1024)]}}
    llm._queue([prompt, prompt], [SamplingParams(alignment=True), SamplingParams()], None, [], [])
    assert [sp.alignment for sp in llm.engine.sps] == [1, 0] and llm.engine.reserved == [3]
    llm.engine = None                                # LLM.__del__ closes its engine
