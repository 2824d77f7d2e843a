"""Host-side logic without a GPU: prompt assembly (t3.py:189-221), tokenizer goldens (data from the reference's
tokenizer files), the vLLM-shaped parameter validation, weight naming, and the data-parallel sharding over gloo."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the reference's two tokenizer vocabulary files (t3/tokenizer.json, t3/grapheme_mtl_merged_expanded_v1.json), byte for byte
EN_VOCAB, MTL_VOCAB = os.path.join(G, "vocab_en_tokenizer.json"), os.path.join(G, "vocab_grapheme_mtl_merged_expanded_v1.json")


def test_prompt_assembly_layout():
    from chatterbox_vllm2_amd.prompt import assemble_prompt_ids, build_mm_tensor
    ids = [255, 7, 9, 0]
    p = assemble_prompt_ids(ids)
    assert p == [695] + [255] * 32 + [696] + ids + [697] and len(p) == 34 + len(ids) + 1
    mm = build_mm_tensor(torch.ones(34, 1024) * 3, len(ids))
    assert mm.shape == (len(p), 1024)
    assert (mm[:34] == 3).all() and not mm[-1].any()
    assert [int(r.sum()) for r in mm[34:-1]] == [1, 2, 3, 4]          # row j carries j+1 ones (t3.py:94-102, read back at :621)
    with pytest.raises(ValueError):
        assemble_prompt_ids([])


def test_tokenizer_goldens():
    """Token ids of the fixed utterances, re-derived from the committed copies of the reference's vocabulary files."""
    tok = json.load(open(os.path.join(G, "tokenizer.json")))
    assert len(tok["en_english_ids"]) == 73 and tok["en_english_ids"][0] == 255 and tok["en_english_ids"][-1] == 0
    assert len(tok["en_mtl_ids"]) == 81 and len(tok["es_mtl_ids"]) == 106
    assert tok["en_mtl_ids"][0] == tok["lang"]["[en]"] == 708 and tok["es_mtl_ids"][0] == tok["lang"]["[es]"] == 635
    assert tok["special"] == {"[START]": 255, "[STOP]": 0, "[SPACE]": 2, "[UNK]": 1, "[PLACEHOLDER55]": 695, "[PLACEHOLDER56]": 696, "[PLACEHOLDER57]": 697}
    assert tok["en_vocab"] == 704 and tok["mtl_vocab"] == 2454
    from chatterbox_vllm2_amd.prompt import TextTokenizer
    en = TextTokenizer("EnTokenizer", EN_VOCAB)
    assert en.encode("[START]" + tok["en_text"] + "[STOP]") == tok["en_english_ids"]
    mtl = TextTokenizer("MtlTokenizer", MTL_VOCAB)
    assert mtl.encode("<es>[START]" + tok["es_text"] + "[STOP]") == tok["es_mtl_ids"]
    # quirk: the multilingual path lower-cases the whole string, so [START]/[STOP] are NOT ids 255/0 there
    assert 255 not in tok["en_mtl_ids"]


def test_tokenizer_matches_reference_classes():
    """prompt string -> ids.  tests/golden/tokenizer_cases.json holds the ids the reference's own
    EnTokenizer / MTLTokenizer classes produced (make_golden.py g7b); the vocabulary JSON files those classes read are
    committed beside it (tests/golden/vocab_*.json, the reference's data files unchanged), so the comparison runs everywhere.
    zh / ja / he / ru normalisers need absent packages: parity unpinned for those."""
    cases = json.load(open(os.path.join(G, "tokenizer_cases.json")))
    assert len(cases["en"]) >= 10 and len(cases["mtl"]) >= 10
    for c in cases["en"]:
        assert c["ids"][0] == 255 and c["ids"][-1] == 0                       # [START] ... [STOP]
    for c in cases["mtl"]:
        assert 255 not in c["ids"]                                            # lower-cased "[start]" is spelled out in pieces
    second = next(c for c in cases["mtl"] if "a > b" in c["prompt"])
    assert len(second["ids"]) == 8                                            # text.split('>')[1]: everything after the 2nd '>' is dropped
    from chatterbox_vllm2_amd.prompt import build_prompt_strings, punc_norm
    for c in cases["punc_norm"]:                                              # outputs of the reference's text_utils.punc_norm
        assert punc_norm(c["text"]) == c["out"], repr(c["text"])
    assert build_prompt_strings(["hi there"], "ES", multilingual=True) == ["<es>[START]Hi there.[STOP]"]      # tts.py:435-441
    assert build_prompt_strings(["hi there"]) == ["[START]Hi there.[STOP]"]
    from chatterbox_vllm2_amd.prompt import TextTokenizer
    en = TextTokenizer("EnTokenizer", EN_VOCAB)
    mtl = TextTokenizer("MtlTokenizer", MTL_VOCAB)
    for c in cases["en"]:
        assert en.encode(c["prompt"]) == c["ids"], c["prompt"]
    for c in cases["mtl"]:
        assert mtl.encode(c["prompt"]) == c["ids"], c["prompt"]


def test_sampling_params_validation():
    from chatterbox_vllm2_amd.llm import SamplingParams
    sp = SamplingParams(temperature=0.8, stop_token_ids=[9062], max_tokens=1000, top_p=0.8, repetition_penalty=2.0)
    assert sp.top_k == 0 and sp.min_p == 0.0 and sp.seed is None
    for bad in (dict(temperature=-1), dict(top_p=0), dict(top_p=1.5), dict(top_k=-2), dict(min_p=2), dict(max_tokens=0), dict(n=2)):
        with pytest.raises(ValueError):
            SamplingParams(**bad)
    with pytest.raises(TypeError):
        SamplingParams(not_a_vllm_field=1)


def test_synthetic_weights_are_deterministic_and_complete():
    from chatterbox_vllm2_amd.weights import synthetic_tensors
    a = dict(synthetic_tensors(1, 704, 1234)); b = dict(synthetic_tensors(1, 704, 1234))
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    assert a["speech_head.weight"].shape == (8194, 1024) and a["speech_pos_emb.emb.weight"].shape == (4100, 1024)
    assert a["tfmr.layers.0.mlp.down_proj.weight"].shape == (1024, 4096) and a["text_emb.weight"].dtype == torch.bfloat16
    n = sum(v.numel() for k, v in a.items() if k.startswith("tfmr.layers.0."))
    assert n == 16779264                              # per-layer parameter count


def test_shard_indices_balanced_and_complete():
    from chatterbox_vllm2_amd.dp import shard_indices
    costs = [100, 1, 1, 1, 50, 50, 2, 2]
    sh = shard_indices(costs, 2)
    assert sorted(sh[0] + sh[1]) == list(range(8))
    loads = [sum(costs[i] for i in s) for s in sh]
    assert abs(loads[0] - loads[1]) <= 4
    assert shard_indices([1.0] * 7, 3) == [[0, 3, 6], [1, 4], [2, 5]]
    assert shard_indices([], 4) == [[], [], [], []]


_DP_WORKER = r'''
import os, sys
sys.path.insert(0, sys.argv[1])
import torch.distributed as dist
from chatterbox_vllm2_amd.dp import generate_sharded
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
costs = [116 + 884, 141 + 859, 50, 700, 300, 20, 999]
def fake_generate(idxs):                 # stands in for the engine: tokens depend on the GLOBAL utterance id only
    return [[2500 + (i * 31 + t) % 6000 for t in range(3 + i)] for i in idxs]
mine, res = generate_sharded(fake_generate, len(costs), costs, rank, world)
single = fake_generate(list(range(len(costs))))
assert res == single, (rank, res)
dist.barrier(); dist.destroy_process_group()
print("rank", rank, "ok", mine)
'''


def test_data_parallel_sharding_world2_gloo(tmp_path):
    """world_size-2 gloo run: shards are disjoint + complete and the gathered result equals the 1-process result."""
    script = tmp_path / "w.py"; script.write_text(_DP_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29561", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script), ROOT], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    outs = [p.communicate(timeout=120)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert all("ok" in o for o in outs)


def test_strict_tokenizer_refuses_unpinned_languages(tmp_path):
    """zh / ja / he / ru need normalisers (mtltokenizer.py:311-320) that cannot run here: refuse rather than emit other ids."""
    from chatterbox_vllm2_amd.prompt import TextTokenizer
    strict, loose = TextTokenizer("MtlTokenizer", MTL_VOCAB), TextTokenizer("MtlTokenizer", MTL_VOCAB, strict=False)
    for lang in ("zh", "ja", "he", "ru"):
        with pytest.raises(ValueError):
            strict.encode(f"<{lang}>[START]x[STOP]")
        assert len(loose.encode(f"<{lang}>[START]x[STOP]")) > 3
    assert strict.encode("<fr>[START]oui[STOP]") == loose.encode("<fr>[START]oui[STOP]")


def test_c4_fixture_shape():
    c4 = json.load(open(os.path.join(G, "c4_requests.json")))
    reqs = c4["requests"]
    assert len(reqs) == 499 and {r["lang"] for r in reqs} == {"en", "fr", "zh"}
    for r in reqs:
        T = 34 + len(r["text_ids"]) + 1
        assert 200 <= r["max_tokens"] <= 800 and T + r["max_tokens"] <= c4["max_model_len"] - 1 + 1
        assert all(0 <= t < 2454 for t in r["text_ids"])


def test_safetensors_iterator_yields_checkpoint_names(tmp_path):
    """weights.iter_safetensors: the real-checkpoint entry (tts.py:225-229 symlinks it to <model dir>/model.safetensors)."""
    from safetensors.torch import save_file
    from chatterbox_vllm2_amd.weights import iter_safetensors, synthetic_tensors
    sd = {k: v.contiguous() for k, v in synthetic_tensors(1, 704, 1234)}
    sd["text_head.weight"] = torch.zeros(704, 1024)              # fp32 extras are cast on the way in
    d = tmp_path / "m"; d.mkdir(); save_file(sd, str(d / "model.safetensors"))
    got = dict(iter_safetensors(str(d)))
    assert set(got) == set(sd) and all(t.dtype == torch.bfloat16 for t in got.values())
    assert torch.equal(got["tfmr.layers.0.mlp.down_proj.weight"], sd["tfmr.layers.0.mlp.down_proj.weight"])


def test_bench_window_is_centred_and_self_launching(monkeypatch, capsys):
    """bench.py: the timed window sits on the run midpoint whatever --steps is, and `--gpus N` without a launcher starts the ranks."""
    import importlib, types
    bench = importlib.import_module("bench")
    centres = []
    for steps, warmup in ((20, 5), (800, 20), (200, 0), (1, 0)):
        a = types.SimpleNamespace(steps=steps, warmup=warmup, max_model_len=1000, batch=32, layers=30)
        ff, first, last = bench.plan_window(a)
        assert ff >= 0 and last <= 1000 - 141 - 3 + 1
        centres.append((first + last - 1) / 2)
    assert max(centres) - min(centres) <= 2.0 and abs(centres[0] - 430) <= 2.0          # C3 mean context 128.5 + ~430
    assert "C3" in bench.workload_string(types.SimpleNamespace(steps=20, warmup=5, max_model_len=1000, batch=32, layers=30), 1, 2)
    assert "custom" in bench.workload_string(types.SimpleNamespace(steps=20, warmup=5, max_model_len=400, batch=1, layers=30), 1, 2)
    seen = {}
    def fake_run(cmd, **kw):
        seen["cmd"] = cmd
        return types.SimpleNamespace(returncode=0, stdout='noise\n{"metric": "m", "value": 1}\n')
    monkeypatch.setattr(bench.subprocess, "run", fake_run)
    monkeypatch.setenv("T3_BENCH_BACKEND", "gloo")          # (under nccl, more ranks than GPUs is refused before anything is started: tests/test_bench_host.py)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "20", "--warmup", "5"])
    with pytest.raises(SystemExit) as ex:
        bench.spawn_ranks(types.SimpleNamespace(gpus=4))
    assert ex.value.code == 0
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node=4" in cmd and "127.0.0.1" in cmd and cmd[-6:] == ["--gpus", "4", "--steps", "20", "--warmup", "5"]
    assert capsys.readouterr().out.strip() == '{"metric": "m", "value": 1}'
