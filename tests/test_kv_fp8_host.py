"""Host side of the FP8 KV pool switch (no GPU): vLLM's kv_cache_dtype names, the environment default, the C struct field."""
import ctypes
import warnings

import pytest


@pytest.mark.parametrize("name,code", [("auto", 0), ("bfloat16", 0), ("fp8", 1), ("fp8_e4m3", 1)])
def test_kv_cache_dtype_names(name, code, monkeypatch):
    from chatterbox_vllm2_amd import engine
    assert engine.kv_cache_dtype_code(name) == code
    monkeypatch.setenv("T3_KV_CACHE_DTYPE", name)
    assert engine.kv_cache_dtype_code(None) == code
    monkeypatch.delenv("T3_KV_CACHE_DTYPE")
    assert engine.kv_cache_dtype_code(None) == 0


@pytest.mark.parametrize("name", ["fp8_e5m2", "int8", ""])
def test_unknown_kv_cache_dtype_is_a_value_error(name):
    from chatterbox_vllm2_amd import engine
    from chatterbox_vllm2_amd.llm import LLM
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        engine.T3Engine(n_layers=1, kv_cache_dtype=name)
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        LLM(model="", kv_cache_dtype=name)


def test_llm_takes_the_keyword_without_a_warning():
    from chatterbox_vllm2_amd import engine
    from chatterbox_vllm2_amd.llm import LLM
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        with pytest.raises((engine.T3Error, ValueError), match="no HIP device|no checkpoint"):      # without / with a GPU: there is no such model directory
            LLM(model="/nonexistent", kv_cache_dtype="fp8", num_hidden_layers=1, max_model_len=64, max_num_seqs=1, kv_cache_bytes=1 << 26)
    assert not [w for w in seen if "kv_cache_dtype" in str(w.message)]


def test_config_field_and_its_validation():
    from chatterbox_vllm2_amd import engine
    assert ctypes.sizeof(engine.T3EngineConfig) == 56 and engine.T3EngineConfig.kv_cache_dtype.offset == 52
    lib = engine.load_library()
    cfg = engine.T3EngineConfig(0, 1, 704, 64, 1, 0, 1 << 26, 0.9, 0.5, 1, 0, 0, 2)
    h = ctypes.c_void_p()
    assert lib.t3_create(ctypes.byref(cfg), ctypes.byref(h)) == engine.T3_E_INVALID       # checked before the device is looked for
    assert b"kv_cache_dtype" in lib.t3_last_error(None)
