"""Host side of the MXFP4 KV pool switch (no GPU): the names, the environment default, the C struct field's new value, the new symbols."""
import ctypes

import pytest


@pytest.mark.parametrize("name", ["mxfp4", "fp4"])
def test_kv_cache_dtype_names(name, monkeypatch):
    from chatterbox_vllm2_amd import engine
    assert engine.kv_cache_dtype_code(name) == 4
    monkeypatch.setenv("T3_KV_CACHE_DTYPE", name)
    assert engine.kv_cache_dtype_code(None) == 4


def test_code_4_passes_argument_validation():
    from chatterbox_vllm2_amd import engine
    lib = engine.load_library()
    cfg = engine.T3EngineConfig(0, 1, 704, 64, 1, 0, 1 << 26, 0.9, 0.5, 1, 0, 0, 4)
    h = ctypes.c_void_p()
    rc = lib.t3_create(ctypes.byref(cfg), ctypes.byref(h))
    if rc == engine.T3_OK:
        lib.t3_destroy(h)
    else:
        assert rc == engine.T3_E_DEVICE and b"no HIP device" in lib.t3_last_error(None)


def test_new_symbols_are_part_of_the_abi():
    from chatterbox_vllm2_amd import engine
    lib = engine.load_library()
    for name in ("t3k_fp4_roundtrip", "t3k_rope_attention_fp4", "t3k_decode_attention_fp4"):
        assert name in engine.ABI_SYMBOLS and hasattr(lib, name)
