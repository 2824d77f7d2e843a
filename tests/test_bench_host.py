"""bench.py host logic that needs no GPU."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_more_ranks_than_gpus_is_refused_in_the_bench_own_words():
    """`--gpus N` on a node with fewer GPUs must stop with bench.py's message before any GPU call or rank is started
    (RCCL would fail inside init_process_group over duplicate devices).  This container has no GPU: N = 2 > 0."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "T3_BENCH_BACKEND")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "5"], env=env, capture_output=True, text=True, timeout=300)
    import torch
    if torch.cuda.device_count() >= 2:
        return
    assert p.returncode != 0 and "needs one GPU per rank" in p.stderr and "T3_BENCH_BACKEND=gloo" in p.stderr and "Traceback" not in p.stderr


def test_full_is_off_by_default_and_outputs_dump_as_float32(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import numpy as np
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert not a.full and a.dump_outputs is None and a.steps == 7 and a.warmup == 3
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", str(tmp_path)])
    a = bench.parse()
    assert a.full and a.dump_outputs == str(tmp_path) and a.steps == 800
    bench.dump_outputs(str(tmp_path / "a"), [[2501, 2502, 2503], [2600, 2601, 2602]], n_cols=3)
    tok, last = np.load(tmp_path / "a" / "tokens.npy"), np.load(tmp_path / "a" / "last_step_tokens.npy")
    assert tok.dtype == np.float32 and tok.tolist() == [[2501, 2502, 2503], [2600, 2601, 2602]] and last.tolist() == [2503, 2602]
    bench.dump_outputs(str(tmp_path / "b"), [[2501], [2600, 2601]])           # ragged (c4): padded with -1, lengths beside it
    assert np.load(tmp_path / "b" / "tokens.npy").tolist() == [[2501, -1], [2600, 2601]] and np.load(tmp_path / "b" / "lengths.npy").tolist() == [1, 2]


def test_steps_beyond_one_life_are_shared_among_lives_of_the_batch():
    """--steps sets the number of timed steps whatever it is: past the 856 decode steps a C3 utterance can take, the batch lives again."""
    sys.path.insert(0, ROOT)
    import bench
    for wl, mml, cap in (("c3", 1000, 856), ("c2", 400, 289)):
        for steps, warmup in ((1, 0), (20, 5), (cap, 0), (cap - 5, 5), (cap - 4, 5), (cap + 1, 0), (5000, 20), (12345, 7)):
            a = type("A", (), dict(workload=wl, max_model_len=mml, steps=steps, warmup=warmup, batch=32, layers=30))()
            lives = bench.plan_lives(a)
            spans = [last - first for _, first, last in lives]
            assert sum(spans) == steps and max(spans) - min(spans) <= 1 and len(lives) == -(-steps // (cap - warmup))
            for ff, first, last in lives:
                assert ff >= 0 and first == 1 + ff + warmup and last - 1 <= cap        # every life fits its utterances
            if len(lives) == 1:
                assert lives[0] == bench.plan_window(a)
            else:                                                                       # each window centred like a single one
                assert all(abs((first + last) // 2 - (mml - (141 if wl == "c3" else 108)) // 2) <= warmup // 2 + 1 for _, first, last in lives)
    assert " lives of the batch" in bench.workload_string(a, 1, 2, 3) and "lives" not in bench.workload_string(a, 1, 2)


def test_window_plans():
    sys.path.insert(0, ROOT)
    import bench
    a = type("A", (), dict(workload="c2", max_model_len=400, steps=200, warmup=20, batch=1, layers=30))()
    ff, first, last = bench.plan_window(a)
    assert last - first == 200 and first == 1 + ff + 20 and (first + last) // 2 in range(140, 152)          # centred on decode step 146 of 292
    assert bench.workload_string(a, first, last).startswith("C2:")
    a = type("A", (), dict(workload="c3", max_model_len=1000, steps=20, warmup=5, batch=32, layers=30))()
    ff, first, last = bench.plan_window(a)
    assert bench.workload_string(a, first, last).startswith("C3:") and abs((first + last) // 2 - 430) <= 2
