"""What do per-token log-probabilities cost a decode step?  One engine, bench.py's C3 (or C2) window (fast-forward, warmup, K timed steps) run
with no request marked and with every request marked at k = 0 and k = 20 in raw and in processed mode (t3_set_logprobs_mode), the five passes
alternating `rounds` times in one process; prints the median / mean step time (t3_step_times) of every pass.  "off" runs first, before any reserve:
the engine as it is without the feature.
usage: python tools/logprobs_cost.py [steps] [rounds] [c3|c2]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import bench
from chatterbox_vllm2_amd import engine as E
from chatterbox_vllm2_amd.weights import synthetic_cond_emb, synthetic_tensors

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 400
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 2
c2 = len(sys.argv) > 3 and sys.argv[3] == "c2"
warm = 20
args = type("A", (), dict(workload="c2" if c2 else "c3", batch=1 if c2 else 32, max_model_len=400 if c2 else 1000, layers=30, steps=steps, warmup=warm,
                          vocab=704 if c2 else 2454))()
ff, first, last = bench.plan_window(args)
eng = E.T3Engine(n_layers=30, text_vocab=args.vocab, max_model_len=args.max_model_len, max_seqs=args.batch, gpu_memory_utilization=0.5, max_batched_rows=8192,
                 enforce_eager=False)
eng.load_tensors(list(synthetic_tensors(30, args.vocab, 1234))); eng.finalize()
cond = synthetic_cond_emb(1)
out = {"workload": args.workload, "steps": steps, "fast_forward": ff, "passes": []}
PASSES = (("off", None, None), ("raw k=0", "raw_logprobs", 0), ("processed k=0", "processed_logprobs", 0), ("raw k=20", "raw_logprobs", 20),
          ("processed k=20", "processed_logprobs", 20))
for rnd in range(rounds):
    for name, mode, k in PASSES:
        if k is not None and eng.logprobs_max_k < 20:
            eng.reserve_logprobs(20)
        if mode is not None:
            eng.set_logprobs_mode(mode)
        reqs = bench.build_requests(E, args, 0)
        for rid, prompt, sp in reqs:
            eng.add_request(rid, prompt, cond, sp)
            if k is not None:
                eng.request_logprobs(rid, k)
        while True:
            r = eng.step()
            if r.n_prefill_rows == 0 or r.n_waiting == 0 and r.n_sampled == len(reqs):
                break
        assert eng.run_steps(ff + warm) == ff + warm
        eng.reset_stats(); torch.cuda.synchronize()
        assert eng.run_steps(steps) == steps
        torch.cuda.synchronize()
        ms, _ = eng.step_times(steps)
        eng.run_until_done()
        for rid, _, _ in reqs:
            eng.release(rid)
        out["passes"].append({"pass": name, "round": rnd, "median_ms": round(float(np.median(ms)), 4), "mean_ms": round(float(ms.mean()), 4)})
print(json.dumps(out))
eng.close()
