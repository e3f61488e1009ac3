"""Cost of --do_sample (profiles/sampling/README.md).

  python scripts/sampling_bench.py kernel            # fls_sample_rows next to fls_argmax_rows on the same
                                                     # rows: 160 x 32000 and 160 x 151936
  python scripts/sampling_bench.py gen [--gen 8]     # Llama-2-70B geometry resident in HBM, 32 prompts x 5
                                                     # suffixes: greedy and sampled generations alternated
                                                     # on one weight store (T 0.8, top_k 50, top_p 0.95)

The kernel rows are softmax outputs of random logits (std 4: a few hundred columns carry the mass,
the rest are tiny, as in a real row), written just before the timed launches so that they sit
in L2 / Infinity Cache as they do behind the LM head's softmax.
"""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PARAMS = dict(temperature=0.8, top_k=50, top_p=0.95, seed=0)


def _time(fn, iters):
    for _ in range(5):
        fn()
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(times)), float(min(times))


def kernel_bench(iters: int) -> None:
    from flexible_llm_sharding_amd.ops import get_ops
    from flexible_llm_sharding_amd.sampling import top_p_units, weight_table
    dev = torch.device("cuda", 0)
    ops = get_ops(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    for rows, V in ((160, 32000), (160, 151936)):
        probs = torch.softmax(torch.randn(rows, V, device=dev, generator=g) * 4, dim=-1).half()
        flat = torch.full((rows, V), 1.0 / V, device=dev).half()
        draws = torch.from_numpy(np.random.default_rng(0).integers(0, 1 << 64, rows, dtype=np.uint64).view(np.int64)).to(dev)
        nz = int((probs > 0).sum().item()) // rows
        out = {"rows": rows, "V": V, "bytes": rows * V * 2, "nonzero_per_row": nz, "iters": iters}
        out["argmax_us"] = _time(lambda: ops.argmax_rows(probs), iters)
        for name, T, k, p, x in (("sample_T0.8_k50_p0.95", 0.8, 50, 0.95, probs), ("sample_T1_k0_p1", 1.0, 0, 1.0, probs),
                                 ("sample_T1_k0_p0.9", 1.0, 0, 0.9, probs), ("sample_flat_row_T1", 1.0, 0, 1.0, flat)):
            table = torch.from_numpy(weight_table(T).view(np.int32)).to(dev)
            out[name + "_us"] = _time(lambda: ops.sample_rows(x, table, draws, k, top_p_units(p)), iters)
        print(json.dumps(out), flush=True)


def gen_bench(a) -> None:
    from flexible_llm_sharding_amd.api import generation_loop
    from flexible_llm_sharding_amd.config import preset
    from flexible_llm_sharding_amd.engine import ShardedRunner
    from flexible_llm_sharding_amd.parallel.comm import Comm
    from flexible_llm_sharding_amd.runtime.weights import HostStore
    from flexible_llm_sharding_amd.sampling import SamplingParams
    from flexible_llm_sharding_amd.utils.synthetic import synthetic_prompts
    from flexible_llm_sharding_amd.utils.tokenizer import load_tokenizer, write_synthetic_tokenizer
    dev = torch.device("cuda", 0)
    cfg = preset(a.model, **({} if a.num_layers is None else {"num_hidden_layers": a.num_layers}))
    store = HostStore.synthetic(cfg, dev, seed=0, fold_norms=True)
    tok_dir = f"/tmp/fls_sampling_bench_tok_{os.getpid()}"
    write_synthetic_tokenizer(tok_dir, cfg.vocab_size)
    tok = load_tokenizer(tok_dir)
    prompts = synthetic_prompts(a.prompts, 1024, 5, 64, cfg.vocab_size, seed=0)
    for rnd in range(a.rounds):
        for name in ("greedy", "sample"):
            args = argparse.Namespace(num_gen_token=a.gen, data_parallel=False, num_batch=1, do_sample=name == "sample",
                                      **(PARAMS if name == "sample" else {}))
            r = ShardedRunner(cfg, store, dev, tok, layer_num_per_shard=1, prefix_kv_cache=True, suffix_kv_cache=True,
                              resident=True, sampling=SamplingParams.from_args(args))
            step_s = []
            t = time.perf_counter()
            s, u = generation_loop(args, r, Comm(0, 1, dev), tok, prompts, step_s)
            res = {"arm": name, "round": rnd, "total_s": round(time.perf_counter() - t, 3),
                   "step_s": [round(x, 4) for x in step_s],
                   "later_step_s_median": round(float(np.median(step_s[2:])), 4) if len(step_s) > 2 else None,
                   "speculative_dropped": r.spec_dropped,
                   "last_step": {k: r.stats.get(k) for k in ("tokens", "speculative", "graph_replays")},
                   "finite": bool(all(np.isfinite(x.astype(np.float32)).all() for x in s))}
            print(json.dumps(res), flush=True)
            r.close()
            del r, s, u
            gc.collect()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "gen"])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--gen", type=int, default=8)
    ap.add_argument("--prompts", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--model", default="llama2-70b")
    ap.add_argument("--num-layers", type=int, default=None)
    a = ap.parse_args()
    kernel_bench(a.iters) if a.what == "kernel" else gen_bench(a)
