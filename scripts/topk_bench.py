"""Cost of --score_top_k (profiles/topk/README.md).

  python scripts/topk_bench.py kernel            # fls_topk_rows (K = 1, 20, 1024) next to fls_argmax_rows and
                                                 # fls_sample_rows on the same rows: 160 x 32000 and 160 x 151936
  python scripts/topk_bench.py gen [--gen 8]     # Llama-2-70B geometry resident in HBM, 32 prompts x 5 suffixes:
                                                 # generations without and with --score_top_k 20 alternated on
                                                 # one weight store; step times and score D2H bytes per step

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
    return round(float(np.median(times)), 1), round(float(min(times)), 1)


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
        table = torch.from_numpy(weight_table(0.8).view(np.int32)).to(dev)
        picked = ops.argmax_rows(probs)
        nz = int((probs > 0).sum().item()) // rows
        out = {"rows": rows, "V": V, "bytes": rows * V * 2, "nonzero_per_row": nz, "iters": iters}
        # two rounds, the kernels alternated inside each
        for rnd in range(2):
            out[f"argmax_us_r{rnd}"] = _time(lambda: ops.argmax_rows(probs), iters)
            out[f"sample_T0.8_k50_p0.95_us_r{rnd}"] = _time(
                lambda: ops.sample_rows(probs, table, draws, 50, top_p_units(0.95)), iters)
            for K in (1, 20, 1024):
                out[f"topk_K{K}_us_r{rnd}"] = _time(lambda: ops.topk_rows(probs, K, picked=picked), iters)
            out[f"topk_K20_flat_row_us_r{rnd}"] = _time(lambda: ops.topk_rows(flat, 20, picked=picked), iters)
        print(json.dumps(out), flush=True)


def gen_bench(a) -> None:
    from flexible_llm_sharding_amd.api import generation_loop
    from flexible_llm_sharding_amd.config import preset
    from flexible_llm_sharding_amd.engine import ShardedRunner
    from flexible_llm_sharding_amd.parallel.comm import Comm
    from flexible_llm_sharding_amd.runtime.weights import HostStore
    from flexible_llm_sharding_amd.utils.synthetic import synthetic_prompts
    from flexible_llm_sharding_amd.utils.tokenizer import load_tokenizer, write_synthetic_tokenizer
    dev = torch.device("cuda", 0)
    cfg = preset(a.model, **({} if a.num_layers is None else {"num_hidden_layers": a.num_layers}))
    store = HostStore.synthetic(cfg, dev, seed=0, fold_norms=True)
    tok_dir = f"/tmp/fls_topk_bench_tok_{os.getpid()}"
    write_synthetic_tokenizer(tok_dir, cfg.vocab_size)
    tok = load_tokenizer(tok_dir)
    prompts = synthetic_prompts(a.prompts, 1024, 5, 64, cfg.vocab_size, seed=0)
    updated = {}
    for rnd in range(a.rounds):
        for name, K in (("full", 0), ("top_k", a.k)):
            args = argparse.Namespace(num_gen_token=a.gen, data_parallel=False, num_batch=1, do_sample=False)
            r = ShardedRunner(cfg, store, dev, tok, layer_num_per_shard=1, prefix_kv_cache=True, suffix_kv_cache=True,
                              resident=True, score_top_k=K)
            step_s = []
            t = time.perf_counter()
            s, u = generation_loop(args, r, Comm(0, 1, dev), tok, prompts, step_s)
            updated.setdefault(name, u)
            res = {"arm": name, "k": K, "round": rnd, "total_s": round(time.perf_counter() - t, 3),
                   "step_s": [round(x, 4) for x in step_s],
                   "later_step_s_median": round(float(np.median(step_s[2:])), 4) if len(step_s) > 2 else None,
                   "speculative_dropped": r.spec_dropped,
                   "last_step": {k: r.stats.get(k) for k in ("tokens", "speculative", "graph_replays")},
                   "score_d2h_bytes_per_step": r.score_d2h_bytes,
                   "output_bytes": int(sum(x.nbytes for x in s)),
                   "same_prompts_as_full": u == updated["full"]}
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
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--prompts", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--model", default="llama2-70b")
    ap.add_argument("--num-layers", type=int, default=None)
    a = ap.parse_args()
    kernel_bench(a.iters) if a.what == "kernel" else gen_bench(a)
