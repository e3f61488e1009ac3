"""Cost of --score_mode loglik (profiles/loglik/README.md).

  python scripts/loglik_bench.py kernel              # fls_logprob_rows bytes/s at 1024 x 32000 / 151936
  python scripts/loglik_bench.py pass [--steps N]    # bench.py's headline configuration (Llama-2-70B
                                                     # geometry, 32 prompts of 1024 + 5 x 64 tokens,
                                                     # --max_vram_gb 6), loglik and next-token passes
                                                     # interleaved on one runner and one box

The pass comparison flips one runner between the modes (the three attributes the constructor
sets), so both modes see the same weights, allocator and weight slots; a VRAM-capped runner plans
every call anew, so each pass runs under its own mode's plan.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def kernel_bench(iters: int) -> None:
    from flexible_llm_sharding_amd.ops import get_ops
    dev = torch.device("cuda", 0)
    ops = get_ops(dev)
    for rows, V in ((1024, 32000), (1024, 151936)):
        x = (torch.randn(rows, V, device=dev) * 2).half()
        t = torch.randint(0, V, (rows,), device=dev, dtype=torch.int32)
        out = torch.empty(rows, 2, dtype=torch.float32, device=dev)
        for _ in range(5):
            ops.logprob_rows(x, t, out=out)
        times = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.logprob_rows(x, t, out=out)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e-3)
        med = float(np.median(times))
        print(json.dumps({"kernel": "fls_logprob_rows", "rows": rows, "V": V, "median_us": med * 1e6,
                          "min_us": min(times) * 1e6, "bytes": rows * V * 2, "TB_per_s_median": rows * V * 2 / med / 1e12,
                          "iters": iters}), flush=True)


def set_mode(r, loglik: bool) -> None:
    r.loglik = r.ctx.loglik = loglik
    r.score_mode = "loglik" if loglik else "next_token"
    r.ctx.prune_last = not loglik


def pass_bench(a) -> None:
    for k in ("PYTORCH_HIP_ALLOC_CONF", "PYTORCH_CUDA_ALLOC_CONF"):
        os.environ.setdefault(k, "expandable_segments:True")
    from flexible_llm_sharding_amd import knobs
    from flexible_llm_sharding_amd.config import preset
    from flexible_llm_sharding_amd.engine import ShardedRunner
    from flexible_llm_sharding_amd.runtime.weights import HostStore
    from flexible_llm_sharding_amd.utils.synthetic import synthetic_prompts
    from flexible_llm_sharding_amd.utils.tokenizer import clear_prefix_ids, load_tokenizer, write_synthetic_tokenizer
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = preset(a.model, **({} if a.num_layers is None else {"num_hidden_layers": a.num_layers}))
    store = HostStore.synthetic(cfg, dev, seed=0, fold_norms=knobs.get_int("FLS_QKV_FOLD") == 1)
    torch.cuda.empty_cache()
    tok_dir = f"/tmp/fls_loglik_bench_tok_{os.getpid()}"
    write_synthetic_tokenizer(tok_dir, cfg.vocab_size)
    tok = load_tokenizer(tok_dir)
    prompts = synthetic_prompts(32, 1024, 5, 64, cfg.vocab_size, seed=0)
    r = ShardedRunner(cfg, store, dev, tok, layer_num_per_shard=1, storage_location="cpu",
                      max_vram_gb=a.max_vram_gb or None)
    times = {"next_token": [], "loglik": []}
    for i in range(a.warmup + a.steps):
        for loglik in (False, True):
            set_mode(r, loglik)
            clear_prefix_ids()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            r(prompts)
            torch.cuda.synchronize(dev)
            dt = time.perf_counter() - t0
            if i >= a.warmup:
                times[r.score_mode].append(dt)
            print(f"[loglik_bench] step {i} {r.score_mode}: {dt:.3f}s plan={r.vram_plan}", flush=True)
    res = {m: {"median_s": float(np.median(v)), "min_s": min(v), "max_s": max(v), "n": len(v)} for m, v in times.items()}
    res["ratio_median"] = res["loglik"]["median_s"] / res["next_token"]["median_s"]
    res["config"] = {"model": a.model, "layers": cfg.num_hidden_layers, "prompts": 32, "tokens": 32 * (1024 + 320),
                     "pairs": 32 * 320, "max_vram_gb": a.max_vram_gb}
    print(json.dumps(res), flush=True)
    r.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "pass"])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--model", default="llama2-70b")
    ap.add_argument("--num-layers", type=int, default=None)
    ap.add_argument("--max-vram-gb", type=float, default=6.0)
    a = ap.parse_args()
    kernel_bench(a.iters) if a.what == "kernel" else pass_bench(a)
