"""Cost of --score_mode classify (profiles/classify/README.md).

  python scripts/classify_bench.py kernel        # fls_classify_rows at 160 x 8192 x {1, 19} and 10,240 x 8192 x 1
  python scripts/classify_bench.py pass --mode classify_last | classify_all | embed_last [--steps N]
        # bench.py's headline configuration (Llama-2-70B geometry, 32 prompts of 1024 + 5 x 64 tokens,
        # --max_vram_gb 6): full passes of one mode, one mode per process (the cap is per process)
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
    H = 8192
    for rows, L in ((160, 1), (160, 19), (10240, 1)):
        x = torch.randn(rows, H, device=dev).half()
        w = (torch.randn(L, H, device=dev) * H ** -0.5).half()
        b = torch.randn(L, device=dev)
        out = torch.empty(rows, L, dtype=torch.float32, device=dev)
        for _ in range(5):
            ops.classify_rows(x, w, b, "none", out=out)
        times = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.classify_rows(x, w, b, "none", out=out)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e-3)
        med, nbytes = float(np.median(times)), x.numel() * 2
        print(json.dumps({"kernel": "fls_classify_rows", "rows": rows, "H": H, "L": L, "median_us": med * 1e6,
                          "min_us": min(times) * 1e6, "x_bytes": nbytes, "TB_per_s_median": nbytes / med / 1e12,
                          "iters": iters}), flush=True)


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
    names = cfg.layer_names()[:-1]
    store = HostStore.synthetic(cfg, dev, seed=0, names=names, fold_norms=knobs.get_int("FLS_QKV_FOLD") == 1)
    torch.cuda.empty_cache()
    tok_dir = f"/tmp/fls_classify_bench_tok_{os.getpid()}"
    write_synthetic_tokenizer(tok_dir, cfg.vocab_size)
    tok = load_tokenizer(tok_dir)
    prompts = synthetic_prompts(32, 1024, 5, 64, cfg.vocab_size, seed=0)
    kw = dict(layer_num_per_shard=1, storage_location="cpu", max_vram_gb=a.max_vram_gb or None)
    if a.mode == "embed_last":
        r = ShardedRunner(cfg, store, dev, tok, score_mode="embed", embed_pooling="last", **kw)
    else:
        r = ShardedRunner(cfg, store, dev, tok, score_mode="classify", classify_rows=a.mode.split("_")[1], **kw)
    times = []
    for i in range(a.warmup + a.steps):
        clear_prefix_ids()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        r(prompts)
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        if i >= a.warmup:
            times.append(dt)
        print(f"[classify_bench] step {i} {a.mode}: {dt:.3f}s d2h={r.score_d2h_bytes}", flush=True)
    print(json.dumps({"mode": a.mode, "median_s": float(np.median(times)), "min_s": min(times), "max_s": max(times),
                      "n": len(times), "score_d2h_bytes": r.score_d2h_bytes, "plan": r.vram_plan,
                      "num_labels": r.classify.num_labels if a.mode != "embed_last" else None}), flush=True)
    r.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "pass"])
    ap.add_argument("--mode", choices=["classify_last", "classify_all", "embed_last"], default="classify_last")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--model", default="llama2-70b")
    ap.add_argument("--num-layers", type=int, default=None)
    ap.add_argument("--max-vram-gb", type=float, default=6.0)
    a = ap.parse_args()
    kernel_bench(a.iters) if a.what == "kernel" else pass_bench(a)
