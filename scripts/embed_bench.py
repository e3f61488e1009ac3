"""Cost of --score_mode embed (profiles/embed/README.md).

  python scripts/embed_bench.py kernel             # fls_pool_rows: 160 segments x 64 rows x 8192, bytes/s
  python scripts/embed_bench.py pass --mode M [--steps N]
        # bench.py's headline configuration (Llama-2-70B geometry, 32 prompts of 1024 + 5 x 64 tokens,
        # --max_vram_gb 6), M = next_token | embed_last | embed_mean (unpruned last layer) |
        # embed_mean_pruned (last layer pruned to the suffix rows): full passes of one mode

One mode per process: a VRAM cap (the allocator limit, the measured memory outside the allocator)
is per process, so every mode plans from the same clean state; run the modes one after another in
one job on one box to compare them.
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
    n_seg, n, H = 160, 64, 8192
    x = torch.randn(n_seg * n, H, device=dev).half()
    ss = torch.arange(0, n_seg * n + 1, n, dtype=torch.int32, device=dev)
    one = torch.arange(0, n_seg + 1, dtype=torch.int32, device=dev)
    for name, rows, seg, norm in (("mean", x, ss, False), ("mean+normalize", x, ss, True),
                                  ("last+normalize", x[:n_seg], one, True)):
        out = torch.empty(n_seg, H, dtype=torch.float32, device=dev)
        for _ in range(5):
            ops.pool_rows(rows, seg, 0, norm, out=out)
        times = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.pool_rows(rows, seg, 0, norm, out=out)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e-3)
        med, nbytes = float(np.median(times)), rows.numel() * 2
        print(json.dumps({"kernel": "fls_pool_rows", "case": name, "segments": n_seg, "rows": rows.shape[0], "H": H,
                          "median_us": med * 1e6, "min_us": min(times) * 1e6, "bytes_read": nbytes,
                          "TB_per_s_median": nbytes / med / 1e12, "iters": iters}), flush=True)


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
    tok_dir = f"/tmp/fls_embed_bench_tok_{os.getpid()}"
    write_synthetic_tokenizer(tok_dir, cfg.vocab_size)
    tok = load_tokenizer(tok_dir)
    prompts = synthetic_prompts(32, 1024, 5, 64, cfg.vocab_size, seed=0)
    kw = dict(layer_num_per_shard=1, storage_location="cpu", max_vram_gb=a.max_vram_gb or None)
    m = a.mode
    if m == "next_token":
        r = ShardedRunner(cfg, store, dev, tok, **kw)
    else:
        r = ShardedRunner(cfg, store, dev, tok, score_mode="embed", embed_pooling="last" if m == "embed_last" else "mean",
                          **kw)
        if m == "embed_mean_pruned":
            r.set_mean_variant(True)
    times = []
    for i in range(a.warmup + a.steps):
        clear_prefix_ids()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = r(prompts)
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        if i >= a.warmup:
            times.append(dt)
        print(f"[embed_bench] step {i} {m}: {dt:.3f}s d2h={r.score_d2h_bytes} plan={r.vram_plan}", flush=True)
    res = {"mode": m, "median_s": float(np.median(times)), "min_s": min(times), "max_s": max(times), "n": len(times),
           "score_d2h_bytes": r.score_d2h_bytes, "plan": r.vram_plan,
           "config": {"model": a.model, "layers": cfg.num_hidden_layers, "prompts": 32, "tokens": 32 * (1024 + 320),
                      "suffix_rows": 32 * 320, "max_vram_gb": a.max_vram_gb}}
    if a.save and m != "next_token":
        np.save(a.save, np.concatenate(out))
    print(json.dumps(res), flush=True)
    r.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "pass"])
    ap.add_argument("--mode", choices=["next_token", "embed_last", "embed_mean", "embed_mean_pruned"],
                    default="embed_last")
    ap.add_argument("--save", default=None, help="pass: write the embeddings here (.npy)")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--model", default="llama2-70b")
    ap.add_argument("--num-layers", type=int, default=None)
    ap.add_argument("--max-vram-gb", type=float, default=6.0)
    a = ap.parse_args()
    kernel_bench(a.iters) if a.what == "kernel" else pass_bench(a)
