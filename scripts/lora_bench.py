"""Cost of merging a LoRA adapter as the weights land (profiles/lora/README.md).  Figures only.

  python scripts/lora_bench.py kernel [--iters N]
        # fls_lora_merge at r = 8 / 16 / 64 / 256 and fls_fold_norm (an in-place kernel with the same
        # weight traffic) on the 70B shapes 8192 x 8192, 10240 x 8192, 57344 x 8192 and 8192 x 28672:
        # median and minimum of N timed calls after 3 warm-up calls (device events around each call),
        # achieved read + write bytes/s of the weight (4 bytes per weight; the adapter's own bytes,
        # read from L2, are listed but not counted)
  python scripts/lora_bench.py write --dir D [--model llama2-70b] [--which fp16,int4] [--ranks 16,64]
        # synthetic checkpoints D/fp16 and D/int4 (one decoder layer file, the rest hard-linked) and
        # adapters D/lora_r16, D/lora_r64 on all seven targets
  python scripts/lora_bench.py pass --store stream_fp16|compact_int4|host_fp16 [--lora D/lora_r16] [--dir D]
                                    [--steps N] [--prompts P] [--max-vram-gb 6]
        # P prompts of 1,024 + 5 x 64 tokens, one layer per shard: tok/s, peak device memory
        # (hipMemGetInfo, sampled), merge launches and the planned chunk sizes; host_fp16 (the fp16
        # checkpoint pinned whole, 138 GB for 70B) also times the merge and the norm fold at build
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((8192, 8192), (10240, 8192), (57344, 8192), (8192, 28672))
RANKS = (8, 16, 64, 256)


def _time(fn, iters):
    times = []
    for i in range(iters + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= 3:
            times.append(e0.elapsed_time(e1) * 1e-3)
    return float(np.median(times)), min(times)


def kernel_bench(a) -> None:
    from flexible_llm_sharding_amd.ops import get_ops
    dev = torch.device("cuda", 0)
    ops = get_ops(dev)
    for rows, cols in SHAPES:
        n = rows * cols
        w = (torch.randn(n // 8, device=dev) * 0.02).half().repeat(8).view(rows, cols)
        gamma = (torch.rand(cols, device=dev) * 1e-3 + 1).half()           # (repeated folds stay finite)
        med, mn = _time(lambda: ops.fold_norm(w, gamma), a.iters)
        print(json.dumps({"kernel": "fls_fold_norm", "shape": [rows, cols], "median_us": med * 1e6, "min_us": mn * 1e6,
                          "weight_bytes": 4 * n, "TB_per_s_median": 4 * n / med / 1e12, "iters": a.iters}), flush=True)
        for r in RANKS:
            R = (r + 3) // 4 * 4
            A = torch.randn(R, cols, device=dev) * 0.01
            Bs = torch.randn(rows, R, device=dev) * 1e-3                  # (repeated merges stay finite)
            med, mn = _time(lambda: ops.lora_merge(w, A, Bs, r), a.iters)
            print(json.dumps({"kernel": "fls_lora_merge", "shape": [rows, cols], "r": r, "median_us": med * 1e6,
                              "min_us": mn * 1e6, "weight_bytes": 4 * n, "adapter_bytes": 4 * R * (rows + cols),
                              "TB_per_s_median": 4 * n / med / 1e12, "mfma_TFLOP_per_s": 2 * n * R / med / 1e12,
                              "iters": a.iters}), flush=True)
            del A, Bs
        del w


def _cfg(a):
    from flexible_llm_sharding_amd.config import preset
    return preset(a.model, **({} if a.num_layers is None else {"num_hidden_layers": a.num_layers}))


def write_bench(a) -> None:
    from flexible_llm_sharding_amd import lora
    from flexible_llm_sharding_amd.utils.synthetic import write_synthetic_checkpoint
    cfg = _cfg(a)
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    for sub in a.which.split(","):
        t0 = time.perf_counter()
        write_synthetic_checkpoint(cfg, os.path.join(a.dir, sub), seed=0, unique_layers=1, device=dev,
                                   quantize=None if sub == "fp16" else sub, int4_group=128)
        print(f"[lora_bench] wrote {sub} in {time.perf_counter() - t0:.1f}s", flush=True)
    for r in (int(x) for x in a.ranks.split(",")):
        t0 = time.perf_counter()
        lora.write_synthetic_adapter(cfg, os.path.join(a.dir, f"lora_r{r}"), r=r, seed=r, std=0.01)
        print(f"[lora_bench] wrote the r = {r} adapter in {time.perf_counter() - t0:.1f}s", flush=True)


class _PeakSampler(threading.Thread):
    """Device memory in use (hipMemGetInfo) every 2 ms."""

    def __init__(self, dev):
        super().__init__(daemon=True)
        self.dev, self.peak, self.stop = dev, 0, False

    def run(self):
        while not self.stop:
            free, total = torch.cuda.mem_get_info(self.dev)
            self.peak = max(self.peak, total - free)
            time.sleep(0.002)


def pass_bench(a) -> None:
    for k in ("PYTORCH_HIP_ALLOC_CONF", "PYTORCH_CUDA_ALLOC_CONF"):
        os.environ.setdefault(k, "expandable_segments:True")
    from flexible_llm_sharding_amd import lora
    from flexible_llm_sharding_amd.engine import ShardedRunner
    from flexible_llm_sharding_amd.runtime.stream import FileLayerSource
    from flexible_llm_sharding_amd.runtime.weights import CompactHostStore, HostStore
    from flexible_llm_sharding_amd.utils.synthetic import synthetic_prompts
    from flexible_llm_sharding_amd.utils.tokenizer import clear_prefix_ids, load_tokenizer, write_synthetic_tokenizer
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = _cfg(a)
    t0 = time.perf_counter()
    adapter = lora.LoraAdapter.load(cfg, a.lora) if a.lora else None
    load_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    phases = {}
    kind, sub = a.store.split("_")
    files = FileLayerSource(cfg, os.path.join(a.dir, sub))
    if kind == "compact":
        store = CompactHostStore(files)
    elif kind == "host":
        store = HostStore.from_source(files)
        phases["pin_s"] = time.perf_counter() - t0
        if adapter is not None:
            t1 = time.perf_counter()
            store.merge_lora(adapter, dev)          # once, at build (ends in a device synchronise)
            phases["merge_at_build_s"] = time.perf_counter() - t1
        t1 = time.perf_counter()
        store.fold_norms(dev)
        torch.cuda.synchronize(dev)
        phases["fold_s"] = time.perf_counter() - t1
    else:
        store = files
    build_s = time.perf_counter() - t0
    torch.cuda.empty_cache()
    tok_dir = f"/tmp/fls_lora_bench_tok_{os.getpid()}"
    write_synthetic_tokenizer(tok_dir, cfg.vocab_size)
    tok = load_tokenizer(tok_dir)
    prompts = synthetic_prompts(a.prompts, 1024, 5, 64, cfg.vocab_size, seed=0)
    r = ShardedRunner(cfg, store, dev, tok, layer_num_per_shard=1, storage_location="cpu",
                      max_vram_gb=a.max_vram_gb or None, lora=adapter)
    sampler = _PeakSampler(dev)
    sampler.start()
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
        print(f"[lora_bench] step {i} {a.store} lora={a.lora}: {dt:.3f}s", flush=True)
    sampler.stop = True
    sampler.join()
    tokens = a.prompts * (1024 + 320)
    print(json.dumps({"store": a.store, "lora": a.lora, "median_s": float(np.median(times)), "min_s": min(times),
                      "max_s": max(times), "n": len(times), "tok_per_s_median": tokens / float(np.median(times)),
                      "peak_device_bytes": sampler.peak,
                      "lora_tensors": adapter.n_tensors if adapter else 0, "lora_rank_max": adapter.rank_max if adapter else 0,
                      "lora_bytes": adapter.nbytes if adapter else 0,
                      "lora_staging_bytes": r.lora_staging.device_bytes() if r.lora_staging is not None else 0,
                      "lora_merge_launches": adapter.merge_launches if adapter else 0,
                      "adapter_load_s": load_s, "build_s": build_s, "build_phases": phases, "passes_total": a.warmup + a.steps,
                      "prefetcher": type(r.prefetcher).__name__, "plan": r.vram_plan,
                      "config": {"model": a.model, "layers": cfg.num_hidden_layers, "prompts": a.prompts,
                                 "tokens": tokens, "max_vram_gb": a.max_vram_gb}}), flush=True)
    r.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "write", "pass"])
    ap.add_argument("--store", choices=["stream_fp16", "compact_int4", "stream_int4", "host_fp16"], default="stream_fp16")
    ap.add_argument("--lora", default=None)
    ap.add_argument("--dir", default="/tmp/fls_lora_bench")
    ap.add_argument("--which", default="fp16,int4")
    ap.add_argument("--ranks", default="16,64")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--prompts", type=int, default=32)
    ap.add_argument("--model", default="llama2-70b")
    ap.add_argument("--num-layers", type=int, default=None)
    ap.add_argument("--max-vram-gb", type=float, default=6.0)
    a = ap.parse_args()
    {"kernel": kernel_bench, "write": write_bench, "pass": pass_bench}[a.what](a)
