"""Cost of weight-only FP8 checkpoints (profiles/fp8/README.md).  Figures only, nothing pass/fail.

  python scripts/fp8_bench.py kernel [--iters N]
        # fls_dequant_fp8 in place on 8192 x 28672 and 8192 x 8192 tensors, tensor / channel / block128
        # scales, against fls_cast_f16 (bf16 in place) on the same element counts: device events,
        # median and minimum, bytes = 3 per weight (1 read + 2 written; the cast moves 4)
  python scripts/fp8_bench.py write --dir D [--model llama2-70b] [--unique-layers K] [--num-layers L]
        # an FP8 (channel scales) synthetic checkpoint in D/fp8 and an fp16 one in D/fp16, decoder
        # layers >= K hard-linked to layer i % K
  python scripts/fp8_bench.py pass --store S [--dir D] [--steps N] [--o-direct]
        # full scoring passes (32 prompts of 1024 + 5 x 64 tokens, --max_vram_gb 6) with the weights from
        # S = compact (CompactHostStore over D/fp8) | fp16_landing_fold (HostStore.synthetic, norms folded
        # as each layer lands) | fp16_prefolded (HostStore.synthetic(fold_norms=True), the default) |
        # stream_fp8 (D/fp8 streamed) | stream_fp16 (D/fp16 streamed): tok/s, the peak device memory
        # from a 2 ms sampler, pinned bytes and H2D bytes

One store per process (a VRAM cap is per process); run them alternated in one job on one box.
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


def _time(fn, prep, iters):
    times = []
    for i in range(iters + 3):
        prep()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= 3:
            times.append(e0.elapsed_time(e1) * 1e-3)
    return float(np.median(times)), min(times)


def kernel_bench(iters: int) -> None:
    from flexible_llm_sharding_amd import _native, fp8
    from flexible_llm_sharding_amd.ops import get_ops
    dev = torch.device("cuda", 0)
    ops, k = get_ops(dev), _native.kernels()
    for rows, cols in ((8192, 28672), (8192, 8192)):
        n = rows * cols
        region = torch.empty(2 * n, dtype=torch.uint8, device=dev)
        # random bytes with the two NaN patterns masked out (0x7F -> 0x7E, 0xFF -> 0xFE)
        bits = torch.randint(0, 256, (n,), dtype=torch.uint8, device=dev)
        bits = torch.where((bits & 0x7F) == 0x7F, bits - 1, bits)
        for kind, name in ((fp8.KIND_TENSOR, "tensor"), (fp8.KIND_CHANNEL, "channel"), (fp8.KIND_BLOCK, "block128")):
            cnt = {fp8.KIND_TENSOR: 1, fp8.KIND_CHANNEL: rows, fp8.KIND_BLOCK: -(-rows // 128) * -(-cols // 128)}[kind]
            scale = (torch.rand(cnt, device=dev) + 0.5) * 1e-3
            med, mn = _time(lambda: ops.dequant_fp8(region, n, scale, kind, cols), lambda: region[n:].copy_(bits), iters)
            print(json.dumps({"kernel": "fls_dequant_fp8", "shape": [rows, cols], "scale": name,
                              "launches": int(k.fls_dequant_fp8_launches(n)), "median_us": med * 1e6, "min_us": mn * 1e6,
                              "bytes": 3 * n, "TB_per_s_median": 3 * n / med / 1e12, "iters": iters}), flush=True)
        src = torch.randn(n // 4, device=dev).bfloat16().repeat(4).view(torch.uint8)
        med, mn = _time(lambda: ops.cast_f16(region, region, 1), lambda: region.copy_(src), iters)
        print(json.dumps({"kernel": "fls_cast_f16 (bf16, in place)", "shape": [rows, cols], "launches": 1,
                          "median_us": med * 1e6, "min_us": mn * 1e6, "bytes": 4 * n,
                          "TB_per_s_median": 4 * n / med / 1e12, "iters": iters}), flush=True)
        del region, bits, src


def _cfg(a):
    from flexible_llm_sharding_amd.config import preset
    return preset(a.model, **({} if a.num_layers is None else {"num_hidden_layers": a.num_layers}))


def write_bench(a) -> None:
    from flexible_llm_sharding_amd.utils.synthetic import write_synthetic_checkpoint
    cfg = _cfg(a)
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    for sub, q in (("fp8", "fp8"), ("fp16", None)):
        t0 = time.perf_counter()
        write_synthetic_checkpoint(cfg, os.path.join(a.dir, sub), seed=0, unique_layers=a.unique_layers, device=dev,
                                   quantize=q, fp8_scale="channel")
        print(f"[fp8_bench] wrote {sub} in {time.perf_counter() - t0:.1f}s", flush=True)


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
    from flexible_llm_sharding_amd.engine import ShardedRunner
    from flexible_llm_sharding_amd.runtime import hostmem
    from flexible_llm_sharding_amd.runtime.stream import FileLayerSource
    from flexible_llm_sharding_amd.runtime.weights import CompactHostStore, HostStore
    from flexible_llm_sharding_amd.utils.synthetic import synthetic_prompts
    from flexible_llm_sharding_amd.utils.tokenizer import clear_prefix_ids, load_tokenizer, write_synthetic_tokenizer
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = _cfg(a)
    t0 = time.perf_counter()
    s = a.store
    if s == "compact":
        store = CompactHostStore(FileLayerSource(cfg, os.path.join(a.dir, "fp8")))
    elif s in ("stream_fp8", "stream_fp16"):
        store = FileLayerSource(cfg, os.path.join(a.dir, s[len("stream_"):]), direct=a.o_direct)
    else:
        store = HostStore.synthetic(cfg, dev, seed=0, fold_norms=s == "fp16_prefolded")
    build_s = time.perf_counter() - t0
    torch.cuda.empty_cache()
    tok_dir = f"/tmp/fls_fp8_bench_tok_{os.getpid()}"
    write_synthetic_tokenizer(tok_dir, cfg.vocab_size)
    tok = load_tokenizer(tok_dir)
    prompts = synthetic_prompts(32, 1024, 5, 64, cfg.vocab_size, seed=0)
    r = ShardedRunner(cfg, store, dev, tok, layer_num_per_shard=1, storage_location="cpu",
                      max_vram_gb=a.max_vram_gb or None)
    sampler = _PeakSampler(dev)
    sampler.start()
    times, h2d = [], []
    for i in range(a.warmup + a.steps):
        clear_prefix_ids()
        torch.cuda.synchronize(dev)
        b0 = r.prefetcher.bytes_h2d
        t0 = time.perf_counter()
        r(prompts)
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        if i >= a.warmup:
            times.append(dt)
            h2d.append(r.prefetcher.bytes_h2d - b0)
        print(f"[fp8_bench] step {i} {s}: {dt:.3f}s", flush=True)
    sampler.stop = True
    sampler.join()
    tokens = 32 * (1024 + 320)
    st = store.stats() if hasattr(store, "stats") else {}
    pinned = hostmem.pinned_peak + (store.pinned_bytes() if isinstance(store, FileLayerSource) else 0)
    print(json.dumps({"store": s, "o_direct": bool(a.o_direct), "median_s": float(np.median(times)), "min_s": min(times),
                      "max_s": max(times), "n": len(times), "tok_per_s_median": tokens / float(np.median(times)),
                      "peak_device_bytes": sampler.peak, "pinned_bytes": int(pinned),
                      "slot_h2d_image_bytes_per_pass": int(np.median(h2d)),
                      "source_h2d_bytes_total": int(st.get("h2d_bytes", 0)), "build_s": build_s,
                      "prefetcher": type(r.prefetcher).__name__, "plan": r.vram_plan,
                      "config": {"model": a.model, "layers": cfg.num_hidden_layers, "prompts": 32, "tokens": tokens,
                                 "max_vram_gb": a.max_vram_gb}}), flush=True)
    r.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "write", "pass"])
    ap.add_argument("--store", choices=["compact", "fp16_landing_fold", "fp16_prefolded", "stream_fp8", "stream_fp16"],
                    default="compact")
    ap.add_argument("--dir", default="/tmp/fls_fp8_bench")
    ap.add_argument("--o-direct", action="store_true")
    ap.add_argument("--unique-layers", type=int, default=1)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--model", default="llama2-70b")
    ap.add_argument("--num-layers", type=int, default=None)
    ap.add_argument("--max-vram-gb", type=float, default=6.0)
    a = ap.parse_args()
    {"kernel": kernel_bench, "write": write_bench, "pass": pass_bench}[a.what](a.iters if a.what == "kernel" else a)
