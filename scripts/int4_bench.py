"""Cost of weight-only INT4 checkpoints (profiles/int4/README.md).  Figures only, nothing pass/fail.

  python scripts/int4_bench.py kernel [--iters N]
        # fls_dequant_int4 (g 32 / 128 / per channel; fp16 and fp32 scales), fls_dequant_fp8 (channel
        # scales) and fls_cast_f16 in place on 8192 x 28672 and 8192 x 8192 tensors: launches, median
        # and minimum of N timed calls after 3 warm-up calls (device events around each call, the
        # source restored outside them), achieved bytes/s at 2.5 (INT4), 3 (FP8), 4 (cast) bytes/weight
  python scripts/int4_bench.py write --dir D [--model llama2-70b] [--unique-layers K] [--num-layers L]
                                     [--which int4,fp8,fp16] [--group 128]
        # synthetic checkpoints D/int4 (fp16 group scales), D/fp8 (channel scales), D/fp16; decoder
        # layers beyond K hard-linked
  python scripts/int4_bench.py pass --store S [--dir D] [--steps N] [--prompts P] [--o-direct]
                                    [--max-vram-gb 6]
        # S = compact_int4 | stream_int4 | compact_fp8 | stream_fp8 | stream_fp16 | fp16_landing_fold:
        # P prompts of 1,024 + 5 x 64 tokens; tok/s, peak device memory (hipMemGetInfo, sampled),
        # pinned host bytes, H2D bytes per pass and the planned chunk sizes
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


def _row(kernel, rows, cols, launches, med, mn, nbytes, iters, **kw):
    print(json.dumps({"kernel": kernel, "shape": [rows, cols], **kw, "launches": launches, "median_us": med * 1e6,
                      "min_us": mn * 1e6, "bytes": nbytes, "TB_per_s_median": nbytes / med / 1e12, "iters": iters}),
          flush=True)


def kernel_bench(iters: int) -> None:
    from flexible_llm_sharding_amd import _native, fp8, int4
    from flexible_llm_sharding_amd.ops import get_ops
    dev = torch.device("cuda", 0)
    ops, k = get_ops(dev), _native.kernels()
    for rows, cols in ((8192, 28672), (8192, 8192)):
        n = rows * cols
        region = torch.empty(2 * n, dtype=torch.uint8, device=dev)
        nibbles = torch.randint(0, 256, (n // 2,), dtype=torch.uint8, device=dev)
        for g, dtype in ((32, torch.float32), (128, torch.float16), (cols, torch.float16)):
            es = torch.empty((), dtype=dtype).element_size()
            scale = ((torch.rand(n // g, device=dev) + 0.5) * 1e-3).to(dtype).view(torch.uint8)
            base, span = int4.landing_span(n, g, es)
            landed = torch.empty(span, dtype=torch.uint8, device=dev)      # the landed bytes, restored before each call
            int4.land(region, nibbles, scale, n, g, es)
            landed.copy_(region[base:])
            med, mn = _time(lambda: ops.dequant_int4(region, n, g, dtype), lambda: region[base:].copy_(landed), iters)
            _row("fls_dequant_int4", rows, cols, int(k.fls_dequant_int4_launches(n, g, es)), med, mn,
                 n // 2 + n // g * es + 2 * n, iters, group=g, scale_dtype=str(dtype).split(".")[-1])
            del landed, scale
        bits = torch.randint(0, 256, (n,), dtype=torch.uint8, device=dev)
        bits = torch.where((bits & 0x7F) == 0x7F, bits - 1, bits)
        sc = (torch.rand(rows, device=dev) + 0.5) * 1e-3
        med, mn = _time(lambda: ops.dequant_fp8(region, n, sc, fp8.KIND_CHANNEL, cols), lambda: region[n:].copy_(bits), iters)
        _row("fls_dequant_fp8", rows, cols, int(k.fls_dequant_fp8_launches(n)), med, mn, 3 * n, iters, scale="channel")
        src = torch.randn(n // 4, device=dev).bfloat16().repeat(4).view(torch.uint8)
        med, mn = _time(lambda: ops.cast_f16(region, region, 1), lambda: region.copy_(src), iters)
        _row("fls_cast_f16 (bf16, in place)", rows, cols, 1, med, mn, 4 * n, iters)
        del region, bits, src, nibbles


def _cfg(a):
    from flexible_llm_sharding_amd.config import preset
    return preset(a.model, **({} if a.num_layers is None else {"num_hidden_layers": a.num_layers}))


def write_bench(a) -> None:
    from flexible_llm_sharding_amd.utils.synthetic import write_synthetic_checkpoint
    cfg = _cfg(a)
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    for sub in a.which.split(","):
        t0 = time.perf_counter()
        write_synthetic_checkpoint(cfg, os.path.join(a.dir, sub), seed=0, unique_layers=a.unique_layers, device=dev,
                                   quantize=None if sub == "fp16" else sub, fp8_scale="channel", int4_group=a.group)
        print(f"[int4_bench] wrote {sub} in {time.perf_counter() - t0:.1f}s", flush=True)


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
    if s.startswith("compact_"):
        store = CompactHostStore(FileLayerSource(cfg, os.path.join(a.dir, s[len("compact_"):])))
    elif s.startswith("stream_"):
        store = FileLayerSource(cfg, os.path.join(a.dir, s[len("stream_"):]), direct=a.o_direct)
    else:
        store = HostStore.synthetic(cfg, dev, seed=0, fold_norms=False)
    build_s = time.perf_counter() - t0
    torch.cuda.empty_cache()
    tok_dir = f"/tmp/fls_int4_bench_tok_{os.getpid()}"
    write_synthetic_tokenizer(tok_dir, cfg.vocab_size)
    tok = load_tokenizer(tok_dir)
    prompts = synthetic_prompts(a.prompts, 1024, 5, 64, cfg.vocab_size, seed=0)
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
        print(f"[int4_bench] step {i} {s}: {dt:.3f}s", flush=True)
    sampler.stop = True
    sampler.join()
    tokens = a.prompts * (1024 + 320)
    st = store.stats() if hasattr(store, "stats") else {}
    files = getattr(store, "files", store)
    pinned = hostmem.pinned_peak + (store.pinned_bytes() if isinstance(store, FileLayerSource) else 0)
    print(json.dumps({"store": s, "o_direct": bool(a.o_direct), "median_s": float(np.median(times)), "min_s": min(times),
                      "max_s": max(times), "n": len(times), "tok_per_s_median": tokens / float(np.median(times)),
                      "peak_device_bytes": sampler.peak, "pinned_bytes": int(pinned),
                      "slot_h2d_image_bytes_per_pass": int(np.median(h2d)),
                      "weight_file_bytes": int(files.file_bytes()) if hasattr(files, "file_bytes") else None,
                      "source_h2d_bytes_total": int(st.get("h2d_bytes", 0)), "passes_total": a.warmup + a.steps,
                      "build_s": build_s, "prefetcher": type(r.prefetcher).__name__, "plan": r.vram_plan,
                      "config": {"model": a.model, "layers": cfg.num_hidden_layers, "prompts": a.prompts,
                                 "tokens": tokens, "max_vram_gb": a.max_vram_gb}}), flush=True)
    r.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "write", "pass"])
    ap.add_argument("--store", choices=["compact_int4", "stream_int4", "compact_fp8", "stream_fp8", "stream_fp16",
                                        "fp16_landing_fold"], default="compact_int4")
    ap.add_argument("--dir", default="/tmp/fls_int4_bench")
    ap.add_argument("--which", default="int4,fp8,fp16")
    ap.add_argument("--group", type=int, default=128)
    ap.add_argument("--o-direct", action="store_true")
    ap.add_argument("--unique-layers", type=int, default=1)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--prompts", type=int, default=32)
    ap.add_argument("--model", default="llama2-70b")
    ap.add_argument("--num-layers", type=int, default=None)
    ap.add_argument("--max-vram-gb", type=float, default=6.0)
    a = ap.parse_args()
    {"kernel": kernel_bench, "write": write_bench, "pass": pass_bench}[a.what](a.iters if a.what == "kernel" else a)
