"""Cost of bitsandbytes 4-bit (NF4) checkpoints (profiles/nf4/README.md).  Figures only, nothing pass/fail.

  python scripts/nf4_bench.py kernel [--iters N]
        # in one process: the expansion chains of fls_dequant_nf4 (block 64; U8 absmax with nested blocks
        # of 256, and fp32 absmax) and of fls_dequant_int4 (group 64 and 128, fp16 scales) in place on
        # 8192 x 28672 and 8192 x 8192 tensors: launches, median and minimum of N timed calls after 3
        # warm-up calls (device events around each call, the landed bytes restored outside them),
        # achieved bytes/s at the bytes read plus 2 bytes written per weight, and NF4 / INT4 (group 64)
  python scripts/nf4_bench.py write --dir D [--model llama2-70b] [--unique-layers K] [--num-layers L]
                                    [--which nf4,int4]
        # synthetic checkpoints D/nf4 (block 64, double quantisation) and D/int4 (group 128, fp16
        # scales); decoder layers beyond K hard-linked
  python scripts/nf4_bench.py pass --store stream_nf4|stream_int4|compact_nf4|compact_int4 [--dir D]
                                   [--steps N] [--prompts P] [--o-direct] [--max-vram-gb 6]
        # P prompts of 1,024 + 5 x 64 tokens: tok/s, weight_stall_gpu_s and weight_wait_s per pass, H2D
        # bytes per pass, the table arena and the planned chunk sizes
"""
import argparse
import json
import os
import sys
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
    return med


def kernel_bench(iters: int) -> None:
    from flexible_llm_sharding_amd import _native, int4, nf4
    from flexible_llm_sharding_amd.ops import get_ops
    dev = torch.device("cuda", 0)
    ops, k = get_ops(dev), _native.kernels()
    code = torch.tensor(nf4.NF4_CODE, dtype=torch.float32, device=dev)
    code2 = nf4.writer_code2().to(dev)
    for rows, cols in ((8192, 28672), (8192, 8192)):
        n = rows * cols
        region = torch.empty(2 * n, dtype=torch.uint8, device=dev)
        packed = torch.randint(0, 256, (n // 2,), dtype=torch.uint8, device=dev)
        med = {}
        for kind, es in (("u8", 1), ("f32", 4)):
            block = 64
            if es == 1:
                absmax = torch.randint(0, 256, (n // block,), dtype=torch.uint8, device=dev)
                nested = (torch.rand(-(-(n // block) // 256), device=dev) + 0.5) * 1e-3
                tables = (code2, nested, 256, 2e-3)
            else:
                absmax = ((torch.rand(n // block, device=dev) + 0.5) * 1e-3).view(torch.uint8)
                tables = (None, None, 0, 0.0)
            base, span = nf4.landing_span(n, block, es)
            landed = torch.empty(span, dtype=torch.uint8, device=dev)      # the landed bytes, restored before each call
            nf4.land(region, packed, absmax, n, block, es)
            landed.copy_(region[base:])
            ak = nf4.ABSMAX_U8 if es == 1 else nf4.ABSMAX_F32
            m, mn = _time(lambda: ops.dequant_nf4(region, n, block, ak, code, *tables), lambda: region[base:].copy_(landed),
                          iters)
            med[kind] = _row("fls_dequant_nf4", rows, cols, int(k.fls_dequant_nf4_launches(n, block, es)), m, mn,
                             n // 2 + n // block * es + 2 * n, iters, block=block, absmax=kind)
            del landed, absmax
        for g in (64, 128):
            scale = ((torch.rand(n // g, device=dev) + 0.5) * 1e-3).to(torch.float16).view(torch.uint8)
            base, span = int4.landing_span(n, g, 2)
            landed = torch.empty(span, dtype=torch.uint8, device=dev)
            int4.land(region, packed, scale, n, g, 2)
            landed.copy_(region[base:])
            m, mn = _time(lambda: ops.dequant_int4(region, n, g, torch.float16), lambda: region[base:].copy_(landed), iters)
            med[g] = _row("fls_dequant_int4", rows, cols, int(k.fls_dequant_int4_launches(n, g, 2)), m, mn,
                          n // 2 + n // g * 2 + 2 * n, iters, group=g, scale_dtype="float16")
            del landed, scale
        print(json.dumps({"shape": [rows, cols], "nf4_u8_over_int4_g64": med["u8"] / med[64],
                          "nf4_f32_over_int4_g64": med["f32"] / med[64], "nf4_u8_over_int4_g128": med["u8"] / med[128],
                          "nf4_f32_over_int4_g128": med["f32"] / med[128]}), flush=True)
        del region, packed


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
                                   quantize=sub, int4_group=128, nf4_block=64, nf4_double_quant=True)
        print(f"[nf4_bench] wrote {sub} in {time.perf_counter() - t0:.1f}s", flush=True)


def pass_bench(a) -> None:
    for k in ("PYTORCH_HIP_ALLOC_CONF", "PYTORCH_CUDA_ALLOC_CONF"):
        os.environ.setdefault(k, "expandable_segments:True")
    from flexible_llm_sharding_amd.engine import ShardedRunner
    from flexible_llm_sharding_amd.runtime.stream import FileLayerSource
    from flexible_llm_sharding_amd.runtime.weights import CompactHostStore
    from flexible_llm_sharding_amd.utils.synthetic import synthetic_prompts
    from flexible_llm_sharding_amd.utils.tokenizer import clear_prefix_ids, load_tokenizer
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = _cfg(a)
    how, sub = a.store.split("_")
    path = os.path.join(a.dir, sub)
    t0 = time.perf_counter()
    files = FileLayerSource(cfg, path, direct=a.o_direct)
    store = CompactHostStore(files) if how == "compact" else files
    build_s = time.perf_counter() - t0
    tok = load_tokenizer(path)
    prompts = synthetic_prompts(a.prompts, 1024, 5, 64, cfg.vocab_size, seed=0)
    r = ShardedRunner(cfg, store, dev, tok, layer_num_per_shard=1, storage_location="cpu",
                      max_vram_gb=a.max_vram_gb or None)
    times, stall, wait, h2d = [], [], [], []
    for i in range(a.warmup + a.steps):
        clear_prefix_ids()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        r(prompts)
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        if i >= a.warmup:
            times.append(dt)
            stall.append(r.stats["weight_stall_gpu_s"])
            wait.append(r.stats["weight_wait_s"])
            h2d.append(r.stats["weight_h2d_bytes"])
        print(f"[nf4_bench] step {i} {a.store}: {dt:.3f}s", flush=True)
    tokens = a.prompts * (1024 + 320)
    print(json.dumps({"store": a.store, "o_direct": bool(a.o_direct), "median_s": float(np.median(times)), "min_s": min(times),
                      "max_s": max(times), "n": len(times), "tok_per_s_median": tokens / float(np.median(times)),
                      "weight_stall_gpu_s_median": float(np.median(stall)), "weight_wait_s_median": float(np.median(wait)),
                      "weight_h2d_bytes_per_pass": int(np.median(h2d)), "weight_file_bytes": int(files.file_bytes()),
                      "scale_arena_bytes": int(files.scale_arena_bytes()), "nf4_tensors": int(files.nf4_tensors()),
                      "int4_tensors": int(files.int4_tensors()), "build_s": build_s,
                      "prefetcher": type(r.prefetcher).__name__, "plan": r.vram_plan,
                      "config": {"model": a.model, "layers": cfg.num_hidden_layers, "prompts": a.prompts,
                                 "tokens": tokens, "max_vram_gb": a.max_vram_gb}}), flush=True)
    r.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "write", "pass"])
    ap.add_argument("--store", choices=["stream_nf4", "stream_int4", "compact_nf4", "compact_int4"], default="stream_nf4")
    ap.add_argument("--dir", default="/tmp/fls_nf4_bench")
    ap.add_argument("--which", default="nf4,int4")
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
