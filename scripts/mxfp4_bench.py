"""Expansion rate of MXFP4 against INT4, and the checkpoints of the interference runs
(profiles/mxfp4/README.md).  Figures only, nothing pass/fail.

  python scripts/mxfp4_bench.py --write DIR [--model llama2-70b]
        # the checkpoints of the interference runs: DIR/mxfp4, DIR/int4 (g = 128, fp16 scales) and DIR/fp16
        # (the same seeded weights, not quantised), one decoder layer written and the others hard-linked to it,
        # and DIR/prompts.pkl (32 prompts of 1,024 + 5 x 64 tokens).  Each then runs as
        #   python main.py --model_path DIR/<fmt> --prompt_pickle DIR/prompts.pkl --output_file out.pkl
        #       --weight_cache host --max_vram_gb 6 --num_gen_token 2 --prefix_kv_cache false
        #       --suffix_kv_cache false --metrics_json <fmt>.json
        # (two full passes; step_s, tokens_last_pass, weight_pinned_bytes and peak_hbm_bytes of the metrics)
  python scripts/mxfp4_bench.py [--iters N] [--rounds R] [--rows 8192] [--cols 28672]
        # in one process, R rounds alternating the two chains in place on a rows x cols tensor:
        # fls_dequant_mxfp4 (scale bytes 120..134, the hardware convert) and fls_dequant_int4 (group 128,
        # fp16 scales).  Per round and kernel: launches, median and minimum of N timed calls after 3 warm-up
        # calls (device events around each call, the landed bytes restored outside them) and GB/s of fp16
        # written (2 bytes per weight).  Then the spread of the medians over the rounds and their ratio.
"""
import argparse
import json
import os
import pickle
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


def write(root: str, model: str) -> None:
    from flexible_llm_sharding_amd.config import preset
    from flexible_llm_sharding_amd.utils.synthetic import synthetic_prompts, write_synthetic_checkpoint
    cfg = preset(model)
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    for sub, q in (("fp16", None), ("int4", "int4"), ("mxfp4", "mxfp4")):
        t0 = time.perf_counter()
        write_synthetic_checkpoint(cfg, os.path.join(root, sub), seed=0, unique_layers=1, device=dev, quantize=q,
                                   int4_group=128)
        print(f"[mxfp4_bench] wrote {sub} in {time.perf_counter() - t0:.1f}s", flush=True)
    with open(os.path.join(root, "prompts.pkl"), "wb") as f:
        pickle.dump(synthetic_prompts(32, 1024, 5, 64, cfg.vocab_size, seed=0), f)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", default=None, metavar="DIR")
    ap.add_argument("--model", default="llama2-70b")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--cols", type=int, default=28672)
    a = ap.parse_args(argv)
    if a.write:
        write(a.write, a.model)
        return 0
    if not torch.cuda.is_available():
        raise SystemExit("mxfp4_bench needs the GPU")
    from flexible_llm_sharding_amd import _native, int4, mxfp4
    from flexible_llm_sharding_amd.ops import get_ops
    dev = torch.device("cuda", 0)
    ops, k = get_ops(dev), _native.kernels()
    n = a.rows * a.cols
    region = torch.empty(2 * n, dtype=torch.uint8, device=dev)
    packed = torch.randint(0, 256, (n // 2,), dtype=torch.uint8, device=dev)
    cases = {}
    e8 = torch.randint(120, 135, (n // 32,), dtype=torch.uint8, device=dev)
    s16 = ((torch.rand(n // 128, device=dev) + 0.5) * 1e-3).to(torch.float16).view(torch.uint8)
    for name, mod, scales, g, es, fn, launches in (
            ("fls_dequant_mxfp4", mxfp4, e8, 32, 1, lambda: ops.dequant_mxfp4(region, n), k.fls_dequant_mxfp4_launches(n)),
            ("fls_dequant_int4", int4, s16, 128, 2, lambda: ops.dequant_int4(region, n, 128, torch.float16),
             k.fls_dequant_int4_launches(n, 128, 2))):
        base, span = mod.landing_span(n, g, es)
        mod.land(region, packed, scales, n, g, es)
        cases[name] = (fn, base, region[base:].clone(), int(launches), n // 2 + n // g * es)
    meds = {name: [] for name in cases}
    for rnd in range(a.rounds):
        for name, (fn, base, landed, launches, read) in cases.items():
            med, mn = _time(fn, lambda: region[base:].copy_(landed), a.iters)
            meds[name].append(med)
            print(json.dumps({"kernel": name, "round": rnd, "shape": [a.rows, a.cols], "launches": launches,
                              "median_us": med * 1e6, "min_us": mn * 1e6, "fp16_GB_per_s_median": 2 * n / med / 1e9,
                              "read_plus_written_GB_per_s_median": (read + 2 * n) / med / 1e9, "iters": a.iters}), flush=True)
    out = {name: {"median_us": float(np.median(v)) * 1e6, "spread_pct": (max(v) - min(v)) / float(np.median(v)) * 100,
                  "fp16_GB_per_s": 2 * n / float(np.median(v)) / 1e9} for name, v in meds.items()}
    out["mxfp4_over_int4_time"] = float(np.median(meds["fls_dequant_mxfp4"])) / float(np.median(meds["fls_dequant_int4"]))
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
