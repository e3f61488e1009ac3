"""Sliding-window attention microbenchmark at the 70B head geometry (64 query heads, 8 KV heads,
hd 128) over 8k-token prefixes read from the K/V cache: one attention launch with W = 4096 against
the same launch without a window, for

  * suffix  - a full pass of the suffix tokens: 5 x 64-row suffixes per prompt (64-row items, range
              0 from the cache, attn_fwd),
  * decode  - a generation step: one new row per suffix after 63 kept ones (range 2, attn_decode).

A windowed row sees W keys, so its item walks about W / 64 key tiles of the prefix instead of all
of them; the expectation is that the launch time follows the walked tiles.  The metadata comes from
``pack_prompts`` (the arrays the engine hands the kernel).  Every arm runs in a child process of its
own under a time limit, the launches captured in a HIP graph (GPU time, not host dispatch).

    python scripts/attn_window_bench.py [--prompts 8] [--prefix 8192] [--window 4096] [--iters 20]
"""
import argparse
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NH, NKV, HD = 64, 8, 128
N_SUFFIX, SUFFIX_LEN = 5, 64
ARM_TIMEOUT_S = 120


def one(a, kind: str, window: int) -> None:
    from flexible_llm_sharding_amd.ops.hip_backend import HipOps
    from flexible_llm_sharding_amd.runtime.batch import pack_prompts
    from flexible_llm_sharding_amd.utils.tokenizer import TokenizedPrompt
    dev = torch.device("cuda", 0)
    ops = HipOps()
    tps = [TokenizedPrompt(list(range(a.prefix)), [list(range(SUFFIX_LEN))] * N_SUFFIX, SUFFIX_LEN,
                           [SUFFIX_LEN - 1] * N_SUFFIX) for _ in range(a.prompts)]
    per = a.prefix + N_SUFFIX * 64                     # cache rows per prompt: prefix, then 64-row suffix regions
    offs = [j * per for j in range(a.prompts)]
    rows = [[j * per + a.prefix + s * 64 for s in range(N_SUFFIX)] for j in range(a.prompts)]
    keep = [[SUFFIX_LEN - 1] * N_SUFFIX for _ in tps] if kind == "decode" else None
    b = pack_prompts(tps, list(range(a.prompts)), prefix_offsets=offs, kv_cached=True, suffix_rows=rows,
                     suffix_keep=keep, window=window)
    m = b.device_tensors(dev)
    kv0 = (torch.randn(a.prompts * per, 2 * NKV * HD, device=dev) * 0.5).half()
    qkv = (torch.randn(b.num_tokens, (NH + 2 * NKV) * HD, device=dev) * 0.5).half()
    kw = {"seg_lo": m["seg_lo"], "kv0": kv0}
    if window:
        kw.update(r0_lo=m["r0_lo"], r0_item=m["r0_item"])
    if kind == "decode":
        kw.update(work2=m["work2"], r2win=m["r2win"], q_block=b.r2_q_block)
    # key tiles the launch walks: range 0 from the tile of each item's smallest lower bound
    first = b.r0_item[:, 0] if window else np.zeros(b.work.shape[0], np.int64)
    tiles = int(sum(-(-int(w[4]) // 64) - min(int(f), int(w[4])) // 64 for w, f in zip(b.work, first)))

    def run():
        ops.attention(qkv, m["work"], NH, NKV, HD, **kw)
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        with torch.cuda.graph(g, stream=st):
            for _ in range(a.iters):
                run()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1000 / a.iters
    print(f"{kind:7s} W={window or 'none':>5}: {us:9.1f} us/launch  {b.work.shape[0]} items x {b.num_tokens} rows, "
          f"{tiles} prefix key tiles walked  ({us / max(tiles, 1):.3f} us/tile)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompts", type=int, default=8)
    ap.add_argument("--prefix", type=int, default=8192)
    ap.add_argument("--window", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--one", nargs=2, metavar=("KIND", "WINDOW"), help="(internal) run one arm in this process")
    a = ap.parse_args()
    if a.one:
        one(a, a.one[0], int(a.one[1]))
        return
    for kind in ("suffix", "decode"):
        for w in (0, a.window):
            cmd = [sys.executable, os.path.abspath(__file__), "--prompts", str(a.prompts), "--prefix", str(a.prefix),
                   "--iters", str(a.iters), "--one", kind, str(w)]
            rc = subprocess.run(cmd, timeout=ARM_TIMEOUT_S).returncode
            if rc != 0:
                sys.exit(f"{kind} W={w}: exit status {rc}; stopping")


if __name__ == "__main__":
    main()
