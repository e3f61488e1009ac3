"""Cost of --lookup_decoding (profiles/lookup/README.md).

  python scripts/lookup_bench.py kernel             # fls_verify_rows next to fls_argmax_rows on the rows of a
                                                    # drafted call: 160 suffixes x (D + 1) rows of 32000, D = 4, 8
  python scripts/lookup_bench.py gen [--cap 6]      # Llama-2-70B geometry, 32 prompts x 5 suffixes: the plain
                                                    # generation, then D = 4 and 8 with an oracle drafter (every
                                                    # draft accepted: the upper bound) and with a drafter that is
                                                    # always wrong (every draft rejected: the worst case), on one
                                                    # weight store; the time of every call.  --cap G: under
                                                    # --max_vram_gb G (host-mode caches) instead of resident
  python scripts/lookup_bench.py gen --arms plain   # the plain arm alone (runs on a tree without the feature too)

The weights are random: the acceptance of the real drafter on such a model says nothing about real
text, so only the two bounds are measured.
"""
import argparse
import gc
import json
import os
import sys
import tempfile
import time
import types

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
    dev = torch.device("cuda", 0)
    ops = get_ops(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    V, n_sfx = 32000, 160
    for D in (4, 8):
        rows = n_sfx * (D + 1)
        probs = torch.softmax(torch.randn(rows, V, device=dev, generator=g) * 4, dim=-1).half()
        row_start = torch.arange(0, rows + 1, D + 1, dtype=torch.int32, device=dev)
        tok = ops.argmax_rows(probs)
        last = torch.arange(rows, device=dev) % (D + 1) == D
        out = {"suffixes": n_sfx, "D": D, "rows": rows, "V": V, "bytes": rows * V * 2, "iters": iters}
        for name, draft in (("all_accepted", torch.where(last, -1, tok)), ("all_rejected", torch.full_like(tok, -1))):
            draft = draft.to(torch.int32).contiguous()
            for rnd in range(2):
                out[f"argmax_us_r{rnd}"] = _time(lambda: ops.argmax_rows(probs), iters)
                out[f"verify_{name}_us_r{rnd}"] = _time(lambda: ops.verify_rows(probs, row_start, draft), iters)
            _, accept, _, n_kept = ops.verify_rows(probs, row_start, draft)
            out[f"kept_{name}"] = int(n_kept.item())
        print(json.dumps(out), flush=True)


def _oracles():
    """The continuation table and the drafters of the tests (tests/lookup_ref.py)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import lookup_ref
    return lookup_ref


def gen_bench(a) -> None:
    from flexible_llm_sharding_amd.api import generation_loop, greedy_tokens
    from flexible_llm_sharding_amd.config import preset
    from flexible_llm_sharding_amd.engine import ShardedRunner
    from flexible_llm_sharding_amd.parallel.comm import Comm
    from flexible_llm_sharding_amd.runtime.weights import HostStore
    from flexible_llm_sharding_amd.utils.synthetic import synthetic_prompts
    from flexible_llm_sharding_amd.utils.tokenizer import load_tokenizer, write_synthetic_tokenizer
    dev = torch.device("cuda", 0)
    cfg = preset(a.model, **({} if a.num_layers is None else {"num_hidden_layers": a.num_layers}))
    store = HostStore.synthetic(cfg, dev, seed=0, fold_norms=True)
    with tempfile.TemporaryDirectory(prefix="fls_lookup_bench_tok_") as tok_dir:
        write_synthetic_tokenizer(tok_dir, cfg.vocab_size)
        tok = load_tokenizer(tok_dir)
    # (every suffix ends with a space: s + decode(tokens) then re-tokenizes to the suffix's ids + the tokens)
    prompts = [(p, tuple(s + " " for s in sfx)) for p, sfx in synthetic_prompts(a.prompts, 1024, 5, 64, cfg.vocab_size,
                                                                                seed=0)]
    V = cfg.vocab_size
    arms = [x for x in a.arms.split(",") if x]
    plain_tokens, table, updated = None, None, {}

    def drafter_for(kind):
        lr = _oracles()
        return lr.oracle_drafter(table) if kind == "oracle" else lr.all_wrong(table, V)

    for rnd in range(a.rounds):
        for arm in arms:
            kind, _, dd = arm.partition(":")
            D = int(dd or 0)
            if D and table is None:
                raise SystemExit("the plain arm comes first: the drafters are built from its tokens")
            args = argparse.Namespace(num_gen_token=a.gen, data_parallel=False, num_batch=1, do_sample=False,
                                      lookup_decoding=D, lookup_ngram=3)
            kw = dict(resident=True) if not a.cap else dict(max_vram_gb=a.cap)
            r = ShardedRunner(cfg, store, dev, tok, layer_num_per_shard=1, prefix_kv_cache=True,
                              suffix_kv_cache=bool(a.suffix_kv), **kw)
            step_s, stats = [], {}
            t = time.perf_counter()
            extra = dict(drafter=drafter_for(kind), lookup_stats=stats) if D else {}
            s, u = generation_loop(args, r, Comm(0, 1, dev), tok, prompts, step_s, **extra)
            total = time.perf_counter() - t
            updated.setdefault("plain", u)
            if plain_tokens is None:
                plain_tokens = [np.asarray(greedy_tokens(x)) for x in s]
                if any(":" in x for x in arms):
                    table = _oracles().continuation_table((cfg, tok, prompts, None),
                                                          types.SimpleNamespace(tokens=plain_tokens), gen=a.gen)
            res = {"arm": arm, "round": rnd, "cap_gb": a.cap, "suffix_kv": bool(a.suffix_kv), "calls": len(step_s),
                   "total_s": round(total, 3), "call_s": [round(x, 4) for x in step_s],
                   "lookup": stats, "speculative_dropped": getattr(r, "spec_dropped", None),
                   "last_call": {k: r.stats.get(k) for k in ("tokens", "speculative", "graph_replays", "weight_h2d_bytes")},
                   "score_d2h_bytes_last_call": r.score_d2h_bytes,
                   "same_prompts_as_plain": u == updated["plain"],
                   "same_scores_as_plain": None}
            if kind == "plain":
                updated.setdefault("scores", s)
            else:
                res["same_scores_as_plain"] = all(np.array_equal(x.view(np.uint16), y.view(np.uint16))
                                                  for x, y in zip(s, updated["scores"]))
            print(json.dumps(res), flush=True)
            r.close()
            del r, s, u
            gc.collect()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "gen"])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--gen", type=int, default=28)
    ap.add_argument("--prompts", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--cap", type=float, default=0.0, help="--max_vram_gb (0: weights resident)")
    ap.add_argument("--suffix-kv", type=int, default=1, help="suffix K/V reuse (0: the capped default, prefix cache only)")
    ap.add_argument("--arms", default="plain,oracle:4,oracle:8,wrong:4,wrong:8")
    ap.add_argument("--model", default="llama2-70b")
    ap.add_argument("--num-layers", type=int, default=None)
    a = ap.parse_args()
    kernel_bench(a.iters) if a.what == "kernel" else gen_bench(a)
