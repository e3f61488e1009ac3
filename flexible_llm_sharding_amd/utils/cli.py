"""Command-line interface — the reference flags verbatim plus additive ones.

Reference: ``/root/reference/main.py:30-49``.  Deliberate fix:
``--data_parallel`` is parsed as a real boolean (the reference uses
``type=bool``, so ``--data_parallel False`` silently meant True); a bare
``--data_parallel`` also enables it.
"""
from __future__ import annotations

import argparse


def str2bool(v) -> bool:
    if isinstance(v, bool):
        return v
    s = str(v).strip().lower()
    if s in ("1", "true", "t", "yes", "y", "on"):
        return True
    if s in ("0", "false", "f", "no", "n", "off", ""):
        return False
    raise argparse.ArgumentTypeError(f"boolean expected, got {v!r}")


def bool_or_auto(v):
    return "auto" if str(v).strip().lower() == "auto" else str2bool(v)


def gb_or_auto(v):
    return "auto" if str(v).strip().lower() == "auto" else float(v)


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="MI355X-native layer-sharded Llama scoring / generation")
    # ---- reference flags (main.py:31-46)
    p.add_argument("--model_path", type=str, default="./")
    p.add_argument("--prompt_pickle", type=str, required=True, help="Path to the input prompt pickle file")
    p.add_argument("--output_file", type=str, required=True, help="Path to the LLM output scores file")
    p.add_argument("--num_batch", type=int, default=1)
    p.add_argument("--layer_num_per_shard", type=int, default=1,
                   help="upper bound on layers per shard (balanced split)")
    p.add_argument("--storage_location", type=str, default="cpu", choices=["gpu", "cpu", "disk"],
                   help="'gpu': keep intermediate activations in HBM, 'cpu': pinned host RAM, 'disk': spill files")
    p.add_argument("--max_activation_in_cpu", type=int, default=100)
    p.add_argument("--data_parallel", type=str2bool, nargs="?", const=True, default=False,
                   help="multi-GPU: data parallel if true, model (pipeline) parallel otherwise")
    p.add_argument("--disk_folder", type=str, default="./temp",
                   help="folder for intermediate activation files in 'disk' mode")
    p.add_argument("--num_gen_token", type=int, default=1, help="how many new tokens to be generated")
    # ---- additive flags
    p.add_argument("--num_gpus", type=int, default=None, help="GPUs to use (default: all visible; 0 = CPU)")
    p.add_argument("--prefix_attention", choices=["bidirectional", "causal"], default="bidirectional",
                   help="prefix self-attention: reference-compatible bidirectional (default) or causal")
    p.add_argument("--sliding_window_mode", choices=["error", "apply"], default="error",
                   help="models with a sliding window (Mistral, Mixtral, Phi-3, Qwen with use_sliding_window) and a "
                        "prompt longer than it: error (default) refuses the call; apply runs sliding-window "
                        "attention (a query sees the last sliding_window positions, its own included; calls that "
                        "fit the window run unchanged)")
    p.add_argument("--score_mode", choices=["next_token", "loglik", "embed"], default="next_token",
                   help="next_token (default): the next-token distribution after each suffix ([n_s, 1, V] fp16 per "
                        "prompt).  loglik: log p(suffix | prefix), summed over the suffix's tokens in one pass "
                        "([n_s, 3] float32 per prompt: the sum, the token count, 1 if every token is the greedy "
                        "one); --output_file then holds the per-token log-probabilities.  Not with --num_gen_token "
                        "> 1, --hip_graphs, --prefix_kv_cache / --suffix_kv_cache true, --resume_dir or model "
                        "parallel.  embed: each suffix's pooled final-norm hidden state ([n_s, D] float32 per "
                        "prompt; --embed_pooling, --embed_dim, --embed_normalize); the pass ends at model.norm, so "
                        "a model directory without lm_head.safetensors runs.  Not with what loglik refuses, nor "
                        "with --do_sample, --score_top_k or --lookup_decoding")
    p.add_argument("--embed_pooling", choices=["last", "mean"], default=None,
                   help="with --score_mode embed: last (default): the final-norm row of the suffix's last token "
                        "(the row the LM head scores); mean: the fp32 mean of the final-norm rows of the suffix's "
                        "own tokens (the prefix is not pooled)")
    p.add_argument("--embed_dim", type=int, default=None, metavar="D",
                   help="with --score_mode embed: keep the first D columns (Matryoshka truncation); 1 to the hidden "
                        "size, 0 (default): the hidden size")
    p.add_argument("--embed_normalize", type=str2bool, nargs="?", const=True, default=None,
                   help="with --score_mode embed: divide each embedding by max(its L2 norm over the kept "
                        "columns, 1e-12) (default true)")
    p.add_argument("--do_sample", type=str2bool, nargs="?", const=True, default=False,
                   help="draw every generated token from the next-token distribution instead of taking its "
                        "argmax (temperature, then top-k, then top-p; integer-exact, so device and host draw the "
                        "same token: sampling.py).  The scores are unchanged; a run is a function of its prompts "
                        "and --seed.  Not with --score_mode loglik")
    p.add_argument("--temperature", type=float, default=1.0,
                   help="with --do_sample: sample from p^(1/T) renormalised (softmax(logits / T) over the tokens "
                        "whose fp16 probability is non-zero); > 0")
    p.add_argument("--top_k", type=int, default=0, help="with --do_sample: keep the k most probable tokens (0: off)")
    p.add_argument("--top_p", type=float, default=1.0,
                   help="with --do_sample: keep the shortest most-probable prefix holding this share of the "
                        "(temperature-weighted, top-k truncated) mass; in (0, 1]")
    p.add_argument("--seed", type=int, default=0, help="with --do_sample: the seed of every draw")
    p.add_argument("--score_top_k", type=int, default=0,
                   help="with --score_mode next_token: instead of the whole [n_s, steps, V] distribution, return "
                        "per suffix and step the K most probable (token id, fp16 probability) pairs, selected on "
                        "the device in rank order (probability descending, id ascending; topk.py), and the id and "
                        "probability of the appended token; the [rows, V] scores are never copied to the host.  "
                        "0 (default): off; at most 1024 and the vocabulary size.  Tokens, probabilities and "
                        "updated prompts are those of the run without the flag.  Not with --score_mode loglik, nor "
                        "with --do_sample on several GPUs or with --num_batch > 1")
    p.add_argument("--lookup_decoding", type=int, default=0, metavar="D",
                   help="prompt-lookup speculative generation: every call also scores up to D draft tokens per "
                        "suffix, guessed from the latest earlier occurrence of the text's last n-gram "
                        "(--lookup_ngram), and keeps those the greedy decoding produces itself, so a call can "
                        "yield up to D + 1 tokens per suffix.  Output files are those of the run without the flag "
                        "(every call is row-exact); only the number of calls changes.  0 (default): off; 1..16.  "
                        "Greedy, one GPU, --num_batch 1; not with --do_sample, --score_mode loglik, --hip_graphs, "
                        "--prefix_kv_cache / --suffix_kv_cache / --exact_reuse false or --resume_dir")
    p.add_argument("--lookup_ngram", type=int, default=3, metavar="N",
                   help="with --lookup_decoding: the longest n-gram tried (n = N .. 1, the first that occurs "
                        "earlier in the text decides); 1..8")
    p.add_argument("--hip_graphs", type=str2bool, nargs="?", const=True, default=False,
                   help="with --resident: capture each micro-batch's whole forward as one HIP graph and "
                        "replay it (shape-bucketed; removes per-op host dispatch for small batches)")
    p.add_argument("--prefix_kv_cache", type=bool_or_auto, nargs="?", const=True, default="auto",
                   help="keep every prompt's prefix K/V per layer in HBM and reuse it in later calls on the same "
                        "prefixes (each --num_gen_token step then computes only the suffix tokens; exact). "
                        "auto (default): on when --num_gen_token > 1")
    p.add_argument("--suffix_kv_cache", type=bool_or_auto, nargs="?", const=True, default="auto",
                   help="with the prefix K/V cache: also keep every suffix's K/V and, in the next call (generation "
                        "step), compute only the tokens after the longest common token prefix with the last call's "
                        "suffix (each step then costs its new tokens).  Exact: with the prefix cache every call runs "
                        "row-independent kernels, so a reused step's scores are bit for bit those of recomputing "
                        "every suffix token (PARITY.md C21).  auto (default): on with the prefix K/V cache on one GPU "
                        "without --max_vram_gb (capped steps are PCIe-bound: staging the suffix regions costs more "
                        "than recomputing the suffix tokens)")
    p.add_argument("--exact_reuse", type=str2bool, nargs="?", const=True, default=True,
                   help="with the K/V caches: run every call row-exact (default), so reused steps are bit for "
                        "bit the full recomputation; false: the faster small-M kernels (skinny / split-K GEMMs, "
                        "multi-suffix attention items), scores equal to rounding and tokens not guaranteed")
    p.add_argument("--prefix_cache_entries", type=int, default=8,
                   help="prefix K/V cache: calls (prompt batches) kept, LRU")
    p.add_argument("--resident", type=str2bool, nargs="?", const=True, default=False,
                   help="keep every shard resident in HBM after first load (288 GB fits 70B)")
    p.add_argument("--hbm_cache_gb", type=gb_or_auto, default="auto",
                   help="keep this many GB of shards resident in HBM after their first load, spread evenly "
                        "over the pass; the others stream every pass (generation steps with a partly "
                        "cached model move fewer bytes over PCIe).  auto (default): with repeated passes "
                        "over the same weights (--num_gen_token > 1 or --num_batch > 1) the free HBM minus "
                        "the activation plan (the whole 70B model on one 288 GB MI355X; data parallel: "
                        "resident all-gathered layers when they fit), else 0")
    p.add_argument("--weight_cache", choices=["auto", "host", "stream", "disk"], default="auto",
                   help="host: read every layer once into pinned host RAM (needs ~model-size RAM); "
                        "stream (alias disk, the reference behaviour): re-read the per-layer safetensors every "
                        "pass through a small pinned chunk ring (~256 MB of RAM) straight into HBM; "
                        "auto: host if it fits --host_mem_gb, else stream")
    p.add_argument("--host_mem_gb", type=float, default=None,
                   help="host RAM budget for --weight_cache auto / host (default: 80%% of MemAvailable)")
    p.add_argument("--o_direct", type=str2bool, nargs="?", const=True, default=False,
                   help="stream layer files with O_DIRECT (bypass the page cache)")
    p.add_argument("--dp_gather_comm", choices=["torch", "native"], default="torch",
                   help="data parallel: the weight all-gathers on a torch.distributed group (default) or on the "
                        "native RCCL communicator (csrc/comm/rccl_comm.cpp), issued from C on the copy stream")
    p.add_argument("--dp_weight_shard", type=str2bool, nargs="?", const=True, default=True,
                   help="data parallel: scatter-load 1/G of each layer per GPU + RCCL all-gather")
    p.add_argument("--rx_window", type=int, default=2,
                   help="model parallel: HBM receive-ring slots per rank (receives in flight at the point of use)")
    p.add_argument("--pipeline_stages", choices=["round_robin", "contiguous"], default="round_robin",
                   help="model parallel: shard k on GPU k mod G (reference) or one contiguous stage per GPU")
    p.add_argument("--token_budget", type=int, default=49152,
                   help="max tokens per packed micro-batch (MLP still runs in 16k-row chunks)")
    p.add_argument("--max_vram_gb", type=float, default=None,
                   help="HBM cap per GPU: sizes --token_budget and the MLP chunk to fit (reference: 70B in 6 GB)")
    p.add_argument("--dtype", choices=["float16", "float32"], default=None,
                   help="activation dtype (default fp16 on GPU, fp32 on CPU)")
    p.add_argument("--verbose", type=str2bool, nargs="?", const=True, default=False)
    p.add_argument("--metrics_json", type=str, default=None, help="write run metrics here (rank 0)")
    p.add_argument("--lora", type=str, default=None, metavar="DIR",
                   help="a LoRA adapter in PEFT's saved form (adapter_config.json + adapter_model.safetensors), merged "
                        "into the weights in HBM as they land (W += s B A, lora.py); the base checkpoint is read as it "
                        "is, fp16 / bf16, FP8, INT4 or NF4 (bitsandbytes 4-bit: the QLoRA base)")
    p.add_argument("--lora_scale", type=float, default=None,
                   help="multiplies the adapter's scale alpha / r (default 1.0; needs --lora)")
    p.add_argument("--max_token_len", type=int, default=None,
                   help="token cap per prefix / suffix (reference: 4096, utils.py:14); also sizes the RoPE tables")
    p.add_argument("--synthetic", type=str, default=None, metavar="PRESET",
                   help="random-init weights of a preset architecture (tiny|small|llama2-7b|llama2-13b|llama2-70b) "
                        "generated in pinned host RAM, plus a synthetic tokenizer; --model_path is not read")
    p.add_argument("--resume_dir", type=str, default=None,
                   help="checkpoint inter-shard activations here and resume a crashed run from them "
                        "(single-GPU, data-parallel and model-parallel)")
    p.add_argument("--checkpoint_every", type=int, default=8, help="shards between checkpoints (with --resume_dir)")
    p.add_argument("--profile", type=str2bool, nargs="?", const=True, default=False,
                   help="emit roctx ranges (shard load / micro-batch compute) for rocprofv3 --marker-trace")
    return p


def check_score_mode(args) -> None:
    """``--score_mode loglik`` refuses what it is not built for, naming the flag (``auto`` K/V
    caches resolve to off: they follow ``--num_gen_token``, which must be 1)."""
    if getattr(args, "score_mode", "next_token") != "loglik":
        return
    for bad, flag in ((getattr(args, "num_gen_token", 1) != 1, "--num_gen_token other than 1"),
                      (getattr(args, "hip_graphs", False), "--hip_graphs"),
                      (getattr(args, "prefix_kv_cache", False) is True, "--prefix_kv_cache true"),
                      (getattr(args, "suffix_kv_cache", False) is True, "--suffix_kv_cache true"),
                      (getattr(args, "resume_dir", None), "--resume_dir")):
        if bad:
            raise ValueError(f"--score_mode loglik does not combine with {flag}")


def check_embed(args, hidden_size: int = 0) -> None:
    """``--score_mode embed`` and the ``--embed_*`` flags: values in range (``--embed_dim`` against
    ``hidden_size`` once the model is known), no ``--embed_*`` flag without the mode, and none of
    the modes it is not built for; a ``ValueError`` names the flag."""
    from ..embed import check_embed_values
    pooling, dim, norm = (getattr(args, "embed_pooling", None), getattr(args, "embed_dim", None),
                          getattr(args, "embed_normalize", None))
    if getattr(args, "score_mode", "next_token") != "embed":
        for v, flag in ((pooling, "--embed_pooling"), (dim, "--embed_dim"), (norm, "--embed_normalize")):
            if v is not None:
                raise ValueError(f"{flag} needs --score_mode embed")
        return
    check_embed_values(pooling or "last", dim or 0)
    if hidden_size and (dim or 0) > hidden_size:
        raise ValueError(f"--embed_dim must be in 1..{hidden_size} (the hidden size), got {dim}")
    sampled = (getattr(args, "do_sample", False) or getattr(args, "temperature", 1.0) != 1.0
               or getattr(args, "top_k", 0) != 0 or getattr(args, "top_p", 1.0) != 1.0)
    for bad, flag in ((getattr(args, "num_gen_token", 1) != 1, "--num_gen_token other than 1"),
                      (sampled, "--do_sample (and --temperature / --top_k / --top_p)"),
                      (getattr(args, "score_top_k", 0), "--score_top_k"),
                      (getattr(args, "lookup_decoding", 0), "--lookup_decoding"),
                      (getattr(args, "hip_graphs", False), "--hip_graphs"),
                      (getattr(args, "prefix_kv_cache", False) is True, "--prefix_kv_cache true"),
                      (getattr(args, "suffix_kv_cache", False) is True, "--suffix_kv_cache true"),
                      (getattr(args, "resume_dir", None), "--resume_dir")):
        if bad:
            raise ValueError(f"--score_mode embed does not combine with {flag}")


def check_lora(args) -> None:
    """``--lora`` / ``--lora_scale``: one adapter directory, no scale without an adapter, and no
    adapter on ``--synthetic`` weights; a ``ValueError`` names the flag."""
    path, scale = getattr(args, "lora", None), getattr(args, "lora_scale", None)
    if scale is not None and not path:
        raise ValueError("--lora_scale needs --lora")
    if not path:
        return
    if isinstance(path, (list, tuple)):
        raise ValueError("--lora takes one adapter directory")
    if getattr(args, "synthetic", None):
        raise ValueError("--lora does not combine with --synthetic: there are no files to adapt, and the synthetic "
                         "store folds its norms as it generates")
    if scale is not None and not (scale == scale and abs(scale) != float("inf")):
        raise ValueError(f"--lora_scale {scale!r}: not finite")


def check_sampling(args) -> None:
    """The sampling flags: values in range, no sampling parameter without ``--do_sample``, no
    sampling inside ``--score_mode loglik``; a ``ValueError`` names the flag."""
    from ..sampling import check_sampling_values
    t, k, p = getattr(args, "temperature", 1.0), getattr(args, "top_k", 0), getattr(args, "top_p", 1.0)
    check_sampling_values(t, k, p)
    if not getattr(args, "do_sample", False):
        for v, default, flag in ((t, 1.0, "--temperature"), (k, 0, "--top_k"), (p, 1.0, "--top_p")):
            if v != default:
                raise ValueError(f"{flag} needs --do_sample (generation is greedy without it)")
        return
    if getattr(args, "score_mode", "next_token") == "loglik":
        raise ValueError("--do_sample does not combine with --score_mode loglik")


def check_top_k(args, world: int = 1) -> None:
    """``--score_top_k``: 0 (off) or 1..1024, in ``--score_mode next_token`` only, and not where
    sampled tokens are drawn on the host from the full rows (``--do_sample`` with several ranks
    or ``--num_batch > 1``); a ``ValueError`` names the flag.  The vocabulary bound is checked
    where the runner is built."""
    from ..topk import check_k
    k = getattr(args, "score_top_k", 0)
    if k == 0 and not isinstance(k, bool):
        return
    if isinstance(k, bool) or int(k) != k or k < 0:
        raise ValueError(f"--score_top_k must be an integer >= 0, got {k!r}")
    check_k(k)
    if getattr(args, "score_mode", "next_token") == "loglik":
        raise ValueError("--score_top_k does not combine with --score_mode loglik")
    if getattr(args, "do_sample", False) and (world > 1 or getattr(args, "num_batch", 1) > 1):
        raise ValueError("--score_top_k does not combine with --do_sample on several GPUs or with --num_batch > 1: "
                         "the host sampler needs the full rows")


def check_lookup(args, world: int = 1) -> None:
    """``--lookup_decoding`` / ``--lookup_ngram``: values in range, and with D > 0 none of the modes
    the verification is not built for — it is greedy, row-exact, on one rank and one batch; a
    ``ValueError`` names the flag."""
    from ..lookup import DEFAULT_NGRAM, check_lookup_values
    d, _ = check_lookup_values(getattr(args, "lookup_decoding", 0), getattr(args, "lookup_ngram", DEFAULT_NGRAM))
    if d == 0:
        return
    ngpu = getattr(args, "num_gpus", None)
    for bad, flag in ((getattr(args, "do_sample", False), "--do_sample (verification is greedy)"),
                      (getattr(args, "score_mode", "next_token") == "loglik", "--score_mode loglik"),
                      (getattr(args, "hip_graphs", False), "--hip_graphs"),
                      (getattr(args, "prefix_kv_cache", "auto") is False, "--prefix_kv_cache false"),
                      (getattr(args, "suffix_kv_cache", "auto") is False, "--suffix_kv_cache false"),
                      (getattr(args, "exact_reuse", True) is False, "--exact_reuse false"),
                      (getattr(args, "resume_dir", None), "--resume_dir"),
                      (world > 1 or (ngpu is not None and ngpu > 1), "more than one GPU (rank)"),
                      (getattr(args, "num_batch", 1) > 1, "--num_batch > 1")):
        if bad:
            raise ValueError(f"--lookup_decoding does not combine with {flag}")


def parse_args(argv=None):
    args = build_parser().parse_args(argv)
    check_score_mode(args)
    check_embed(args)
    check_sampling(args)
    check_top_k(args)
    check_lookup(args)
    check_lora(args)
    return args
