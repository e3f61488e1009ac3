"""End-to-end driver: ``main.py`` semantics on one process per GPU.

Reference (``/root/reference/main.py:52-98``): load the prompt pickle, split
it into ``--num_batch`` contiguous batches, run every batch through the
sharded model on all GPUs (threads; DP = ``np.array_split`` of prompts, MP =
the same list on every GPU), then ``--num_gen_token`` times extend every
suffix with the greedy argmax token (re-running the whole model each time),
and finally dump ``<prompts>_updated.pkl`` and the score list.

Here >1 GPU means >1 process (spawned by :func:`main` or launched by
``torchrun``), RCCL between them, and every rank runs the same loop; rank 0
owns the file I/O.
"""
from __future__ import annotations

import copy
import json
import os
import pickle
import socket
import sys
import tempfile
import time
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import gptq, knobs, quant
from .config import MAX_TOKEN_LEN, ModelConfig
from .classify import ClassifyParams
from .classify import pass_layer_names as mode_layer_names
from .embed import EmbedParams
from .engine import ShardedRunner
from .parallel.comm import Comm
from .parallel.planner import make_plan
from .runtime.stream import FileLayerSource
from .runtime.weights import HostStore
from .sampling import SamplingParams, draws as sample_draws, sample_tokens
from .utils.cli import (check_classify, check_embed, check_lookup, check_sampling, check_score_mode,
                        check_suffix_attention, check_top_k, parse_args)
from .utils.tokenizer import load_tokenizer


def batch_ranges(n: int, num_batch: int):
    """main.py:19-20 (contiguous batches; the last one takes the remainder)."""
    ends = [n // num_batch * i for i in range(1, num_batch)] + [n]
    return list(zip([0] + ends[:-1], ends))


def resolve_weight_cache(args, cfg: ModelConfig, comm: Comm, names: Sequence[str], sliced: bool,
                         source=None) -> str:
    """``--weight_cache`` -> ``host`` or ``stream``.

    ``auto`` pins the packed layers in host RAM only when they fit the host budget
    (``--host_mem_gb``, default 80% of MemAvailable shared by this node's ranks), and
    otherwise streams them from the layer files every pass — the reference's small-RAM mode
    (README: 70B with >= 8 GB RAM).  ``disk`` is the reference-named alias of ``stream``.
    An explicit ``host`` that cannot fit is rejected instead of being OOM-killed mid-load
    (e.g. ``--dp_weight_shard false`` would pin the whole model once per rank)."""
    from .models.layout import layer_kind, layer_layout
    from .runtime.stream import host_ram_available
    from .runtime.weights import piece_slices
    mode = getattr(args, "weight_cache", "auto")
    if getattr(args, "synthetic", None):
        return "host"                  # generated in host RAM; there are no files to stream
    if mode in ("disk", "stream"):
        return "stream"
    need = 0
    if source is not None and not sliced and source.quantized():
        # a quantised checkpoint is pinned as its file bytes (runtime.weights.CompactHostStore), not
        # as the fp16 image: a 70B FP8 model asks for about 70 GB instead of 138 GB, an INT4 one for 35 GB
        need = source.file_bytes(names)
        names = ()
    for n in names:
        lay = layer_layout(cfg, layer_kind(n))
        need += sum(p.chunk for p in piece_slices(lay, comm.world)) if sliced else lay.nbytes
    local = int(os.environ.get("LOCAL_WORLD_SIZE", comm.world))
    if getattr(args, "host_mem_gb", None):
        budget = int(args.host_mem_gb * 1e9) // max(1, local)
    else:
        budget = int(0.8 * host_ram_available()) // max(1, local)
    fits = budget <= 0 or need <= budget            # unknown RAM size: trust the user
    if mode == "host":
        if not fits:
            raise SystemExit(f"--weight_cache host needs {need / 1e9:.1f} GB of pinned RAM per rank, the budget "
                             f"is {budget / 1e9:.1f} GB: use --weight_cache stream (or auto)")
        return "host"
    return "host" if fits else "stream"


def load_lora(args, cfg: ModelConfig):
    """``--lora DIR`` (``--lora_scale X``) -> the loaded adapter (lora.LoraAdapter), or None."""
    from .utils.cli import check_lora
    check_lora(args)
    if not getattr(args, "lora", None):
        return None
    from .lora import LoraAdapter
    scale = getattr(args, "lora_scale", None)
    return LoraAdapter.load(cfg, args.lora, 1.0 if scale is None else float(scale))     # (0 is a scale)


def build_source(args, cfg: ModelConfig, comm: Comm, device: torch.device, lora=None):
    # (embed mode ends at model.norm: the LM head is neither planned nor read, and need not exist)
    names = mode_layer_names(cfg, getattr(args, "score_mode", "next_token"))
    plan = make_plan(len(names), args.layer_num_per_shard, comm.world, comm.rank, args.data_parallel,
                     getattr(args, "pipeline_stages", "round_robin"))
    mine = [names[i] for i in sorted({i for sh in plan.my_shards for i in sh})]
    # GPU: host-cached weights are kept with their RMSNorms folded into the projections (once, on
    # the device), which the fused-norm GEMMs read as they are (HostStore.fold_norms)
    fold = device.type == "cuda" and knobs.get_int("FLS_QKV_FOLD") == 1
    if getattr(args, "synthetic", None):
        return HostStore.synthetic(cfg, device, seed=0, pinned=device.type == "cuda", names=mine, fold_norms=fold)
    src = FileLayerSource(cfg, args.model_path, names=mine, direct=getattr(args, "o_direct", False))
    tensors = src.tensors()                # (every layer's plan is made now: a bad file is refused here)
    if tensors["gptq"] or tensors["awq"]:
        gptq.check_quantization_config(args.model_path)     # (bits, gptq_v2, AWQ's GEMV, desc_act)
    for f in quant.ALL_FORMATS:
        if tensors[f.name] and getattr(args, "verbose", False):
            print(f.verbose.format(n=tensors[f.name], ignored=len(src.ignored_scales())), file=sys.stderr)
    if resolve_weight_cache(args, cfg, comm, mine, sliced=False, source=src) == "stream":
        return src
    if src.quantized():
        # the files' bytes pinned as they are, FP8 as FP8; norms are folded as each layer lands
        from .runtime.weights import CompactHostStore
        return CompactHostStore(src, pinned=device.type == "cuda")
    st = HostStore.from_source(src, pinned=device.type == "cuda", names=mine)
    if lora is not None:
        st.merge_lora(lora, device)        # once, before the fold: (W + sBA) diag(norm)
    return st.fold_norms(device) if fold else st


def check_fp8_dp_shard(args, cfg: ModelConfig) -> None:
    """Data-parallel weight sharding streams 1/G byte slices of every layer image, which cut through
    tensors; an FP8 tensor loads whole (it is expanded in place in its own region), so an FP8
    checkpoint is refused there.  (``--dp_weight_shard false`` and model parallel load whole
    layers and are fine.)"""
    if getattr(args, "synthetic", None) or not getattr(args, "model_path", None):
        return
    names = mode_layer_names(cfg, getattr(args, "score_mode", "next_token"))
    src = FileLayerSource(cfg, args.model_path, names=names)
    tensors = src.tensors()
    for f in reversed(quant.ALL_FORMATS):
        if tensors[f.name]:
            raise ValueError(f"--dp_weight_shard true does not serve an {f.label} checkpoint (its 1/G byte slices cut "
                             "through tensors): pass --dp_weight_shard false, or run model parallel")


def repeated_passes(args) -> bool:
    """The same weights stream more than once per run (reference: every generation step and every
    batch re-streams the whole model, ``main.py:19-23,65-76``)."""
    return getattr(args, "num_gen_token", 1) > 1 or getattr(args, "num_batch", 1) > 1


def resolve_prefix_kv_cache(args) -> bool:
    """``--prefix_kv_cache auto``: on for greedy generation (exact: later steps re-score the same
    prefixes, runtime/prefix_cache.py).  Under ``--max_vram_gb`` the cache lives in pinned host
    memory (host mode: a staging buffer of one layer's K/V in HBM, planned by runtime/memplan.py);
    ``build_runner`` turns an auto cache off when the host lacks the memory for it."""
    v = getattr(args, "prefix_kv_cache", False)
    if v == "auto":
        return getattr(args, "num_gen_token", 1) > 1 and not getattr(args, "resume_dir", None)
    return bool(v)


# host mode may take at most this share of the host's available memory
HOST_KV_SHARE = 0.5


def host_kv_fits(nbytes: int) -> bool:
    import psutil
    return nbytes <= HOST_KV_SHARE * psutil.virtual_memory().available


def resolve_suffix_kv_cache(args, world: int = 1) -> bool:
    """``--suffix_kv_cache auto``: on whenever the prefix K/V cache is, on one rank, without a VRAM
    cap.  Under ``--max_vram_gb`` the caches live in host memory and a step is PCIe-bound (weights +
    staged K/V): the suffix regions add more bytes per step than recomputing the suffix tokens costs
    (70B, 32 prompts: 2.93 s per step with reuse against 2.84 s prefix-only, same tokens,
    profiles/r6_decode), so auto keeps the prefix cache only."""
    v = getattr(args, "suffix_kv_cache", False)
    if v == "auto":
        return resolve_prefix_kv_cache(args) and world == 1 and not getattr(args, "max_vram_gb", None)
    return bool(v)


def prefix_kv_bytes(cfg: ModelConfig, tok, prompts, n_decoders: int, elem: int = 2,
                    suffix_kv_cache: bool = False, growth: Optional[int] = None) -> int:
    """HBM the prefix K/V cache needs for ``prompts``: post-RoPE K and V of every prefix token, and
    with ``suffix_kv_cache`` every suffix's region too (its tokens + ``growth`` rows, default
    ``PrefixKVCache.SUFFIX_GROWTH``, as ``PrefixKVCache.begin`` sizes them), for every decoder layer
    this rank runs."""
    if tok is None or not prompts:
        return 0
    from .runtime.prefix_cache import PrefixKVCache
    n = sum(len(tok(p[0]).input_ids) for p in prompts)
    if suffix_kv_cache:
        for p in prompts:
            sfx = list(p[1])
            if sfx:
                g = PrefixKVCache.SUFFIX_GROWTH if growth is None else growth
                n += sum(len(ids) + g for ids in tok(sfx).input_ids)
    return n * 2 * cfg.num_key_value_heads * cfg.head_dim * elem * n_decoders


def auto_hbm_cache_bytes(args, cfg: ModelConfig, device: torch.device, reserve: int = 0,
                         n_slots: int = 3) -> int:
    """Free HBM minus this run's activation plan (weight slots, one micro-batch's activations and
    workspace, ``reserve`` — e.g. the prefix K/V cache — and a 4 GB margin)."""
    if device.type != "cuda":
        return 0
    from .runtime.memplan import DEVICE_OVERHEAD, activation_bytes, weight_slot_bytes
    free, _ = torch.cuda.mem_get_info(device)
    need = (weight_slot_bytes(cfg, args.layer_num_per_shard, n_slots)
            + activation_bytes(cfg, getattr(args, "token_budget", 49152), 16384)
            + DEVICE_OVERHEAD + reserve + int(4e9))
    return max(0, free - need)


def resolve_hbm_cache_gb(args, cfg: ModelConfig, device: torch.device, reserve: int = 0) -> float:
    """``--hbm_cache_gb auto``: repeated passes keep as many shards in HBM as fit (the 70B model
    in full on one MI355X, so only the first pass crosses PCIe); a single pass caches nothing."""
    v = getattr(args, "hbm_cache_gb", 0.0)
    if v != "auto":
        return float(v or 0.0)
    if (device.type != "cuda" or not repeated_passes(args) or getattr(args, "resident", False)
            or getattr(args, "max_vram_gb", None) or getattr(args, "resume_dir", None)):
        return 0.0
    return auto_hbm_cache_bytes(args, cfg, device, reserve) / 1e9


def build_runner(args, cfg: ModelConfig, device, comm: Comm, tok, prompts=None) -> ShardedRunner:
    device = torch.device(device)
    from .models.layout import layer_kind
    check_score_mode(args)             # (args built without parse_args too)
    check_sampling(args)
    check_top_k(args, comm.world)
    check_lookup(args, comm.world)
    check_embed(args, cfg.hidden_size)
    check_classify(args)
    check_suffix_attention(args)
    mode = getattr(args, "score_mode", "next_token")
    if mode in ("loglik", "embed", "classify") and comm.world > 1 and not args.data_parallel:
        raise ValueError(f"--score_mode {mode} does not combine with model parallel: pass --data_parallel")
    embed_kw = {}
    if mode == "embed":
        ep = EmbedParams.from_args(args)
        embed_kw = dict(embed_pooling=ep.pooling, embed_dim=ep.dim, embed_normalize=ep.normalize)
    if mode == "classify":
        cp = ClassifyParams.from_args(args)
        embed_kw = dict(classify_rows=cp.rows, classify_activation=cp.activation)
    lora = load_lora(args, cfg)
    pkv = resolve_prefix_kv_cache(args)
    skv = resolve_suffix_kv_cache(args, comm.world) and pkv
    n_dec = sum(1 for n in cfg.layer_names() if layer_kind(n) == "decoder")
    if not args.data_parallel and comm.world > 1:
        n_dec = -(-n_dec // comm.world)
    from .runtime.prefix_cache import suffix_growth
    # (prompt-lookup decoding: a suffix also holds up to D draft tokens)
    growth = suffix_growth(getattr(args, "num_gen_token", 1) + int(getattr(args, "lookup_decoding", 0) or 0))
    reserve = prefix_kv_bytes(cfg, tok, prompts, n_dec, suffix_kv_cache=skv, growth=growth) if pkv else 0
    if pkv and getattr(args, "max_vram_gb", None) and not host_kv_fits(reserve):
        # host mode (a VRAM cap): the cache's pinned host buffers
        msg = (f"the prefix K/V cache needs {reserve / 1e9:.1f} GB of pinned host memory (--max_vram_gb "
               f"keeps it on the host): more than {HOST_KV_SHARE:.0%} of the available memory")
        if getattr(args, "prefix_kv_cache", False) != "auto":
            raise ValueError(msg)
        print(msg + "; running without it", file=sys.stderr)
        pkv = skv = False
        reserve = 0
    if args.data_parallel and comm.world > 1 and args.dp_weight_shard:
        check_fp8_dp_shard(args, cfg)
        from .parallel.data_parallel import build_dp_sharded_runner
        hv = getattr(args, "hbm_cache_gb", 0.0)
        if hv not in ("auto", 0, 0.0, None):
            print("--hbm_cache_gb is not used with the data-parallel all-gather weight path", file=sys.stderr)
        if hv == "auto" and not args.resident and device.type == "cuda" and repeated_passes(args):
            # repeated passes: gather every layer once and keep it (resident) when the model fits
            from .models.layout import layer_layout
            model = sum(layer_layout(cfg, layer_kind(n)).nbytes for n in cfg.layer_names())
            if model <= auto_hbm_cache_bytes(args, cfg, device, reserve, n_slots=0):
                args = copy.copy(args)
                args.resident = True
        wc = resolve_weight_cache(args, cfg, comm, mode_layer_names(cfg, mode), sliced=True)
        return build_dp_sharded_runner(args, cfg, device, comm, tok, weight_cache=wc, prefix_kv_cache=pkv, lora=lora)
    src = build_source(args, cfg, comm, device, lora)
    act = None
    if args.dtype:
        act = torch.float16 if args.dtype == "float16" else torch.float32
    return ShardedRunner(cfg, src, device, tok, layer_num_per_shard=args.layer_num_per_shard,
                         storage_location=args.storage_location, disk_folder=args.disk_folder,
                         max_activation_in_cpu=args.max_activation_in_cpu,
                         prefix_attention=args.prefix_attention, token_budget=args.token_budget,
                         resident=args.resident, comm=comm, data_parallel=args.data_parallel,
                         act_dtype=act, verbose=args.verbose,
                         resume_dir=getattr(args, "resume_dir", None),
                         checkpoint_every=getattr(args, "checkpoint_every", 0),
                         max_token_len=getattr(args, "max_token_len", None) or MAX_TOKEN_LEN,
                         hip_graphs=getattr(args, "hip_graphs", False),
                         hbm_cache_gb=resolve_hbm_cache_gb(args, cfg, device, reserve),
                         prefix_kv_cache=pkv,
                         prefix_cache_entries=getattr(args, "prefix_cache_entries", 8),
                         suffix_kv_cache=skv, exact_reuse=getattr(args, "exact_reuse", True),
                         pipeline_stages=getattr(args, "pipeline_stages", "round_robin"),
                         rx_window=getattr(args, "rx_window", 2),
                         sliding_window_mode=getattr(args, "sliding_window_mode", "error"),
                         suffix_attention=getattr(args, "suffix_attention", "causal"),
                         score_mode=getattr(args, "score_mode", "next_token"),
                         max_vram_gb=getattr(args, "max_vram_gb", None),
                         # one rank draws the tokens on the device; several ranks: rank 0 draws the
                         # same tokens on the host from the gathered scores (generation_loop)
                         sampling=SamplingParams.from_args(args) if comm.world == 1 else None,
                         score_top_k=int(getattr(args, "score_top_k", 0) or 0), lora=lora, **embed_kw)


def load_model_meta(args):
    """(config, tokenizer) from --model_path, or a preset + synthetic tokenizer for --synthetic."""
    if getattr(args, "synthetic", None):
        from .config import preset
        from .utils.tokenizer import write_synthetic_tokenizer
        cfg = preset(args.synthetic)
        tok_dir = os.path.join(tempfile.gettempdir(), f"fls_synth_tok_{cfg.vocab_size}_{os.getpid()}")
        write_synthetic_tokenizer(tok_dir, cfg.vocab_size)
        return cfg, load_tokenizer(tok_dir)
    return ModelConfig.from_pretrained(args.model_path), load_tokenizer(args.model_path)


def run_all(args, runner: ShardedRunner, comm: Comm, prompts: Sequence) -> List[np.ndarray]:
    """One full pass over ``prompts`` on every rank; returns the ordered score list on rank 0."""
    if args.data_parallel and comm.world > 1:
        idx = np.array_split(np.arange(len(prompts)), comm.world)[comm.rank]
        mine = [prompts[i] for i in idx]
    else:
        mine = list(prompts)
    if not prompts:
        return []
    # data parallel with all-gathered weights: every rank runs num_batch passes, even over an
    # empty slice, so the weight collectives line up across ranks
    collective = getattr(runner.prefetcher, "collective", False)
    loglik = getattr(runner, "loglik", False)
    outs: List[np.ndarray] = []
    toks: list = []                    # loglik: every prompt's per-token log-probabilities
    for b0, b1 in batch_ranges(len(mine), args.num_batch):
        if b1 > b0 or collective:
            runner.prompt_base = b0        # (sampling on one rank: the draws take the prompt-file index)
            outs += runner(mine[b0:b1])
            if loglik:
                toks += runner.last_token_logprobs
    if loglik:
        # a few floats per prompt: gathered as objects (gather_scores packs fp16 and would round
        # them); rank 0's runner then holds the whole call's per-token values, in prompt order
        allv = comm.gather_object((outs, toks), dst=0)
        if comm.rank != 0:
            return []
        runner.last_token_logprobs = sum((t for _, t in allv), [])
        return sum((o for o, _ in allv), [])
    if comm.world == 1:
        return outs
    if getattr(runner, "embed", None) is not None or getattr(runner, "classify", None) is not None:
        # float32 [n_s, D] / [*, L] arrays: gathered as objects (gather_scores packs fp16 and would round them)
        allv = comm.gather_object(outs, dst=0)
        return sum(allv, []) if comm.rank == 0 else []
    if getattr(runner, "score_top_k", 0):
        # K (id, probability) pairs per row: gathered as objects (gather_scores packs fp16 and
        # cannot carry the ids)
        allv = comm.gather_object(outs, dst=0)
    else:
        allv = comm.gather_scores(outs, dst=0)
    if comm.rank != 0:
        return []
    if args.data_parallel:
        return sum(allv, [])
    # model parallel: the rank owning lm_head holds every score
    for v in allv:
        if v and all(x is not None for x in v):
            return v
    raise RuntimeError("no rank produced scores")


def generation_loop(args, runner, comm: Comm, tok, original_prompts: Sequence, step_times: Optional[list] = None,
                    token_record: Optional[dict] = None, drafter=None, lookup_stats: Optional[dict] = None):
    """main.py:63-90 — greedy extension of every suffix, one full pass per step (the prefix K/V
    cache and the HBM weight cache, on by default for repeated passes, make the later passes
    cheaper; the scores are the same).  ``step_times`` collects each step's wall time.
    ``--do_sample``: the appended token is drawn from the step's scores instead (sampling.py), on
    the device where the runner holds every prompt, else here on rank 0: the same tokens.
    ``--score_top_k``: every step's output is a ``TOPK_DTYPE`` [n_s, 1, K] array per prompt; rank 0
    fills ``token_record`` with ``token_ids`` (int64 [n_s, steps] per prompt, the appended
    tokens) and ``token_probs`` (float16, their probabilities).
    ``--lookup_decoding D``: :func:`lookup_generation_loop` — the same outputs in fewer calls;
    ``drafter`` (default ``lookup.lookup_draft``) proposes the draft tokens, ``lookup_stats``
    receives the call and acceptance counts."""
    if int(getattr(args, "lookup_decoding", 0) or 0) > 0:
        return lookup_generation_loop(args, runner, comm, tok, original_prompts, step_times, token_record,
                                      drafter, lookup_stats)
    input_prompts = copy.deepcopy(list(original_prompts))
    sampling = SamplingParams.from_args(args)
    top_k = int(getattr(runner, "score_top_k", 0) or 0)
    step_probs: List[List[np.ndarray]] = []          # score_top_k: per prompt, every step's [n_s, 1] fp16
    table = sampling.table() if sampling is not None and comm.rank == 0 else None
    # per prompt: every step's [n_s, 1, V] scores and argmax tokens.  The reference concatenates the
    # scores each step and takes the argmax over all of them (main.py:83-88); the argmax of the
    # earlier steps cannot change, so each step's is taken once, and the scores are concatenated
    # once at the end — same tokens, same output
    step_scores: List[List[np.ndarray]] = []
    step_tokens: List[List[np.ndarray]] = []
    # host-side profile of chosen steps (FLS_PROFILE_GEN_STEPS="2,3" -> cProfile stats in
    # gen_profile.<step>): where a generation step's host time goes
    prof_steps = {int(s) for s in knobs.get("FLS_PROFILE_GEN_STEPS").split(",") if s.strip()}
    # one runner call per step on one rank: each decode-graphed step may enqueue the next one behind
    # itself (ShardedRunner._launch_spec) while the host decodes and re-tokenizes
    spec = comm.world == 1 and len(batch_ranges(len(input_prompts), args.num_batch)) == 1
    pc = getattr(runner, "prefix_cache", None)
    if pc is not None:
        from .runtime.prefix_cache import suffix_growth
        pc.suffix_growth = suffix_growth(args.num_gen_token)      # suffix regions sized for this run
    for i_new in range(args.num_gen_token):
        t_step = time.perf_counter()
        if hasattr(runner, "spec_steps"):
            runner.spec_steps = (args.num_gen_token - 1 - i_new) if spec else 0
        runner.sample_step = i_new
        prof = None
        if i_new in prof_steps:
            import cProfile
            prof = cProfile.Profile()
            prof.enable()
        outputs = run_all(args, runner, comm, input_prompts)
        # the greedy tokens the runner took on the device (one rank holding every prompt), else a
        # host argmax over the gathered scores
        dev_tok = getattr(runner, "last_tokens", None) if comm.world == 1 else None
        if not dev_tok or len(dev_tok) != len(outputs) or any(t is None for t in dev_tok):
            dev_tok = None
        if prof is not None:
            prof.disable()
            prof.dump_stats(f"gen_profile.{i_new}")
        if comm.rank == 0:
            if top_k:
                if dev_tok is not None:
                    probs_t = list(runner.last_token_probs)
                elif sampling is not None:
                    raise RuntimeError("--score_top_k with --do_sample needs the tokens drawn on the device")
                else:
                    # the greedy token is the first ranked entry (several ranks or batches)
                    probs_t = [o["p"][:, :, 0] for o in outputs]
                for pi, pt in enumerate(probs_t):
                    step_probs.append([pt]) if i_new == 0 else step_probs[pi].append(pt)
            if dev_tok is not None:
                toks = dev_tok
            elif top_k:
                toks = [o["id"][:, :, 0].astype(np.int64) for o in outputs]
            elif sampling is None:
                toks = [greedy_tokens(o) for o in outputs]
            else:
                toks = [sample_tokens(o[:, 0, :], table, sampling.top_k, sampling.P,
                                      sample_draws(sampling.seed, [pi], [o.shape[0]], i_new)).reshape(-1, 1)
                        for pi, o in enumerate(outputs)]
            if i_new == 0:
                step_scores = [[o] for o in outputs]
                step_tokens = [[t] for t in toks]
            else:
                for pi, o in enumerate(outputs):
                    step_scores[pi].append(o)
                    step_tokens[pi].append(toks[pi])
            # s + tok.decode(t) for every suffix (main.py:86-88), the decodes in one batched call
            news = [np.concatenate(step_tokens[pi], axis=1) for pi in range(len(input_prompts))]
            flat = [t for nt in news for t in nt]
            texts = iter(tok.batch_decode(flat) if hasattr(tok, "batch_decode") else [tok.decode(t) for t in flat])
            for pi in range(len(input_prompts)):
                prefix, suffix = original_prompts[pi]
                input_prompts[pi] = (prefix, tuple(s + next(texts) for s in suffix))
        if comm.world > 1:
            input_prompts = comm.broadcast_object(input_prompts, src=0)
        if step_times is not None:
            step_times.append(time.perf_counter() - t_step)
        if getattr(args, "verbose", False) and comm.rank == 0:
            print(f"step {i_new}: {time.perf_counter() - t_step:.3f}s", flush=True)
    output_scores = [ss[0] if len(ss) == 1 else np.concatenate(ss, axis=1) for ss in step_scores]
    if top_k and token_record is not None:
        token_record["token_ids"] = [np.concatenate(ts, axis=1).astype(np.int64) for ts in step_tokens]
        token_record["token_probs"] = [np.concatenate(ps, axis=1).astype(np.float16) for ps in step_probs]
    return output_scores, input_prompts


def lookup_generation_loop(args, runner, comm: Comm, tok, original_prompts: Sequence,
                           step_times: Optional[list] = None, token_record: Optional[dict] = None, drafter=None,
                           lookup_stats: Optional[dict] = None):
    """``--lookup_decoding D``: greedy generation in fewer calls, same outputs (lookup.py).

    Every call submits, per suffix with g tokens generated so far, ``s + decode(generated + draft)``
    (the reference's decode rule, main.py:86-88) with ``draft = drafter(prefix + suffix + generated
    ids, N, d)[:d]``, d = min(D, num_gen_token - g - 1).  A draft whose text does not re-tokenize to
    the ids of ``s + decode(generated)`` followed by the draft is dropped for the call (counted).
    The runner scores each suffix's last ``len(draft) + 1`` rows and keeps the accepted draft
    positions and the one after them (``ShardedRunner.run_tokenized(drafts=...)``): the suffix
    gains their greedy tokens and keeps their scores, which — every call being row-exact — are
    those the one-token-per-call loop computes, as long as decoding and re-tokenizing is
    prefix-stable (``lookup_retokenized`` counts the suffixes whose next call's ids are not the
    scored ids plus the gained tokens).  A finished suffix rides along with an empty draft
    (its scores are discarded); a call without any draft takes the plain path.  One rank, one batch."""
    from .lookup import DEFAULT_NGRAM, check_lookup_values, lookup_draft
    from .runtime.prefix_cache import suffix_growth
    from .utils.tokenizer import TokenizedPrompt
    D, N = check_lookup_values(getattr(args, "lookup_decoding", 0), getattr(args, "lookup_ngram", DEFAULT_NGRAM))
    if comm.world != 1 or getattr(args, "num_batch", 1) != 1:
        raise ValueError("--lookup_decoding runs on one rank with --num_batch 1")
    drafter = drafter or lookup_draft
    G = int(args.num_gen_token)
    top_k = int(getattr(runner, "score_top_k", 0) or 0)
    n_p = len(original_prompts)
    gen = [[[] for _ in sfx] for _, sfx in original_prompts]           # generated ids
    kept_scores = [[[] for _ in sfx] for _, sfx in original_prompts]   # their [rows, V] scores, call by call
    kept_probs = [[[] for _ in sfx] for _, sfx in original_prompts]    # score_top_k: the tokens' probabilities
    input_prompts = copy.deepcopy(list(original_prompts))
    pc = getattr(runner, "prefix_cache", None)
    if pc is not None:
        pc.suffix_growth = suffix_growth(G + D)           # a suffix region also holds a call's draft
    if hasattr(runner, "spec_steps"):
        runner.spec_steps = 0                             # no speculative decode-graph step
    stats = {"lookup_calls": 0, "lookup_drafted": 0, "lookup_accepted": 0, "lookup_dropped_roundtrip": 0,
             "lookup_retokenized": 0}
    # ids every suffix is expected to re-tokenize to in the next call: the ids its last call's scores
    # were computed on, followed by the tokens it gained
    expected = [[None for _ in sfx] for _, sfx in original_prompts]
    decode = (lambda seqs: tok.batch_decode(seqs)) if hasattr(tok, "batch_decode") else (
        lambda seqs: [tok.decode(t) for t in seqs])
    while n_p and any(len(g) < G for gp in gen for g in gp):
        t_step = time.perf_counter()
        runner.sample_step = stats["lookup_calls"]
        runner.prompt_base = 0
        base = runner.tokenize(input_prompts)            # ids of s + decode(generated)
        # The scores of an accepted position j were computed on base + draft[:j]; the plain loop
        # computes them on the ids of s + decode(generated + draft[:j]).  The round trip below
        # checks the whole draft only: where decoding and re-tokenizing is not prefix-stable (a
        # merging tokenizer) the two can differ, which shows here, one call later, and is counted
        for pi, tp in enumerate(base):
            for si, ids in enumerate(tp.suffixes):
                if expected[pi][si] is not None and list(ids) != expected[pi][si]:
                    stats["lookup_retokenized"] += 1
        drafts = []
        for pi, tp in enumerate(base):
            row = []
            for si, ids in enumerate(tp.suffixes):
                room = min(D, G - len(gen[pi][si]) - 1)
                d = drafter(np.asarray(list(tp.prefix) + list(ids), dtype=np.int64), N, room) if room > 0 else ()
                row.append([int(t) for t in d][:max(room, 0)])
            drafts.append(row)
        tps = base
        if any(d for row in drafts for d in row):
            flat = [gen[pi][si] + d for pi, row in enumerate(drafts) for si, d in enumerate(row)]
            texts = iter(decode(flat))
            drafted = [(p, tuple(s + next(texts) for s in sfx)) for p, sfx in original_prompts]
            with_d = runner.tokenize(drafted)
            tps = []
            for pi, (tb, td) in enumerate(zip(base, with_d)):
                sfxs = []
                for si, d in enumerate(drafts[pi]):
                    if d and list(td.suffixes[si]) != list(tb.suffixes[si]) + d:
                        stats["lookup_dropped_roundtrip"] += 1
                        drafts[pi][si] = d = []
                    sfxs.append(list(tb.suffixes[si]) + d)
                tps.append(TokenizedPrompt(list(tb.prefix), sfxs, max((len(x) for x in sfxs), default=0),
                                           [len(x) - 1 for x in sfxs]))
        if any(d for row in drafts for d in row):
            outs = runner.run_tokenized(tps, drafts=drafts)
            toks = runner.last_tokens
            probs = runner.last_token_probs if top_k else None
        else:
            # no draft in this call: today's path, one scored row per suffix
            full = runner.run_tokenized(base)
            dev_tok = getattr(runner, "last_tokens", None)
            if not dev_tok or len(dev_tok) != len(full) or any(t is None for t in dev_tok):
                dev_tok = ([o["id"][:, :, 0].astype(np.int64) for o in full] if top_k
                           else [greedy_tokens(o) for o in full])
            outs = [[o[si] for si in range(o.shape[0])] for o in full]
            toks = [[t[si] for si in range(t.shape[0])] for t in dev_tok]
            probs = None
            if top_k:
                pt = runner.last_token_probs
                if not pt or any(x is None for x in pt):
                    pt = [o["p"][:, :, 0] for o in full]
                probs = [[x[si] for si in range(x.shape[0])] for x in pt]
        stats["lookup_calls"] += 1
        for pi in range(n_p):
            for si, d in enumerate(drafts[pi]):
                g = gen[pi][si]
                if len(g) >= G:
                    continue                              # finished: rode along, scores discarded
                t = [int(x) for x in np.asarray(toks[pi][si]).reshape(-1)]
                take = min(len(t), G - len(g))
                stats["lookup_drafted"] += len(d)
                stats["lookup_accepted"] += len(t) - 1
                g.extend(t[:take])
                expected[pi][si] = list(base[pi].suffixes[si]) + t[:take]
                kept_scores[pi][si].append(np.asarray(outs[pi][si])[:take])
                if top_k:
                    kept_probs[pi][si].append(np.asarray(probs[pi][si]).reshape(-1)[:take])
        flat = [g for gp in gen for g in gp]
        texts = iter(decode(flat))
        input_prompts = [(p, tuple(s + next(texts) for s in sfx)) for p, sfx in original_prompts]
        if step_times is not None:
            step_times.append(time.perf_counter() - t_step)
        if getattr(args, "verbose", False):
            print(f"call {stats['lookup_calls'] - 1}: {time.perf_counter() - t_step:.3f}s, "
                  f"{stats['lookup_accepted']} of {stats['lookup_drafted']} draft tokens accepted so far", flush=True)
    if lookup_stats is not None:
        lookup_stats.update(stats)
    # [n_s, num_gen_token, V] (score_top_k: K) per prompt, as the one-token-per-call loop returns
    output_scores = [np.stack([np.concatenate(rows, axis=0) for rows in ks], axis=0) if ks else np.zeros((0, G, 0))
                     for ks in kept_scores]
    if top_k and token_record is not None:
        token_record["token_ids"] = [np.asarray(gp, dtype=np.int64).reshape(len(gp), G) for gp in gen]
        token_record["token_probs"] = [np.stack([np.concatenate(x) for x in kp], axis=0).astype(np.float16)
                                       if kp else np.zeros((0, G), np.float16) for kp in kept_probs]
    return output_scores, input_prompts


def greedy_tokens(scores: np.ndarray) -> np.ndarray:
    """np.argmax(scores, axis=-1) (first index on ties).  fp16 probabilities are >= 0, whose bit
    patterns order like their values: the argmax runs on the uint16 view (numpy has no fast fp16
    compare: ~30x faster at [160, 1, 32000])."""
    if scores.dtype == np.float16:
        bits = scores.view(np.uint16)
        if not (bits >= 0x8000).any():
            return np.argmax(bits, axis=-1)
    return np.argmax(scores, axis=-1)


def _device_for(args, comm: Comm) -> torch.device:
    if comm.world > 1:
        return comm.device
    n = torch.cuda.device_count() if args.num_gpus is None else args.num_gpus
    return torch.device("cuda", 0) if n > 0 and torch.cuda.is_available() else torch.device("cpu")


def run_rank(args, comm: Comm) -> Optional[dict]:
    if getattr(args, "profile", False):
        from .utils import trace
        trace.enable(True)
    device = _device_for(args, comm)
    if args.storage_location == "disk":
        os.makedirs(args.disk_folder, exist_ok=True)
    with open(args.prompt_pickle, "rb") as f:
        original = pickle.load(f)      # the user's own prompt file (reference format)
    cfg, tok = load_model_meta(args)
    t0 = time.perf_counter()
    runner = build_runner(args, cfg, device, comm, tok, original)
    t_build = time.perf_counter() - t0
    t1 = time.perf_counter()
    step_times: List[float] = []
    lk: dict = {}                      # --lookup_decoding: call and acceptance counts
    if getattr(args, "score_mode", "next_token") == "loglik":
        # one scoring pass, no greedy token to append: the prompts are written back as they came;
        # the output file holds the [n_s, 3] arrays and the per-token log-probabilities
        summary = run_all(args, runner, comm, list(original))
        scores = {"scores": summary, "token_logprobs": list(runner.last_token_logprobs) if comm.rank == 0 else []}
        updated = copy.deepcopy(list(original))
        step_times.append(time.perf_counter() - t1)
    elif getattr(args, "score_mode", "next_token") == "embed":
        # one pass, no token to append: the prompts are written back as they came; the output file
        # holds the [n_s, D] float32 embeddings and how they were pooled
        ep = runner.embed
        scores = {"embeddings": run_all(args, runner, comm, list(original)), "pooling": ep.pooling, "dim": ep.dim,
                  "normalized": ep.normalize}
        updated = copy.deepcopy(list(original))
        step_times.append(time.perf_counter() - t1)
    elif getattr(args, "score_mode", "next_token") == "classify":
        # one pass, no token to append: the prompts are written back as they came; the output file
        # holds the head's float32 values ([n_s, L] per prompt, or per suffix [len_s, L]) and how they
        # were taken
        cp = runner.classify
        scores = {"logits": run_all(args, runner, comm, list(original)), "rows": cp.rows,
                  "activation": cp.activation, "num_labels": cp.num_labels}
        updated = copy.deepcopy(list(original))
        step_times.append(time.perf_counter() - t1)
    else:
        rec: dict = {}
        scores, updated = generation_loop(args, runner, comm, tok, original, step_times, token_record=rec,
                                          lookup_stats=lk)
        if getattr(runner, "score_top_k", 0):
            # compact scores: the K best (id, probability) pairs of every suffix and step, and the
            # appended tokens with their probabilities
            scores = {"k": runner.score_top_k,
                      "top_ids": [np.ascontiguousarray(o["id"]) for o in scores],
                      "top_probs": [np.ascontiguousarray(o["p"]) for o in scores],
                      "token_ids": rec.get("token_ids", []), "token_probs": rec.get("token_probs", [])}
    t_run = time.perf_counter() - t1
    tokens = comm.all_reduce_sum(runner.stats.get("tokens", 0.0)) if not (
        comm.world > 1 and not args.data_parallel) else runner.stats.get("tokens", 0.0)
    metrics = {"device": str(device), "world": comm.world, "build_s": t_build, "run_s": t_run,
               "step_s": step_times, "tokens_last_pass": tokens, "stats": runner.stats,
               "hbm_cache_kept_shards": len(getattr(runner.prefetcher, "_sticky", ())),
               "prefix_kv_cache": runner.prefix_cache is not None}
    sampling = SamplingParams.from_args(args)
    metrics["sampling"] = sampling.as_dict() if sampling is not None else {"do_sample": False}
    metrics["score_top_k"] = int(getattr(runner, "score_top_k", 0))
    metrics["score_mode"] = getattr(runner, "score_mode", "next_token")
    if getattr(runner, "embed", None) is not None:
        metrics.update({"embed_pooling": runner.embed.pooling, "embed_dim": runner.embed.dim,
                        "embed_normalize": runner.embed.normalize})
    if getattr(runner, "classify", None) is not None:
        metrics.update({"classify_rows": runner.classify.rows, "classify_activation": runner.classify.activation,
                        "num_labels": runner.classify.num_labels})
    if getattr(args, "lookup_decoding", 0):
        metrics["lookup_decoding"] = int(args.lookup_decoding)
        metrics["lookup_ngram"] = int(getattr(args, "lookup_ngram", 3))
        metrics.update({k: int(v) for k, v in lk.items()})
    src = runner.src
    files = getattr(src, "files", src)        # (a compact store wraps its file source)
    # tensor bytes a pass reads and copies (a packed host store: its images), and how many are FP8
    metrics["weight_file_bytes"] = int(files.file_bytes() if hasattr(files, "file_bytes")
                                       else getattr(src, "total_bytes", 0))
    tensors = files.tensors() if hasattr(files, "tensors") else {}
    metrics.update({f"{f.name}_tensors": int(tensors.get(f.name, 0)) for f in quant.ALL_FORMATS})
    ad = getattr(runner, "lora", None)
    metrics.update({"lora_tensors": int(ad.n_tensors) if ad else 0, "lora_rank_max": int(ad.rank_max) if ad else 0,
                    "lora_bytes": int(ad.nbytes) if ad else 0, "lora_merge_launches": int(ad.merge_launches) if ad else 0})
    metrics["weight_pinned_bytes"] = int(src.pinned_bytes() if hasattr(src, "pinned_bytes")
                                         else getattr(src, "total_bytes", 0))
    metrics["score_d2h_bytes_last_pass"] = int(getattr(runner, "score_d2h_bytes", 0))
    if device.type == "cuda":
        metrics["peak_hbm_bytes"] = torch.cuda.max_memory_allocated(device)
    if comm.rank == 0:
        if args.data_parallel and comm.world > 1:
            updated = np.array(updated, dtype=object)   # reference quirk: main.py:69 makes it an ndarray
        with open(args.prompt_pickle.replace(".pkl", "_updated.pkl"), "wb") as f:
            pickle.dump(updated, f)
        with open(args.output_file, "wb") as f:
            pickle.dump(scores, f)
        if args.verbose:
            print(json.dumps(metrics, default=float))
        if args.metrics_json:
            with open(args.metrics_json, "w") as f:
                json.dump(metrics, f, default=float, indent=1)
    runner.close()
    return metrics


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _spawn_worker(local_rank: int, world: int, port: int, argv: List[str]):
    os.environ.update({"RANK": str(local_rank), "LOCAL_RANK": str(local_rank), "WORLD_SIZE": str(world),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    args = parse_args(argv)
    comm = Comm.from_env("cuda")
    try:
        run_rank(args, comm)
    finally:
        comm.destroy()


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    args = parse_args(argv)
    print(args)
    if "WORLD_SIZE" in os.environ and int(os.environ["WORLD_SIZE"]) > 1:
        comm = Comm.from_env("cuda" if torch.cuda.device_count() > 0 else "cpu")
        try:
            run_rank(args, comm)
        finally:
            comm.destroy()
        return 0
    n = torch.cuda.device_count() if args.num_gpus is None else args.num_gpus
    if n > 1:
        import torch.multiprocessing as mp
        port = _free_port()
        mp.start_processes(_spawn_worker, args=(n, port, argv), nprocs=n, start_method="spawn", join=True)
        return 0
    run_rank(args, Comm(0, 1))
    return 0
