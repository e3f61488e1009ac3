"""Sliding-window attention on the CPU: the engine against HF transformers (causal) and the fp32
oracle (bidirectional prefixes), the window arrays the packer hands the kernel against the windowed
segments, the tolerance argument of the GPU per-row tests (tests/attention_window.py), and
generation with suffix K/V reuse under a window."""
import argparse

import numpy as np
import pytest
import torch

import attention_rows as ar
import attention_window as aw
from flexible_llm_sharding_amd.config import preset
from flexible_llm_sharding_amd.engine import ShardedRunner
from flexible_llm_sharding_amd.models.reference import reference_scores
from flexible_llm_sharding_amd.ops.torch_backend import TorchOps
from flexible_llm_sharding_amd.runtime.stream import FileLayerSource
from flexible_llm_sharding_amd.runtime.weights import HostStore
from flexible_llm_sharding_amd.utils.synthetic import (load_full_state_dict, synthetic_prompts,
                                                       write_synthetic_checkpoint)
from flexible_llm_sharding_amd.utils.tokenizer import load_tokenizer, tokenize_prompt, write_synthetic_tokenizer

W_TINY = 8


def _hf_windowed(tmp_path, family):
    """Tiny random Mistral / Phi-3 checkpoint with sliding_window=8 + its HF model (built as
    test_engine_cpu._hf_family_case builds them)."""
    transformers = pytest.importorskip("transformers")
    if family == "phi3":
        cfg = preset("tiny-phi3", sliding_window=W_TINY)
        rs = dict(cfg.rope_scaling or {"rope_type": "default"}, rope_theta=cfg.rope_theta)
        hf_cfg = transformers.Phi3Config(
            hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
            num_attention_heads=cfg.num_attention_heads, num_key_value_heads=cfg.num_key_value_heads,
            num_hidden_layers=cfg.num_hidden_layers, vocab_size=cfg.vocab_size, rms_norm_eps=cfg.rms_norm_eps,
            max_position_embeddings=cfg.max_position_embeddings, original_max_position_embeddings=4096,
            rope_parameters=rs, sliding_window=cfg.sliding_window, tie_word_embeddings=False, pad_token_id=0)
        model = transformers.Phi3ForCausalLM(hf_cfg)
    else:
        cfg = preset("tiny", model_type="mistral", architectures=["MistralForCausalLM"], rope_theta=1e6,
                     sliding_window=W_TINY)
        hf_cfg = transformers.MistralConfig(
            hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
            num_attention_heads=cfg.num_attention_heads, num_key_value_heads=cfg.num_key_value_heads,
            num_hidden_layers=cfg.num_hidden_layers, vocab_size=cfg.vocab_size, rms_norm_eps=cfg.rms_norm_eps,
            rope_theta=cfg.rope_theta, max_position_embeddings=cfg.max_position_embeddings,
            tie_word_embeddings=False, sliding_window=W_TINY)
        model = transformers.MistralForCausalLM(hf_cfg)
    path = str(tmp_path / family)
    write_synthetic_checkpoint(cfg, path, seed=5, std=0.05)
    write_synthetic_tokenizer(path, cfg.vocab_size)
    sd = load_full_state_dict(cfg, path)
    missing, unexpected = model.float().eval().load_state_dict({k: v.float() for k, v in sd.items()}, strict=False)
    assert not unexpected and all("rotary" in m for m in missing), (missing, unexpected)
    return path, cfg, sd, model


@pytest.mark.parametrize("family", ["mistral", "phi3"])
def test_windowed_scores_match_hf_and_oracle(tmp_path, family):
    """sliding_window=8 on ~20-token prefixes + 5-token suffixes: causal mode == HF transformers
    (2e-3, the bound of test_other_llama_families_match_hf), bidirectional-prefix mode ==
    reference_scores (1e-4); the default mode still refuses the call."""
    path, cfg, sd, model = _hf_windowed(tmp_path, family)
    tok = load_tokenizer(path)
    prompts = synthetic_prompts(3, 20, 2, 5, cfg.vocab_size, seed=9, vary=True)
    with pytest.raises(ValueError, match="sliding-window attention is not implemented"):
        ShardedRunner(cfg, FileLayerSource(cfg, path), "cpu", tok, prefix_attention="causal")(prompts)
    out = ShardedRunner(cfg, FileLayerSource(cfg, path), "cpu", tok, prefix_attention="causal",
                        sliding_window_mode="apply")(prompts)
    differs = 0.0
    full = reference_scores(preset_without_window(cfg), sd, tok, prompts, prefix_attention="causal")
    for (prefix, sufs), o, f in zip(prompts, out, full):
        tp = tokenize_prompt(tok, prefix, sufs)
        assert len(tp.prefix) + max(len(s) for s in tp.suffixes) > W_TINY
        for j, s in enumerate(tp.suffixes):
            with torch.no_grad():
                logits = model(torch.tensor([tp.prefix + s])).logits[0, -1].float()
            assert np.abs(o[j, 0].astype(np.float32) - torch.softmax(logits, -1).numpy()).max() < 2e-3
        differs = max(differs, float(np.abs(o.astype(np.float32) - f).max()))
    assert differs > 2e-3          # the window changes these scores: full attention would not pass
    bid = ShardedRunner(cfg, FileLayerSource(cfg, path), "cpu", tok, layer_num_per_shard=2,
                        sliding_window_mode="apply")(prompts)
    for o, rf in zip(bid, reference_scores(cfg, sd, tok, prompts)):
        assert np.abs(o.astype(np.float32) - rf).max() < 1e-4
    # the grouped attention phase (--max_vram_gb) carries the window arrays too
    r = ShardedRunner(cfg, FileLayerSource(cfg, path), "cpu", tok, sliding_window_mode="apply")
    r.ctx.attn_rows = 30
    for a, b in zip(r(prompts), ShardedRunner(cfg, FileLayerSource(cfg, path), "cpu", tok,
                                              sliding_window_mode="apply")(prompts)):
        assert np.abs(a.astype(np.float32) - b.astype(np.float32)).max() < 1e-5


def preset_without_window(cfg):
    import dataclasses
    return dataclasses.replace(cfg, sliding_window=None)


def test_window_covering_the_call_is_the_unwindowed_path(tmp_path):
    """W >= the longest sequence under ``apply``: bitwise the scores of the same config without
    sliding_window, and the batches carry no window arrays."""
    cfg = preset("tiny", sliding_window=64)
    write_synthetic_tokenizer(str(tmp_path), cfg.vocab_size)
    tok = load_tokenizer(str(tmp_path))
    store = HostStore.synthetic(cfg, "cpu", seed=1)
    prompts = synthetic_prompts(3, 30, 2, 8, cfg.vocab_size, seed=2, vary=True)
    r = ShardedRunner(cfg, store, "cpu", tok, sliding_window_mode="apply")
    tps = r.tokenize(prompts)
    assert max(len(tp.prefix) + max(len(s) for s in tp.suffixes) for tp in tps) <= 64
    assert r._call_window(tps) == 0
    plain = ShardedRunner(preset_without_window(cfg), HostStore.synthetic(preset_without_window(cfg), "cpu", seed=1),
                          "cpu", tok)
    for a, b in zip(r(prompts), plain(prompts)):
        assert np.array_equal(a, b)
    from flexible_llm_sharding_amd.runtime.batch import pack_prompts
    b = pack_prompts(tps, [0, 1, 2], window=r._call_window(tps))
    assert not {"r0_lo", "r0_item", "r0_item_last"} & set(b.host_meta())
    assert b.r0_lo is None and all(sg.window == 0 for sg in b.segments)
    assert set(pack_prompts(tps, [0, 1, 2], window=40).host_meta()) >= {"r0_lo", "r0_item", "r0_item_last"}
    with pytest.raises(ValueError):
        ShardedRunner(cfg, store, "cpu", tok, sliding_window_mode="maybe")


CASES = aw.cases()
IDS = [c[0] for c in CASES]
ARGS = [c[1] for c in CASES]


def _assert_same_masks(got, want):
    assert len(got) == len(want)
    for row, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None), f"row {row}: queried by one side only"
        if w is not None:
            assert len(w) > 0, f"row {row}: no visible key"
            assert np.array_equal(g, w), f"row {row}: work items and segments see different keys"


@pytest.mark.parametrize("args", ARGS, ids=IDS)
def test_work_items_describe_the_windowed_segments(args):
    """The keys visible_keys gives each row under the windowed work items (seg_lo, r2win, r0_lo; the
    pruned forms too) are the keys the windowed Segment masks give it; every bound lies inside the
    tiles its item walks, range-2 walks start on the unwindowed 64-row tile grid, and the K/V cache
    rows no item walks are not visible to any row."""
    c = aw.wcase(*args)
    b, T = c.b, c.b.num_tokens
    reuse = c.kind == "reuse"
    to_cache = None
    if reuse:
        to_cache = np.full(T, -1, dtype=np.int64)
        to_cache[b.sfx_src] = b.sfx_dst
    cached = c.kv0 is not None
    _assert_same_masks(aw.work_item_masks(b, b.work, b.work2, T, reuse),
                       aw.segment_masks(b.segments, cached, T, to_cache))
    _assert_same_masks(aw.work_item_masks(b, b.work_last, b.work2_last, T, reuse),
                       aw.segment_masks(b.last_segments, cached, T, to_cache))
    assert b.r0_lo.dtype == np.int32 and b.r0_lo.shape == (T,)
    for work, r0i, w2, w2_plain in ((b.work, b.r0_item, b.work2, c.base.b.work2),
                                    (b.work_last, b.r0_item_last, b.work2_last, c.base.b.work2_last)):
        assert r0i.dtype == np.int32 and r0i.shape == (work.shape[0], 2)
        for it, w in enumerate(work.tolist()):
            rows = b.r0_lo[w[0]:w[0] + w[1]]
            assert (rows >= 0).all() and (rows <= w[4]).all()
            assert int(r0i[it, 0]) == int(rows.min()) and int(r0i[it, 1]) == int(rows.max())
            if w2 is not None:
                assert (int(w2[it, 0]) - int(w2_plain[it, 0])) % 64 == 0 and w2[it, 0] >= w2_plain[it, 0]
                assert w2[it, 0] + w2[it, 1] == w2_plain[it, 0] + w2_plain[it, 1]
    if cached:
        skipped = aw.skipped_cache_rows(c)
        seen = np.zeros(c.kv0.shape[0], dtype=bool)
        for m in aw.segment_masks(b.segments, cached, T, to_cache) + aw.segment_masks(b.last_segments, cached, T,
                                                                                      to_cache):
            if m is not None:
                seen[(m[m >= (1 << 32)] - (1 << 32))] = True
        assert not seen[skipped].any()
        if c.W <= 65:
            assert len(skipped) >= 64          # whole tiles of the 200-row prefix fall out of every window


@pytest.mark.parametrize("args", ARGS, ids=IDS)
def test_layout_reference_matches_oracle_and_full_pass(args):
    """The windowed fp64 reference in the kernel's layout (kv0, range 2, the poisoned cache) == the
    windowed full packed pass on the same rows, and == TorchOps(float32).attention over the
    windowed segments."""
    c = aw.wcase(*args)
    kv0 = aw.poisoned_cache(c) if c.kv0 is not None else None
    r, queried, _, _ = aw.run(c.qkv, c.b.segments, c.nh, c.nkv, c.hd, kv0=kv0, scale=c.scale)
    assert bool(queried.all()) and bool(torch.isfinite(r).all())
    assert float(ar.row_err(r, c.ref).max()) < 1e-12
    o = TorchOps(torch.float32).attention(c.qkv.float(), c.b.segments, c.nh, c.nkv, c.hd,
                                          kv0=None if kv0 is None else torch.nan_to_num(kv0.float()), scale=c.scale)
    assert float(ar.row_err(o, r).max()) < 1e-5


@pytest.mark.parametrize("args", ARGS, ids=IDS)
def test_bound_separates_rounding_from_one_key(args):
    """min_single_key_effect >= 4 tau with tau = 8 max row_err(emulated_fp16, ref64), both from the
    windowed references (attention_rows' factors)."""
    c = aw.wcase(*args)
    assert c.min_effect >= ar.SEPARATION * c.tau, (c.min_effect, c.tau)


_MUT = [(cid, a) for cid, a in CASES if "-full-" in cid or "decode" in cid]


@pytest.mark.parametrize("args", [a for _, a in _MUT], ids=[c for c, _ in _MUT])
@pytest.mark.parametrize("ranges", [(0,), (1, 2)], ids=["range0", "range12"])
@pytest.mark.parametrize("delta", [1, -1], ids=["W+1", "W-1"])
def test_bound_catches_an_off_by_one_window(args, ranges, delta):
    """The emulated kernel with the lower bound off by one (W + 1 keys: the rule of transformers
    <= 4.35; W - 1 keys: the oldest visible key dropped), in range 0 or in ranges 1 / 2, exceeds tau
    on every (row, head) it touches."""
    c = aw.wcase(*args)
    m, touched = c.mutated(delta, ranges)
    # the rows the mutation must touch, from the positions alone: the key that W + 1 adds (position
    # i - W) or that W - 1 drops (i - W + 1; a row keeps its own key) lies in the named ranges
    full = c.full
    lp = np.zeros(full.num_tokens, dtype=np.int64)
    later = np.zeros(full.num_tokens, dtype=bool)      # bidirectional prefix rows: later keys stay visible
    for sg in full.segments:
        lp[sg.q_start:sg.q_start + sg.q_len] = sg.r0_len
        if not sg.r1_len and not sg.r0_causal:
            later[sg.q_start:sg.q_start + sg.q_len - 1] = True
    rows = c.rows.numpy()
    j = full.positions[rows].astype(np.int64) - c.W + (0 if delta > 0 else 1)
    valid = (j >= 0) & ((c.W + delta >= 1) | later[rows])      # (a row left without any key keeps W)
    expect = valid & ((j < lp[rows]) if ranges == (0,) else (j >= lp[rows]))
    assert np.array_equal(touched.numpy(), expect)
    if 1 < c.W <= 100 and c.kind == "full":
        assert expect.any()                    # (the 130-token suffix and every prefix outgrow these windows)
    if not expect.any():
        return
    err = ar.row_err(m[touched], c.ref[touched])
    assert float(err.min()) > c.tau, (float(err.min()), c.tau)


def test_generation_with_suffix_reuse_under_a_window(tmp_path):
    """num_gen_token=4 with W smaller than the prompts: suffix K/V reuse (range 2 under the window)
    == --suffix_kv_cache false == no cache at all, to the 1e-5 of the CPU generation tests; the
    reused steps computed only new tokens, and the window changes the scores."""
    from flexible_llm_sharding_amd.api import generation_loop
    from flexible_llm_sharding_amd.parallel.comm import Comm
    cfg = preset("tiny", sliding_window=24)
    path = str(tmp_path / "m")
    write_synthetic_checkpoint(cfg, path, seed=3, std=0.05)
    write_synthetic_tokenizer(path, cfg.vocab_size)
    tok = load_tokenizer(path)
    prompts = synthetic_prompts(4, 40, 3, 30, cfg.vocab_size, seed=21, vary=True)
    src = HostStore.from_model_path(cfg, path, pinned=False)
    args = argparse.Namespace(num_gen_token=4, data_parallel=False, num_batch=1)
    plain = ShardedRunner(cfg, src, "cpu", tok, sliding_window_mode="apply")
    s0, u0 = generation_loop(args, plain, Comm(), tok, prompts)
    for sfx in (False, True):
        r = ShardedRunner(cfg, src, "cpu", tok, prefix_kv_cache=True, suffix_kv_cache=sfx,
                          sliding_window_mode="apply")
        s1, u1 = generation_loop(args, r, Comm(), tok, prompts)
        assert u0 == u1
        for a, b in zip(s0, s1):
            assert a.shape == b.shape
            assert np.abs(a.astype(np.float32) - b.astype(np.float32)).max() < 1e-5
        assert r.prefix_cache.hits == 3 and r.stats["prefix_cached"] == 1.0
        assert (r.stats["suffix_tokens_reused"] > 0) == sfx
    nowin = preset_without_window(cfg)
    s2, _ = generation_loop(args, ShardedRunner(nowin, src, "cpu", tok), Comm(), tok, prompts)
    assert max(float(np.abs(a.astype(np.float32) - b.astype(np.float32)).max()) for a, b in zip(s0, s2)) > 1e-4


def test_graph_metadata_carries_the_window():
    """The bucketed graph metadata (runtime/graphs.py) pads the window arrays with the batch's."""
    from flexible_llm_sharding_amd.runtime.batch import pack_prompts
    from flexible_llm_sharding_amd.runtime.graphs import bucket_key, padded_meta
    tps = ar._tps(aw.PROMPTS)
    b = pack_prompts(tps, [0, 1, 2], window=100)
    key = bucket_key(b)
    m = padded_meta(b, key)
    assert m["r0_lo"].shape == m["seg_lo"].shape and m["r0_item"].shape == (m["work"].shape[0], 2)
    assert m["r0_item_last"].shape == (m["work_last"].shape[0], 2)
    assert np.array_equal(m["r0_lo"][:b.num_tokens], b.r0_lo)
    plain = pack_prompts(tps, [0, 1, 2])
    assert bucket_key(plain) != key and "r0_lo" not in padded_meta(plain, bucket_key(plain))
