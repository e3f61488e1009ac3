"""Sliding-window attention on an MI355X: every windowed kernel path against the windowed fp64
reference per (row, head) (tests/attention_window.py; the CPU side of the argument is
tests/test_sliding_window_cpu.py), and the engine against the CPU backend.

Every launch asserts what test_attention_rows_gpu.py asserts: (1) row_err(y, ref64) <= tau on every
queried (row, head), y finite there; (2) the in-place form is bitwise the out-of-place result and
leaves the K and V columns alone; (3) unqueried rows keep the sentinel.  Wherever a K/V cache is
read, its rows in 64-key tiles that lie wholly before every lower bound of every work item hold NaN:
a kernel that walked and masked those tiles instead of skipping them would return NaN (0 x NaN in
P.V).

Measured on an MI355X when these tests were added, W > 1 (tau from the CPU; W = 1 has tau = 0, one
key, and the kernels return that key's V exactly): largest row_err 3.9e-4 (hd 128), 4.7e-4 (hd 64,
128-row items), 4.0e-4 (hd 96) for the full, kv0 and range-2 forms and 4.0e-4 for the decode step on
attn_decode and the one-wave-per-head attn_fwd, split or not, against tau = 2.5e-3 .. 3.1e-3."""
import argparse
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import attention_rows as ar  # noqa: E402
import attention_window as aw  # noqa: E402
from flexible_llm_sharding_amd import _native  # noqa: E402
from flexible_llm_sharding_amd.config import preset  # noqa: E402
from flexible_llm_sharding_amd.engine import ShardedRunner  # noqa: E402
from flexible_llm_sharding_amd.ops.hip_backend import HipOps  # noqa: E402
from flexible_llm_sharding_amd.runtime.weights import HostStore  # noqa: E402
from flexible_llm_sharding_amd.utils.synthetic import synthetic_prompts, write_synthetic_checkpoint  # noqa: E402
from flexible_llm_sharding_amd.utils.tokenizer import (TokenizedPrompt, load_tokenizer,  # noqa: E402
                                                       write_synthetic_tokenizer)

DEV = torch.device("cuda", 0)
SENTINEL = 0x5A5A        # fp16 bit pattern (207.25) no attention output of these inputs can take


@pytest.fixture(scope="module")
def ops():
    o = HipOps()
    assert _native.loaded_libraries().get("k"), "libfls_kernels.so not loaded"
    return o


def _bits(x):
    return x.contiguous().view(torch.int16)


def _check(ops, c, work, r0_item, q_block, ref, queried, qkv=None, work2=None, kv0=None, tag=""):
    """One out-of-place and one in-place windowed launch; assertions 1-3; -> the output (CPU)."""
    m = c.b.device_tensors(DEV)
    qkv = c.qkv if qkv is None else qkv
    T, qs = qkv.shape[0], c.nh * c.hd
    kw = {"seg_lo": m["seg_lo"], "scale": c.scale, "q_block": q_block, "r0_lo": m["r0_lo"], "r0_item": r0_item}
    if kv0 is not None:
        kw["kv0"] = kv0.to(DEV)
    if work2 is not None:
        kw.update(work2=work2, r2win=m["r2win"])
    q = qkv.to(DEV)
    out = torch.full((T, qs), SENTINEL, dtype=torch.int16, device=DEV).view(torch.float16)
    y = ops.attention(q, work, c.nh, c.nkv, c.hd, out=out, **kw)
    inplace = q.clone()
    ops.attention(inplace, work, c.nh, c.nkv, c.hd, out=inplace[:, :qs], **kw)
    torch.cuda.synchronize()
    y, inplace = y.cpu(), inplace.cpu()
    assert bool(torch.isfinite(y[queried]).all()), tag
    err = float(ar.row_err(y[queried], ref[queried]).max())
    print(f"WROWS {tag} W={c.W} hd={c.hd} group={c.nh // c.nkv} q_block={q_block} tau={c.tau:.3e} err={err:.3e}")
    assert err <= c.tau, (tag, err, c.tau)
    assert torch.equal(_bits(inplace[queried, :qs]), _bits(y[queried]))
    assert torch.equal(_bits(inplace[:, qs:]), _bits(qkv[:, qs:]))
    assert bool((_bits(y[~queried]) == torch.tensor(SENTINEL, dtype=torch.int16)).all())
    assert torch.equal(_bits(inplace[~queried, :qs]), _bits(qkv[~queried, :qs]))
    return y


def _padded(work, r0_item):
    """Three padding items (q_len 0) behind the real ones."""
    return (torch.cat([work, torch.zeros(3, 8, dtype=torch.int32, device=DEV)]),
            torch.cat([r0_item, torch.zeros(3, 2, dtype=torch.int32, device=DEV)]))


def _hpbs(c):
    if c.hd == 96:
        return [0]
    return [0] + [h for h in (1, 2, 4) if (c.nh // c.nkv) % h == 0 and h <= (4 if c.q_block == 64 else 2)]


def _full_pass(ops, c, work, r0_item, ref, queried, qkv=None, kv0=None, tag=""):
    """The persistent-kernel switch on and off (a windowed pass takes attn_fwd either way: bitwise
    equal) x every heads-per-block value (bitwise equal)."""
    old_p, old_h = ops.k.fls_attention_set_persistent(1), ops.k.fls_attention_set_hpb(0)
    try:
        ys = []
        for pers in (1, 0):
            ops.k.fls_attention_set_persistent(pers)
            for hpb in _hpbs(c):
                ops.k.fls_attention_set_hpb(hpb)
                ys.append(_check(ops, c, work, r0_item, c.q_block, ref, queried, qkv=qkv, kv0=kv0,
                                 tag=f"{tag} pers={pers} hpb={hpb}"))
        for y in ys[1:]:
            assert torch.equal(_bits(y), _bits(ys[0]))
    finally:
        ops.k.fls_attention_set_persistent(old_p)
        ops.k.fls_attention_set_hpb(old_h)


def _poisoned(c):
    kv0 = aw.poisoned_cache(c)
    skipped = aw.skipped_cache_rows(c)
    assert bool(torch.isnan(kv0[torch.from_numpy(skipped).long()]).all())
    return kv0, skipped


def _pruned_inputs(c, kv0):
    """The pruned last layer: Q of the non-scored rows is unwritten memory (NaN here); expected
    values from the scored rows' own windowed segments == the full pass on those rows."""
    qs = c.nh * c.hd
    scored = torch.zeros(c.b.num_tokens, dtype=torch.bool)
    scored[torch.from_numpy(c.b.last_idx).long()] = True
    qkv = c.qkv.clone()
    qkv[~scored, :qs] = float("nan")
    ref, queried, _, _ = aw.run(qkv, c.b.last_segments, c.nh, c.nkv, c.hd, kv0=kv0, scale=c.scale)
    assert torch.equal(queried, scored) and bool(torch.isfinite(ref[scored]).all())
    assert float(ar.row_err(ref[scored], c.ref[scored]).max()) < 1e-12
    return qkv, ref, scored


_ALL = aw.cases()
_FULL = [(cid, a) for cid, a in _ALL if "-full-" in cid]
_KV0 = [(cid, a) for cid, a in _ALL if "-kv0-" in cid]
_REUSE = [(cid, a) for cid, a in _ALL if "-reuse-" in cid]
_DECODE = [(cid, a) for cid, a in _ALL if "-decode-" in cid]


@pytest.mark.parametrize("args", [a for _, a in _FULL], ids=[c for c, _ in _FULL])
def test_windowed_full_pass_rows(ops, args):
    """Full pass under a window (attn_fwd WIN; hd 64 / 96 / 128, 64- and 128-row items, both prefix
    modes, padding items), and its pruned last-layer form (work_last + r0_item_last)."""
    c = aw.wcase(*args)
    m = c.b.device_tensors(DEV)
    work, r0i = _padded(m["work"], m["r0_item"])
    allq = torch.ones(c.b.num_tokens, dtype=torch.bool)
    _full_pass(ops, c, work, r0i, c.ref, allq, tag="full")
    qkv, ref, scored = _pruned_inputs(c, None)
    assert 0 < int(scored.sum()) < c.b.num_tokens
    _full_pass(ops, c, m["work_last"], m["r0_item_last"], ref, scored, qkv=qkv, tag="pruned")


@pytest.mark.parametrize("args", [a for _, a in _KV0], ids=[c for c, _ in _KV0])
def test_windowed_prefix_from_cache_rows(ops, args):
    """Range 0 from a prefix K/V cache under a window; the tiles in front of every item's first
    visible tile hold NaN (skipped, never walked)."""
    c = aw.wcase(*args)
    kv0, skipped = _poisoned(c)
    assert len(skipped) >= (64 if c.W <= 65 else 0)
    m = c.b.device_tensors(DEV)
    work, r0i = _padded(m["work"], m["r0_item"])
    _full_pass(ops, c, work, r0i, c.ref, torch.ones(c.b.num_tokens, dtype=torch.bool), kv0=kv0, tag="kv0")
    qkv, ref, scored = _pruned_inputs(c, kv0)
    _full_pass(ops, c, m["work_last"], m["r0_item_last"], ref, scored, qkv=qkv, kv0=kv0, tag="kv0-pruned")


def _r2(ops, c, q_blocks, splits, tag):
    kv0, skipped = _poisoned(c)
    m = c.b.device_tensors(DEV)
    allq = torch.ones(c.b.num_tokens, dtype=torch.bool)
    qkv, ref, scored = _pruned_inputs(c, kv0)
    old = ops.k.fls_attention_set_split(1)
    try:
        for q_block in q_blocks:
            assert q_block != 32 or int(c.b.work[:, 1].max()) <= 32
            for split in splits:
                ops.k.fls_attention_set_split(split)
                _check(ops, c, m["work"], m["r0_item"], q_block, c.ref, allq, work2=m["work2"], kv0=kv0,
                       tag=f"{tag} split={split}")
                _check(ops, c, m["work_last"], m["r0_item_last"], q_block, ref, scored, qkv=qkv,
                       work2=m["work2_last"], kv0=kv0, tag=f"{tag}-pruned split={split}")
    finally:
        ops.k.fls_attention_set_split(old)
    return skipped


@pytest.mark.parametrize("args", [a for _, a in _REUSE], ids=[c for c, _ in _REUSE])
def test_windowed_suffix_rows_from_cache_rows(ops, args):
    """Range 0 + range 2 from the K/V cache under a window (attn_fwd R2 WIN; split-KV off / 2 / 3
    + attn_split_combine; hd 96 never splits), the cache's unwalked tiles NaN; work_last too."""
    c = aw.wcase(*args)
    _r2(ops, c, (c.q_block,), (1, 2, 3), "r2")


@pytest.mark.parametrize("args", [a for _, a in _DECODE], ids=[c for c, _ in _DECODE])
def test_windowed_decode_step_rows(ops, args):
    """A decode step (one new row per suffix after the kept ones): attn_decode WIN (q_block 8) and
    the one-wave-per-head attn_fwd R2 WIN (q_block 32), unsplit and split in 2 / 3."""
    c = aw.wcase(*args)
    assert c.b.num_tokens == c.b.n_scored == 6 and c.b.r2_q_block == 8
    skipped = _r2(ops, c, (8, 32), (1, 2, 3), "decode")
    if c.W <= 65:
        assert len(skipped) >= 128             # the 200-row prefix: at least its first two tiles


# --------------------------------------------------------------------------- engine
W_ENGINE = 40


@pytest.fixture(scope="module")
def windowed_model(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("windowed_model"))
    cfg = preset("tiny", model_type="mistral", architectures=["MistralForCausalLM"], rope_theta=1e6,
                 sliding_window=W_ENGINE)
    write_synthetic_checkpoint(cfg, d, seed=4, std=0.05)
    write_synthetic_tokenizer(d, cfg.vocab_size)
    return d, cfg, load_tokenizer(d)


def _tps(cfg, n=3, lp=100, ls=(20, 50)):
    g = np.random.default_rng(3)
    return [TokenizedPrompt(g.integers(3, cfg.vocab_size, lp).tolist(),
                            [g.integers(3, cfg.vocab_size, l).tolist() for l in ls], max(ls), [l - 1 for l in ls])
            for _ in range(n)]


@pytest.mark.parametrize("mode", ["bidirectional", "causal"])
def test_engine_windowed_scores_match_cpu_backend(windowed_model, mode):
    """sliding_window=40 on 100-token prefixes + (20, 50)-token suffixes: HIP scores == the CPU
    backend's (2e-3, the bound of tests/test_engine_gpu.py) with the weights resident, with the
    pruned last layer off, and through the grouped attention phase of --max_vram_gb (forced by its
    row limit: a cap itself limits the allocator of the whole test process)."""
    d, cfg, tok = windowed_model
    tps = _tps(cfg)
    src = HostStore.from_model_path(cfg, d)
    want = ShardedRunner(cfg, src, "cpu", tok, prefix_attention=mode, sliding_window_mode="apply").run_tokenized(tps)
    nowin = ShardedRunner(dataclasses.replace(cfg, sliding_window=None), src, "cpu", tok,
                          prefix_attention=mode).run_tokenized(tps)
    assert max(float(np.abs(a - b).max()) for a, b in zip(want, nowin)) > 2e-3    # the window matters here
    outs = {}
    for name, kw, rows in (("resident", {"resident": True}, 0), ("unpruned", {"prune_last_layer": False}, 0),
                           ("grouped", {}, 200)):
        r = ShardedRunner(cfg, src, "cuda:0", tok, layer_num_per_shard=2, prefix_attention=mode,
                          sliding_window_mode="apply", **kw)
        if rows:
            r.ctx.attn_rows = rows
        outs[name] = r.run_tokenized(tps)
        for o, w in zip(outs[name], want):
            assert o.dtype == np.float16 and np.isfinite(o.astype(np.float32)).all()
            assert np.abs(o.astype(np.float32) - w.astype(np.float32)).max() < 2e-3
        r.close()
    with pytest.raises(ValueError, match="sliding-window attention is not implemented"):
        r = ShardedRunner(cfg, src, "cuda:0", tok, layer_num_per_shard=2, prefix_attention=mode)
        try:
            r.run_tokenized(tps)
        finally:
            r.close()


def test_engine_windowed_generation_reuse_bitwise(windowed_model):
    """Three generated tokens under the window with decode graphs on: suffix K/V reuse (range 2,
    windowed attn_decode in a replayed graph) == the exact re-run (--suffix_kv_cache false) bit for
    bit, with tokens reused and a graph replayed."""
    from flexible_llm_sharding_amd.api import generation_loop
    from flexible_llm_sharding_amd.parallel.comm import Comm
    d, cfg, tok = windowed_model
    prompts = synthetic_prompts(4, 90, 3, 60, cfg.vocab_size, seed=11, vary=True)
    src = HostStore.from_model_path(cfg, d)
    args = argparse.Namespace(num_gen_token=3, data_parallel=False, num_batch=1)
    outs = {}
    for sfx in (False, True):
        r = ShardedRunner(cfg, src, "cuda:0", tok, layer_num_per_shard=1, prefix_kv_cache=True, suffix_kv_cache=sfx,
                          resident=True, sliding_window_mode="apply")
        assert all(r._call_window([tp]) == W_ENGINE for tp in r.tokenize(prompts))
        outs[sfx] = generation_loop(args, r, Comm(), tok, prompts)
        if sfx:
            assert r.stats["suffix_tokens_reused"] > 0
            assert r.stats.get("graph_replays", 0) >= 1
        r.close()
    (s0, u0), (s1, u1) = outs[False], outs[True]
    assert u0 == u1
    for a, b in zip(s0, s1):
        assert np.isfinite(a.astype(np.float32)).all()
        assert np.array_equal(a, b)
