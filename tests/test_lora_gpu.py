"""LoRA adapters on an MI355X: ``fls_lora_merge`` equals the host definition (lora.merge_reference) in
every bit, in place, with no byte written outside the weight; and a run with an adapter — streamed,
host-cached, resident, through the sub-layer piece pool, on quantised bases, generating through decode
graphs — equals the same run on the merged twin checkpoint in every bit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lora_ref as lr  # noqa: E402

from flexible_llm_sharding_amd import lora  # noqa: E402

HAS_GPU = torch.cuda.is_available()
gpu = pytest.mark.gpu
needs_gpu = pytest.mark.skipif(not HAS_GPU, reason="needs an MI355X")
DEV = torch.device("cuda", 0)
CANARY = 64
INVALID = 1                                   # hipErrorInvalidValue
_REFS = {}


def _case(rows, cols, r):
    """The data of one kernel case and its reference, computed once for every base offset."""
    key = (rows, cols, r)
    if key not in _REFS:
        w, A, Bs, facts = lr.kernel_case(rows, cols, r, seed=rows * 100003 + cols * 101 + r)
        want = lora.merge_reference(w, A[:r], Bs[:, :r], None)
        _REFS[key] = (w, A, Bs, facts, want)
    return _REFS[key]


def _run_kernel(w: np.ndarray, A: np.ndarray, Bs: np.ndarray, r: int, base_off: int, call=None):
    """The kernel in place on a weight at ``base_off`` bytes past a 256-byte aligned address, between
    two 0xA5 canaries.  Returns (fp16 result as uint16 bits, canaries intact, return code)."""
    from flexible_llm_sharding_amd import _native
    k = _native.kernels()
    rows, cols = w.shape
    n = 2 * rows * cols
    buf = torch.full((512 + base_off + n + CANARY,), 0xA5, dtype=torch.uint8, device=DEV)
    start = (-buf.data_ptr()) % 256 + 256 + base_off
    assert (buf.data_ptr() + start - base_off) % 256 == 0
    buf[start:start + n].copy_(torch.from_numpy(w.view(np.uint8).reshape(-1).copy()).to(DEV))
    a, b = torch.from_numpy(A).to(DEV), torch.from_numpy(Bs).to(DEV)
    st = torch.cuda.current_stream(DEV).cuda_stream
    if call is None:
        rc = k.fls_lora_merge(buf.data_ptr() + start, rows, cols, a.data_ptr(), b.data_ptr(), r, st)
    else:
        rc = call(k, buf.data_ptr() + start, a.data_ptr(), b.data_ptr(), st)
    torch.cuda.synchronize()
    back = buf.cpu()
    ok = bool((back[:start] == 0xA5).all()) and bool((back[start + n:] == 0xA5).all())
    return back[start:start + n].numpy().view(np.uint16).reshape(rows, cols).copy(), ok, rc


@gpu
@needs_gpu
@pytest.mark.parametrize("base_off", lr.BASE_OFFSETS)
def test_lora_merge_equals_reference(base_off):
    cases = lr.kernel_cases()
    assert {(a, b) for a, b, _ in cases} == {(a, b) for a in lr.ROWS for b in lr.COLS + lr.COLS_NARROW}
    assert {r for _, _, r in cases} == set(lr.RANKS)
    for rows, cols, r in cases:
        w, A, Bs, facts, want = _case(rows, cols, r)
        got, intact, rc = _run_kernel(w, A, Bs, r, base_off)
        assert rc == 0 and intact, (rows, cols, r, rc, "canary overwritten" if not intact else "")
        assert np.array_equal(got, want.view(np.uint16)), (rows, cols, r, int((got != want.view(np.uint16)).sum()))
        for o, i, bits in facts:                                  # the literal answers, whatever the reference says
            assert got[o, i] == bits, (rows, cols, r, o, i, hex(got[o, i]))
        if rows >= 31 and cols >= 7:
            assert got[1, 1] & 0x7FFF == 0x7C00                   # overflow to inf
            assert ((got[3] & 0x7C00) == 0).any()                 # fp16 subnormal results
        if (rows, cols) in ((130, 1032), (33, 20)):
            again, intact, _ = _run_kernel(w, A, Bs, r, base_off)
            assert intact and np.array_equal(again, got)
            # a zero B returns the weights bit for bit (but -0, which the chain's +0 products turn
            # into +0 or keep, as the reference says)
            zero, intact, _ = _run_kernel(w, A, np.zeros_like(Bs), r, base_off)
            keep = w.view(np.uint16) != 0x8000
            assert intact and np.array_equal(zero[keep], w.view(np.uint16)[keep])
            assert np.array_equal(zero, lora.merge_reference(w, A[:r], np.zeros_like(Bs[:, :r]), None).view(np.uint16))


@gpu
@needs_gpu
def test_lora_merge_refusals():
    w, A, Bs, _, _ = _case(33, 40, 5)
    orig = w.view(np.uint16)
    bad = [lambda k, W, a, b, st: k.fls_lora_merge(None, 33, 40, a, b, 5, st),
           lambda k, W, a, b, st: k.fls_lora_merge(W, 33, 40, None, b, 5, st),
           lambda k, W, a, b, st: k.fls_lora_merge(W, 33, 40, a, None, 5, st),
           lambda k, W, a, b, st: k.fls_lora_merge(W, 0, 40, a, b, 5, st),
           lambda k, W, a, b, st: k.fls_lora_merge(W, -1, 40, a, b, 5, st),
           lambda k, W, a, b, st: k.fls_lora_merge(W, 33, 0, a, b, 5, st),
           lambda k, W, a, b, st: k.fls_lora_merge(W, 33, 40, a, b, 0, st),
           lambda k, W, a, b, st: k.fls_lora_merge(W, 33, 40, a, b, 257, st),
           lambda k, W, a, b, st: k.fls_lora_merge(W, 33, 40, a, b, -4, st)]
    for call in bad:
        got, intact, rc = _run_kernel(w, A, Bs, 5, 0, call)
        assert rc == INVALID and intact and np.array_equal(got, orig)
    from flexible_llm_sharding_amd.ops import get_ops
    ops = get_ops(DEV)
    wt = torch.from_numpy(w.copy()).to(DEV)
    a, b = torch.from_numpy(A).to(DEV), torch.from_numpy(Bs).to(DEV)
    with pytest.raises(ValueError):
        ops.lora_merge(wt, a[:5], b, 5)                           # A not padded to R
    with pytest.raises(ValueError):
        ops.lora_merge(wt, a, b, 300)
    with pytest.raises(TypeError):
        ops.lora_merge(wt.float(), a, b, 5)
    torch.cuda.synchronize()
    assert np.array_equal(wt.cpu().numpy().view(np.uint16), orig)


# ---------------------------------------------------------------------- engine
PLAN_KEYS = ("token_budget", "mlp_chunk", "attn_rows", "qkv_chunk")
CAP_GB = 40
_SETUPS = {}


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """Per (preset, quantize), built once: config, base / adapter / twin directories, the loaded
    adapter, tokenizer, prompts and a cache of the twin's scores."""
    root = tmp_path_factory.mktemp("lora_gpu")

    def get(name, quantize=None):
        if (name, quantize) not in _SETUPS:
            from flexible_llm_sharding_amd.utils.tokenizer import load_tokenizer
            cfg, base = lr.make_base(root, name, quantize)
            ad, adapter = lr.make_adapter(root, cfg, name)
            twin = lr.make_twin(root, name, base, adapter, quantize)
            _SETUPS[(name, quantize)] = (cfg, base, ad, adapter, twin, load_tokenizer(base), lr.prompts_for(cfg, 4), {})
        return _SETUPS[(name, quantize)]
    return get


def _twin_scores(s, lnps, **kw):
    """The twin's scores (and memory plan) through the ordinary FileLayerSource, once per (lnps, cap)."""
    from flexible_llm_sharding_amd.engine import ShardedRunner
    from flexible_llm_sharding_amd.runtime.stream import FileLayerSource
    cfg, base, ad, adapter, twin, tok, prompts, cache = s
    key = (lnps, tuple(sorted(kw.items())))
    if key not in cache:
        r = ShardedRunner(cfg, FileLayerSource(cfg, twin), DEV, tok, layer_num_per_shard=lnps, **kw)
        out = r(prompts)
        cache[key] = (out, dict(r.vram_plan) if r.vram_plan else None)
        r.close()
    return cache[key]


def _source(mode, cfg, base, adapter):
    from flexible_llm_sharding_amd.runtime.stream import FileLayerSource
    from flexible_llm_sharding_amd.runtime.weights import CompactHostStore, HostStore
    files = FileLayerSource(cfg, base, chunk_mb=1, n_chunks=2)
    quantised = files.fp8_tensors() or files.int4_tensors()
    if quantised and mode in ("host", "piece_pool"):
        return CompactHostStore(files)                            # merges on every landing
    if mode == "host":                                            # what api.build_source does: merge, then fold
        st = HostStore.from_source(files)
        files.close()
        return st.merge_lora(adapter, DEV).fold_norms(DEV)
    return files                                                  # (the piece pool streams the pieces)


CONFIGS = ([("tiny", None, m, l) for m, l in (("stream", 1), ("stream", 3), ("host", 1), ("resident", 3),
                                              ("piece_pool", 1))]
           + [(n, None, m, 1) for n in ("tiny-qwen2", "tiny-phi3", "tiny-mixtral") for m in ("stream", "piece_pool")]
           + [("tiny", q, m, 1) for q in ("int4", "fp8") for m in ("stream", "host", "piece_pool")]
           + [("tiny", "bf16", m, 1) for m in ("stream", "host")])       # (cast to fp16 in HBM, then merged)


@gpu
@needs_gpu
@pytest.mark.parametrize("name,quantize,mode,lnps", CONFIGS, ids=["-".join(map(str, c)) for c in CONFIGS])
def test_engine_lora_bitwise_equals_twin(setup, name, quantize, mode, lnps):
    from flexible_llm_sharding_amd.engine import ShardedRunner
    from flexible_llm_sharding_amd.runtime.prefetch import PiecePoolPrefetcher
    s = setup(name, quantize)
    cfg, base, ad, adapter, twin, tok, prompts, _ = s
    cap = {"max_vram_gb": CAP_GB} if mode == "piece_pool" else {}
    kw = dict(cap, resident=True) if mode == "resident" else cap
    want, want_plan = _twin_scores(s, lnps, **cap)                # (a capped run's twin runs under the same cap)
    src = _source(mode, cfg, base, adapter)
    at_build = getattr(src, "lora_merged", None) is not None
    r = ShardedRunner(cfg, src, DEV, tok, layer_num_per_shard=lnps, lora=adapter, **kw)
    assert r.ctx.fused_norm                                       # merge first, then the norm fold, on every path
    per_pass = adapter.n_tensors // 2
    n0 = adapter.merge_launches
    first = r(prompts)
    second = r(prompts)                                           # slot rotation: a merge into a reused slot
    torch.cuda.synchronize()
    launches = adapter.merge_launches - n0
    plan = dict(r.vram_plan) if r.vram_plan else None
    staged = r.lora_staging.device_bytes() if r.lora_staging is not None else 0
    if mode == "piece_pool":
        assert isinstance(r.prefetcher, PiecePoolPrefetcher)
    r.close()
    assert lr.same_arrays(want, first) and lr.same_arrays(want, second)
    if at_build:
        assert launches == 0 and staged == 0                      # merged once at build: passes cost nothing
    elif mode == "resident":
        assert launches == per_pass and staged == adapter.staging_bytes()
    else:
        # (three rotating slots: the second call's first layers may already have landed)
        assert 2 * per_pass <= launches <= 3 * per_pass and staged == adapter.staging_bytes()
    if mode == "piece_pool":
        # the adapter adds its staging buffer (allocated before the plan measures the device) and
        # nothing else: the capped plan is the twin's, chunk for chunk
        assert plan is not None and want_plan is not None
        assert {k: plan[k] for k in PLAN_KEYS} == {k: want_plan[k] for k in PLAN_KEYS}
    assert r.lora_staging is None                                 # the runner's close released its staging


@gpu
@needs_gpu
@pytest.mark.parametrize("mode", ["piece_pool", "stream"])
def test_lora_device_memory_is_the_staging_buffer(setup, monkeypatch, mode):
    """Every byte of device memory comes from a raw allocation (``hostmem.alloc_device``: weight
    slots, staging) or from the caching allocator.  A run with the adapter makes the twin run's raw
    allocations plus exactly one more, of ``staging_bytes()``, made before any weight slot exists (so
    before a capped plan measures the device), and merging a layer takes nothing from the caching
    allocator.  (The allocator's peak over a whole run is printed, not compared: it differs by a
    megabyte between two runs of the same twin.)"""
    from flexible_llm_sharding_amd.engine import ShardedRunner
    from flexible_llm_sharding_amd.runtime import hostmem
    from flexible_llm_sharding_amd.runtime.stream import FileLayerSource
    cfg, base, ad, adapter, twin, tok, prompts, _ = setup("tiny")
    real, raw = hostmem.alloc_device, []

    def recording(nbytes, device):
        raw.append(int(nbytes))
        return real(nbytes, device)
    monkeypatch.setattr(hostmem, "alloc_device", recording)
    cap = {"max_vram_gb": CAP_GB} if mode == "piece_pool" else {}
    seen = {}
    for tag, path, a in (("warm", twin, None), ("twin", twin, None), ("lora", base, adapter)):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(DEV)
        del raw[:]
        before = torch.cuda.memory_allocated(DEV)
        r = ShardedRunner(cfg, FileLayerSource(cfg, path, chunk_mb=1, n_chunks=2), DEV, tok, layer_num_per_shard=1,
                          lora=a, **cap)
        out = [r(prompts), r(prompts)]
        torch.cuda.synchronize()
        staged = r.lora_staging.device_bytes() if r.lora_staging is not None else 0
        plan = dict(r.vram_plan) if r.vram_plan else None
        r.close()
        seen[tag] = (list(raw), torch.cuda.max_memory_allocated(DEV) - before, staged, plan, out)
    (raw_t, peak_t, _, plan_t, out_t), (raw_l, peak_l, staged, plan_l, out_l) = seen["twin"], seen["lora"]
    assert lr.same_arrays(out_t, out_l)
    assert adapter.staging_bytes() > 0 and staged == adapter.staging_bytes()
    assert raw_l[0] == adapter.staging_bytes() and sorted(raw_l[1:]) == sorted(raw_t), (raw_l, raw_t)
    print("allocator peak: twin", peak_t, "lora", peak_l)
    # a layer's merges alone, nothing else running: no allocation from the caching allocator
    name = next(n for n in cfg.layer_names() if adapter.targets(n))
    src = FileLayerSource(cfg, base)
    host = torch.empty(src.nbytes(name), dtype=torch.uint8)
    src.read_into(name, host)
    src.close()
    image = host.to(DEV)
    views = src.layout(name).views(image, torch.float16)
    staging = adapter.new_staging(DEV)
    from flexible_llm_sharding_amd.ops import get_ops
    ops = get_ops(DEV)
    torch.cuda.synchronize()
    count = lambda: torch.cuda.memory_stats(DEV)["allocation.all.allocated"]     # noqa: E731
    n0 = count()
    assert adapter.merge_views(ops, name, views, staging) == len(adapter.targets(name))
    torch.cuda.synchronize()
    assert count() == n0
    staging.release()
    if mode == "piece_pool":
        assert {k: plan_l[k] for k in PLAN_KEYS} == {k: plan_t[k] for k in PLAN_KEYS}
        # the planner's measured context grows by the buffer (hipMalloc rounds it up to its granularity)
        grow = plan_l["estimated_peak_bytes"] - plan_t["estimated_peak_bytes"]
        print("estimated peak: twin", plan_t["estimated_peak_bytes"], "lora", plan_l["estimated_peak_bytes"], "grow", grow)


@gpu
@needs_gpu
def test_write_twin_on_the_gpu_equals_the_numpy_twin(setup, tmp_path):
    """``prepare_weights.py --merge_lora`` with a GPU present: ``write_twin`` through ``ops_merge``
    (H2D, ``fls_lora_merge``, back) writes the files of the numpy twin byte for byte."""
    cfg, base, ad, adapter, twin, tok, prompts, _ = setup("tiny")
    out = str(tmp_path / "gpu_twin")
    lora.write_twin(base, adapter, out, merge=lora.ops_merge(DEV))
    names = sorted(os.listdir(twin))
    assert sorted(os.listdir(out)) == names
    for n in names:
        assert open(os.path.join(out, n), "rb").read() == open(os.path.join(twin, n), "rb").read(), n


@gpu
@needs_gpu
def test_engine_lora_differs_from_base(setup):
    from flexible_llm_sharding_amd.engine import ShardedRunner
    from flexible_llm_sharding_amd.runtime.stream import FileLayerSource
    s = setup("tiny")
    cfg, base, ad, adapter, twin, tok, prompts, _ = s
    r = ShardedRunner(cfg, FileLayerSource(cfg, base), DEV, tok)
    plain = r(prompts)
    r.close()
    assert not lr.same_arrays(_twin_scores(s, 1)[0], plain)


@gpu
@needs_gpu
@pytest.mark.parametrize("lookup", [0, 4])
def test_generation_lora_bitwise(setup, lookup):
    """num_gen_token = 4, resident weights, decode graphs, with and without prompt-lookup drafts:
    tokens and every step's scores equal the twin's."""
    import lookup_ref as lk
    from flexible_llm_sharding_amd.runtime.stream import FileLayerSource
    cfg, base, ad, adapter, twin, tok, prompts, _ = setup("tiny")
    a = lk.generate((cfg, tok, prompts, FileLayerSource(cfg, base)), DEV, lookup=lookup, num_gen=4, lora=adapter)
    b = lk.generate((cfg, tok, prompts, FileLayerSource(cfg, twin)), DEV, lookup=lookup, num_gen=4)
    assert a.updated == b.updated and lr.same_arrays(list(a.scores), list(b.scores))
    assert all(np.array_equal(u, v) for u, v in zip(a.tokens, b.tokens))
    assert [c["graph"] for c in a.calls] == [c["graph"] for c in b.calls] and a.calls[-1]["graph"] >= 1
    assert a.stats == b.stats


@gpu
@needs_gpu
@pytest.mark.parametrize("streaming", [False, True])
def test_dp_allgather_lora_bitwise(setup, streaming):
    """The data-parallel weight path on RCCL (a one-rank ``nccl`` group): every layer is H2D'd as a
    byte slice, completed in HBM by the all-gather and merged behind it on the copy stream — from
    pinned slices (which cannot be merged ahead: a rank holds 1/G of a layer) and streamed from the
    layer files.  The run equals the twin's through the same path.  (Two ranks: the gloo test of
    test_lora_cpu.py.)"""
    import socket

    import torch.distributed as dist
    from flexible_llm_sharding_amd.engine import ShardedRunner
    from flexible_llm_sharding_amd.parallel.comm import Comm
    from flexible_llm_sharding_amd.parallel.data_parallel import AllGatherPrefetcher, SlicedHostStore
    from flexible_llm_sharding_amd.parallel.planner import make_plan
    from flexible_llm_sharding_amd.runtime.stream import FileLayerSource
    cfg, base, ad, adapter, twin, tok, prompts, _ = setup("tiny")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    store = dist.TCPStore("127.0.0.1", port, 1, True)
    dist.init_process_group("nccl", store=store, rank=0, world_size=1, device_id=DEV)
    try:
        comm = Comm(0, 1, DEV, "nccl")
        names = cfg.layer_names()
        shards = [sh for sh in make_plan(len(names), 2, 1, 0, True).my_shards if len(sh)]
        outs = {}
        n0 = adapter.merge_launches
        for tag, path, a in (("twin", twin, None), ("lora", base, adapter)):
            files = FileLayerSource(cfg, path)
            src = files if streaming else SlicedHostStore.from_source(files, 0, 1)
            pf = AllGatherPrefetcher(src, names, shards, DEV, comm)
            r = ShardedRunner(cfg, src, DEV, tok, layer_num_per_shard=2, storage_location="cpu", token_budget=200,
                              comm=comm, data_parallel=True, prefetcher=pf, lora=a)
            outs[tag] = [r(prompts), r(prompts)]              # second call: slots recycled behind RCCL writes
            r.close()
        assert lr.same_arrays(outs["twin"][0], outs["lora"][0]) and lr.same_arrays(outs["twin"][0], outs["lora"][1])
        assert adapter.merge_launches - n0 >= 2 * (adapter.n_tensors // 2)
    finally:
        dist.destroy_process_group()
