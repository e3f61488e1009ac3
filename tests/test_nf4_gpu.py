"""bitsandbytes 4-bit (NF4 / FP4) checkpoints on an MI355X: ``fls_dequant_nf4`` equals the host
definition (nf4.dequantize) in every bit, in place, with no byte written outside the tensor's region;
a run on an NF4 checkpoint — streamed, pinned compact, resident, through the sub-layer piece pool,
generating through decode graphs, and with a LoRA adapter — equals the same run on its fp16 twin in
every bit while moving a quarter of the weight bytes and holding only the table arena besides."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nf4_ref as nr  # noqa: E402

from flexible_llm_sharding_amd import nf4  # noqa: E402

HAS_GPU = torch.cuda.is_available()
gpu = pytest.mark.gpu
needs_gpu = pytest.mark.skipif(not HAS_GPU, reason="needs an MI355X")
DEV = torch.device("cuda", 0)
CANARY = 64
NS = (64, 8128, 8192, 8256, 24896, 16448, 1048576)


@pytest.fixture(scope="module", autouse=True)
def _uncap_allocator():
    """``max_vram_gb`` bounds the caching allocator for the whole process: lift the bound after this
    module, so that the capped runs here do not starve the tests that follow."""
    yield
    if HAS_GPU:
        torch.cuda.set_per_process_memory_fraction(1.0)


def _run_kernel(ops, packed, absmax, n, block, code, tables, base_off, twice=False):
    """The kernel in place on a region at ``base_off`` bytes past a 256-byte aligned address, between
    two canaries, stale 0x5A below the landed bytes.  Returns (fp16 result, canaries intact); ``twice``
    lands and expands a second time in the same region."""
    es = absmax.element_size()
    host = torch.full((2 * n,), 0x5A, dtype=torch.uint8)
    nf4.land(host, packed, absmax.view(torch.uint8), n, block, es)
    assert (host[:nf4.landing_span(n, block, es)[0]] == 0x5A).all()
    buf = torch.full((512 + base_off + 2 * n + CANARY,), 0xA5, dtype=torch.uint8, device=DEV)
    start = (-buf.data_ptr()) % 256 + 256 + base_off             # (at least 256 >= CANARY bytes in front)
    assert (buf.data_ptr() + start - base_off) % 256 == 0
    region = buf[start:start + 2 * n]
    kind = nf4.ABSMAX_U8 if es == 1 else nf4.ABSMAX_F32
    outs = []
    for _ in range(2 if twice else 1):
        region.copy_(host.to(DEV))
        ops.dequant_nf4(region, n, block, kind, code, *tables)
        torch.cuda.synchronize()
        outs.append(buf.cpu())
    back = outs[-1]
    ok = bool((back[:start] == 0xA5).all()) and bool((back[start + 2 * n:] == 0xA5).all())
    if twice:
        ok = ok and torch.equal(outs[0], outs[1])
    return back[start:start + 2 * n].clone().view(torch.float16), ok


@gpu
@needs_gpu
@pytest.mark.parametrize("base_off", [0, 2, 6])
@pytest.mark.parametrize("kind", ["f32", "u8_b2_256", "u8_b2_3"])
@pytest.mark.parametrize("block", [64, 128, 4096])
def test_dequant_nf4_equals_host(block, kind, base_off):
    from flexible_llm_sharding_amd import _native
    from flexible_llm_sharding_amd.ops import get_ops
    ops, k = get_ops(DEV), _native.kernels()
    rng = np.random.default_rng(1000 * block + 10 * len(kind) + base_off)
    es = 4 if kind == "f32" else 1
    b2 = {"f32": 0, "u8_b2_256": 256, "u8_b2_3": 3}[kind]
    assert k.fls_dequant_nf4_tail() == nf4.TAIL
    sizes = [n for n in NS if n % block == 0]
    assert sizes and (block != 64 or sizes == list(NS))
    for n in sizes:
        assert k.fls_dequant_nf4_launches(n, block, es) == len(nf4.schedule(n, block, es))
        for mode, extreme in (("lanes", False), ("lanes", True), ("random", False)):
            nib = nr.lanes(n) if mode == "lanes" else rng.integers(0, 16, n).astype(np.uint8)
            packed = nr.t(nr.pack(nib))
            code = nr.t(np.array(nr.NF4, dtype=np.float32) if mode == "random" else nr.full_mantissa_code(rng))
            if es == 4:
                absmax, hk, dk = nr.t(nr.f32_absmax(n // block, rng, extreme)), {}, (None, None, 0, 0.0)
            else:
                a, code2, nested, off = nr.u8_absmax(n // block, b2, rng, extreme)
                absmax = nr.t(a)
                hk = dict(code2=nr.t(code2), nested_absmax=nr.t(nested), nested_block=b2, offset=off)
                dk = (nr.t(code2).to(DEV), nr.t(nested).to(DEV), b2, off)
            want = nf4.dequantize(packed, code, absmax, (n // 32, 32), block, **hk).reshape(-1)
            twice = mode == "random" and n in (8256, 24896, 8192)
            got, intact = _run_kernel(ops, packed, absmax, n, block, code.to(DEV), dk, base_off, twice)
            assert intact, (n, mode, "canary overwritten, or a second run differs")
            assert nr.same_bits(got, want), (n, mode, extreme)
    assert k.fls_dequant_nf4(None, 0, 64, 0, None, None, None, 0, 0.0, None) == 0


@gpu
@needs_gpu
def test_dequant_nf4_refusals():
    from flexible_llm_sharding_amd import _native
    from flexible_llm_sharding_amd.ops import get_ops
    ops, k = get_ops(DEV), _native.kernels()
    region = torch.zeros(2 * 128, dtype=torch.uint8, device=DEV)
    code = torch.tensor(nr.NF4, dtype=torch.float32, device=DEV)
    code2 = torch.zeros(256, dtype=torch.float32, device=DEV)
    nested = torch.ones(4, dtype=torch.float32, device=DEV)
    p, c, c2, nb = region.data_ptr(), code.data_ptr(), code2.data_ptr(), nested.data_ptr()
    assert k.fls_dequant_nf4(None, 128, 64, 0, c, None, None, 0, 0.0, None) != 0          # a null region
    assert k.fls_dequant_nf4(p, 128, 64, 0, None, None, None, 0, 0.0, None) != 0          # a null code book
    assert k.fls_dequant_nf4(p + 1, 64, 64, 0, c, None, None, 0, 0.0, None) != 0          # an odd region address
    assert k.fls_dequant_nf4(p, 96, 48, 0, c, None, None, 0, 0.0, None) != 0              # block % 32
    assert k.fls_dequant_nf4(p, 128, 0, 0, c, None, None, 0, 0.0, None) != 0
    assert k.fls_dequant_nf4(p, 96, 64, 0, c, None, None, 0, 0.0, None) != 0              # n % block
    assert k.fls_dequant_nf4(p, 128, 64, 2, c, c2, nb, 1, 0.0, None) != 0                 # an unknown absmax kind
    assert k.fls_dequant_nf4(p, 128, 64, -1, c, c2, nb, 1, 0.0, None) != 0
    assert k.fls_dequant_nf4(p, 128, 64, 1, c, None, nb, 1, 0.0, None) != 0               # U8 absmax without code2
    assert k.fls_dequant_nf4(p, 128, 64, 1, c, c2, None, 1, 0.0, None) != 0               # ... without nested absmax
    assert k.fls_dequant_nf4(p, 128, 64, 1, c, c2, nb, 0, 0.0, None) != 0                 # ... with nested block 0
    assert k.fls_dequant_nf4_launches(96, 64, 1) < 0 and k.fls_dequant_nf4_launches(64, 32, 2) < 0
    with pytest.raises(ValueError):
        ops.dequant_nf4(region, 96, 32, 0, code)                              # region is not 2 bytes per weight
    with pytest.raises(ValueError):
        ops.dequant_nf4(region, 128, 48, 0, code)
    with pytest.raises(ValueError):
        ops.dequant_nf4(region, 128, 64, 2, code)
    with pytest.raises(ValueError):
        ops.dequant_nf4(region, 128, 64, 1, code)                             # no nested tables
    with pytest.raises(ValueError):
        ops.dequant_nf4(region, 128, 64, 0, code.cpu())                       # a table on another device
    torch.cuda.synchronize()
    assert not region.any()


# ---------------------------------------------------------------------- engine
_PAIRS = {}
PLAN_KEYS = ("token_budget", "mlp_chunk", "attn_rows", "qkv_chunk")
CAP_GB = 40


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    """(cfg, nf4 dir, twin dir, tokenizer, prompts, the twin's scores per lnps) per (preset, kind), built once."""
    root = tmp_path_factory.mktemp("nf4_gpu")

    def get(name, dq=True):
        if (name, dq) not in _PAIRS:
            from flexible_llm_sharding_amd.utils.tokenizer import load_tokenizer
            cfg, q, twin = nr.make_pair(root, name, dq)
            _PAIRS[(name, dq)] = (cfg, q, twin, load_tokenizer(q), nr.prompts_for(cfg, 4), {})
        return _PAIRS[(name, dq)]
    return get


def _twin_scores(p, lnps, **kw):
    """The twin's scores (and memory plan) through the ordinary FileLayerSource, once per (lnps, cap)."""
    from flexible_llm_sharding_amd.engine import ShardedRunner
    from flexible_llm_sharding_amd.runtime.stream import FileLayerSource
    cfg, q, twin, tok, prompts, cache = p
    key = (lnps, tuple(sorted(kw.items())))
    if key not in cache:
        r = ShardedRunner(cfg, FileLayerSource(cfg, twin), DEV, tok, layer_num_per_shard=lnps, **kw)
        out = r(prompts)
        cache[key] = (out, dict(r.vram_plan) if r.vram_plan else None)
        r.close()
    return cache[key]


def _source(mode, cfg, q):
    from flexible_llm_sharding_amd.runtime.stream import FileLayerSource
    from flexible_llm_sharding_amd.runtime.weights import CompactHostStore
    if mode == "compact":
        return CompactHostStore(FileLayerSource(cfg, q))
    return FileLayerSource(cfg, q, chunk_mb=1, n_chunks=2, direct=mode == "stream_direct")


def _same(want, got) -> bool:
    return len(want) == len(got) and all(a.dtype == np.float16 and np.array_equal(w.view(np.uint16), a.view(np.uint16))
                                         for w, a in zip(want, got))


ENGINE = ([("tiny", dq, m, l) for dq in (True, False) for m, l in (("stream", 1), ("stream", 3), ("stream_direct", 1),
                                                                    ("compact", 1), ("resident", 3), ("piece_pool", 1))]
          + [("tiny-qwen2", True, m, 1) for m in ("stream", "compact", "piece_pool")])


@gpu
@needs_gpu
@pytest.mark.parametrize("name,dq,mode,lnps", ENGINE, ids=["-".join(map(str, c)) for c in ENGINE])
def test_engine_nf4_bitwise_equals_twin(pair, name, dq, mode, lnps):
    from flexible_llm_sharding_amd.engine import ShardedRunner
    from flexible_llm_sharding_amd.runtime.prefetch import PiecePoolPrefetcher
    p = pair(name, dq)
    cfg, q, twin, tok, prompts, _ = p
    cap = {"max_vram_gb": CAP_GB} if mode == "piece_pool" else {}
    kw = dict(cap, resident=True) if mode == "resident" else cap
    want, want_plan = _twin_scores(p, lnps, **cap)                # (a capped run's twin runs under the same cap)
    src = _source("compact" if mode == "piece_pool" and name != "tiny" else mode, cfg, q)
    r = ShardedRunner(cfg, src, DEV, tok, layer_num_per_shard=lnps, **kw)
    if mode == "piece_pool":
        assert isinstance(r.prefetcher, PiecePoolPrefetcher)
    first = r(prompts)
    second = r(prompts)                      # slot rotation, re-expansion into a reused slot
    plan = dict(r.vram_plan) if r.vram_plan else None
    files = src if hasattr(src, "nf4_tensors") else src.files
    arena = files.scale_arena_bytes()
    r.close()
    assert _same(want, first) and _same(want, second)
    if mode == "piece_pool":
        # the arena is allocated before the plan measures the device: the plan is the twin's, chunk for chunk
        assert plan is not None and want_plan is not None
        assert {k: plan[k] for k in PLAN_KEYS} == {k: want_plan[k] for k in PLAN_KEYS}
    assert files.nf4_tensors() == 7 * cfg.num_hidden_layers and files.int4_tensors() == 0
    # one code book; with double quantisation also one code2 and a few nested absmax values per tensor
    assert arena == 64 if not dq else 4 * (16 + 256) < arena <= 4 * (16 + 256) + 64 * files.nf4_tensors()


@gpu
@needs_gpu
def test_generation_nf4_bitwise(pair):
    """num_gen_token = 4, resident weights, decode graphs: tokens and every step's scores equal the twin's."""
    import topk_ref as tr
    from flexible_llm_sharding_amd.runtime.stream import FileLayerSource
    cfg, q, twin, tok, prompts, _ = pair("tiny")
    runs = {}
    for tag, path in (("nf4", q), ("twin", twin)):
        runs[tag] = tr.generate((cfg, tok, prompts, FileLayerSource(cfg, path)), DEV, num_gen=4)
    a, b = runs["nf4"], runs["twin"]
    assert a.updated == b.updated and len(a.scores) == len(b.scores)
    for x, y in zip(a.scores, b.scores):
        assert x.shape[1] == 4 and np.array_equal(x.view(np.uint16), y.view(np.uint16))
    for sa, sb in zip(a.tokens, b.tokens):
        assert all(np.array_equal(u, v) for u, v in zip(sa, sb))
    assert a.stats[-1].get("graph_replays", 0) >= 1


@gpu
@needs_gpu
@pytest.mark.parametrize("mode", ["stream", "compact", "piece_pool"])
def test_nf4_lora_bitwise_equals_twin(pair, tmp_path, mode):
    """--lora on the NF4 base (merged after the expansion, on every landing) equals --lora on its twin."""
    from flexible_llm_sharding_amd import lora
    from flexible_llm_sharding_amd.engine import ShardedRunner
    from flexible_llm_sharding_amd.runtime.stream import FileLayerSource
    cfg, q, twin, tok, prompts, _ = pair("tiny")
    ad = str(tmp_path / "adapter")
    lora.write_synthetic_adapter(cfg, ad, r=4, seed=1)
    adapter = lora.LoraAdapter.load(cfg, ad)
    cap = {"max_vram_gb": CAP_GB} if mode == "piece_pool" else {}
    outs = {}
    for tag, src, a in (("twin", FileLayerSource(cfg, twin), adapter), ("plain", FileLayerSource(cfg, q), None),
                        ("nf4", _source("stream" if mode == "piece_pool" else mode, cfg, q), adapter)):
        r = ShardedRunner(cfg, src, DEV, tok, layer_num_per_shard=1, lora=a, **cap)
        outs[tag] = [r(prompts), r(prompts)]
        r.close()
    assert _same(outs["twin"][0], outs["nf4"][0]) and _same(outs["twin"][1], outs["nf4"][1])
    assert not _same(outs["twin"][0], outs["plain"][0])


@gpu
@needs_gpu
@pytest.mark.parametrize("dq", [True, False])
def test_nf4_moves_a_quarter_of_the_bytes(pair, dq):
    from flexible_llm_sharding_amd.engine import ShardedRunner
    from flexible_llm_sharding_amd.runtime.stream import FileLayerSource
    from flexible_llm_sharding_amd.runtime.weights import CompactHostStore
    cfg, q, twin, tok, prompts, _ = pair("tiny", dq)
    es = 1 if dq else 4
    names = cfg.layer_names()
    src = FileLayerSource(cfg, q, chunk_mb=1, n_chunks=2)
    files = sum(src.plan(n).file_bytes for n in names)
    assert files == sum(nr.moved_bytes(q, n) for n in names)
    # (two slots: the engine then prefetches nothing of the next call, so one call is one pass)
    r = ShardedRunner(cfg, src, DEV, tok, layer_num_per_shard=1, n_slots=2)
    r(prompts)
    torch.cuda.synchronize()
    st = src.stats()
    # weight_h2d_bytes == weight_file_bytes: one pass reads and copies exactly the files' tensor bytes
    assert int(st["h2d_bytes"]) == files and src.read_bytes == files == int(st["read_bytes"])
    r.close()
    # ... and those are the packed bytes plus the absmax bytes (plus the tensors that are not 4-bit)
    tsrc = FileLayerSource(cfg, twin)
    for n in names:
        runs = src.plan(n).runs
        weights = sum(r_.numel for r_ in runs if r_.is_nf4)
        rest = sum(r_.file_nbytes for r_ in runs if not r_.is_nf4)
        assert 2 * weights + rest == tsrc.plan(n).file_bytes
        assert src.plan(n).file_bytes == weights // 2 + weights // 64 * es + rest
    store = CompactHostStore(FileLayerSource(cfg, q))
    assert files <= store.total_bytes < files + 16 * sum(len(store.plan(n).pieces()) for n in names)
    store.close()


@gpu
@needs_gpu
@pytest.mark.parametrize("mode", ["piece_pool", "stream"])
def test_nf4_device_memory_is_the_table_arena(pair, monkeypatch, mode):
    """Every byte of device memory comes from a raw allocation (``hostmem.alloc_device``: weight
    slots, the table arena) or from the caching allocator.  A run on the NF4 checkpoint makes the
    twin run's raw allocations plus exactly one more, of ``scale_arena_bytes()``, made before any
    weight slot exists (so before a capped plan measures the device); and an expansion takes nothing
    from the caching allocator."""
    from flexible_llm_sharding_amd.engine import ShardedRunner
    from flexible_llm_sharding_amd.ops import get_ops
    from flexible_llm_sharding_amd.runtime import hostmem
    from flexible_llm_sharding_amd.runtime.stream import FileLayerSource
    cfg, q, twin, tok, prompts, _ = pair("tiny")
    real, raw = hostmem.alloc_device, []

    def recording(nbytes, device):
        raw.append(int(nbytes))
        return real(nbytes, device)
    monkeypatch.setattr(hostmem, "alloc_device", recording)
    cap = {"max_vram_gb": CAP_GB} if mode == "piece_pool" else {}
    seen = {}
    for tag, path in (("warm", twin), ("twin", twin), ("nf4", q)):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        del raw[:]
        src = FileLayerSource(cfg, path, chunk_mb=1, n_chunks=2)
        r = ShardedRunner(cfg, src, DEV, tok, layer_num_per_shard=1, **cap)
        out = [r(prompts), r(prompts)]
        torch.cuda.synchronize()
        arena = src.scale_arena_bytes()
        plan = dict(r.vram_plan) if r.vram_plan else None
        r.close()
        seen[tag] = (list(raw), arena, plan, out)
    (raw_t, arena_t, plan_t, out_t), (raw_n, arena_n, plan_n, out_n) = seen["twin"], seen["nf4"]
    assert _same(out_t[0], out_n[0]) and _same(out_t[1], out_n[1])
    assert arena_t == 0 and arena_n > 0
    assert raw_n[0] == arena_n and sorted(raw_n[1:]) == sorted(raw_t), (raw_n, raw_t)
    if mode == "piece_pool":
        assert {k: plan_n[k] for k in PLAN_KEYS} == {k: plan_t[k] for k in PLAN_KEYS}
    # one tensor's expansion alone, nothing else running: no allocation from the caching allocator
    n, block = 24896, 64
    rng = np.random.default_rng(0)
    a, code2, nested, off = nr.u8_absmax(n // block, 256, rng, False)
    region = torch.zeros(2 * n, dtype=torch.uint8)
    nf4.land(region, nr.t(rng.integers(0, 256, n // 2).astype(np.uint8)), nr.t(a), n, block, 1)
    region, code = region.to(DEV), torch.tensor(nr.NF4, dtype=torch.float32, device=DEV)
    tables = (nr.t(code2).to(DEV), nr.t(nested).to(DEV), 256, off)
    ops = get_ops(DEV)
    torch.cuda.synchronize()
    count = lambda: torch.cuda.memory_stats(DEV)["allocation.all.allocated"]     # noqa: E731
    n0 = count()
    ops.dequant_nf4(region, n, block, nf4.ABSMAX_U8, code, *tables)
    torch.cuda.synchronize()
    assert count() == n0
