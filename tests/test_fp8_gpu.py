"""Weight-only FP8 (e4m3fn) checkpoints on an MI355X: ``fls_dequant_fp8`` equals the host definition
(fp8.dequantize) in every bit, in place, with no byte written outside the tensor's region; and a run
on an FP8 checkpoint — streamed, pinned compact, resident, through the sub-layer piece pool, and
generating through decode graphs — equals the same run on its fp16 twin in every bit while moving
half the weight bytes."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp8_ref as fr  # noqa: E402

from flexible_llm_sharding_amd import fp8  # noqa: E402

HAS_GPU = torch.cuda.is_available()
gpu = pytest.mark.gpu
needs_gpu = pytest.mark.skipif(not HAS_GPU, reason="needs an MI355X")
DEV = torch.device("cuda", 0)
CANARY = 64


def _tail() -> int:
    from flexible_llm_sharding_amd import _native
    return int(_native.kernels().fls_dequant_fp8_tail())


def _shapes():
    """(rows, cols) per element count: 1, 15, 16, 17, T - 1, T, T + 1, 2T + 16, 3T - 1 (flat counts
    factored so that channel and block scales have several rows where the count allows), and the two
    matrices.  T is the tail size the kernel library exports."""
    T = _tail()
    flat = [1, 15, 16, 17, T - 1, T, T + 1, 2 * T + 16, 3 * T - 1]
    out = []
    for n in flat:
        rows = next(r for r in (24, 16, 9, 7, 5, 3, 1) if n % r == 0)
        out.append((rows, n // rows))
    return out + [(200, 328), (1024, 2048)]


def _scale(kind: int, rows: int, cols: int, g: torch.Generator, extreme: bool) -> torch.Tensor:
    shape = {fp8.KIND_TENSOR: (1,), fp8.KIND_CHANNEL: (rows, 1),
             fp8.KIND_BLOCK: (-(-rows // 128), -(-cols // 128))}[kind]
    n = int(np.prod(shape))
    if extreme:
        pool = torch.tensor(fr.EXTREME_SCALES, dtype=torch.float32)
        return pool[torch.randint(0, len(pool), (n,), generator=g)].reshape(shape)
    return ((torch.rand(n, generator=g) + 0.5) * 2e-2).reshape(shape)


def _patterns(n: int, g: torch.Generator, mode: str) -> torch.Tensor:
    if mode == "random":
        return torch.randint(0, 256, (n,), generator=g, dtype=torch.int16).to(torch.uint8)
    # every one of the 256 patterns in every 16-byte lane position: element i holds pattern
    # (i // 16 + i % 16 * 17) % 256, so lane j of consecutive vectors walks all 256 patterns
    i = torch.arange(n, dtype=torch.int64)
    return ((i // 16 + (i % 16) * 17) % 256).to(torch.uint8)


def _run_kernel(ops, bits: torch.Tensor, scale: torch.Tensor, kind: int, rows: int, cols: int, base_off: int):
    """The kernel in place on a region at ``base_off`` bytes past a 256-byte aligned address, between
    two canaries.  Returns (fp16 result, canaries intact)."""
    n = rows * cols
    buf = torch.full((512 + base_off + 2 * n + CANARY,), 0xA5, dtype=torch.uint8, device=DEV)
    start = (-buf.data_ptr()) % 256 + 256 + base_off             # (at least 256 >= CANARY bytes in front)
    assert (buf.data_ptr() + start - base_off) % 256 == 0
    region = buf[start:start + 2 * n]
    region[n:].copy_(bits.to(DEV))
    region[:n].fill_(0x5A)                                       # stale bytes of the slot's last occupant
    s = scale.reshape(-1).contiguous().to(DEV)
    ops.dequant_fp8(region, n, s, kind, cols)
    torch.cuda.synchronize()
    host = buf.cpu()
    ok = bool((host[:start] == 0xA5).all()) and bool((host[start + 2 * n:] == 0xA5).all())
    return host[start:start + 2 * n].clone().view(torch.float16).reshape(rows, cols), ok


@gpu
@needs_gpu
@pytest.mark.parametrize("base_off", [0, 2, 6])
@pytest.mark.parametrize("kind", [fp8.KIND_TENSOR, fp8.KIND_CHANNEL, fp8.KIND_BLOCK])
def test_dequant_equals_host(kind, base_off):
    from flexible_llm_sharding_amd import _native
    from flexible_llm_sharding_amd.ops import get_ops
    ops = get_ops(DEV)
    g = torch.Generator().manual_seed(100 * kind + base_off)
    T = _tail()
    assert T >= 16 and T % 16 == 0
    seen = set()
    for rows, cols in _shapes():
        n = rows * cols
        seen.add(n)
        for mode, extreme in (("lanes", False), ("lanes", True), ("random", False)):
            bits = _patterns(n, g, mode)
            scale = _scale(kind, rows, cols, g, extreme)
            want = fp8.dequantize(bits.reshape(rows, cols), scale)
            got, intact = _run_kernel(ops, bits, scale, kind, rows, cols, base_off)
            assert intact, (rows, cols, mode, "canary overwritten")
            assert fr.same_bits(got, want), (rows, cols, mode, extreme)
            if (rows, cols) in ((200, 328), (24, (2 * T + 16) // 24)):
                again, intact = _run_kernel(ops, bits, scale, kind, rows, cols, base_off)
                assert intact and torch.equal(again.view(torch.int16), got.view(torch.int16))
    assert seen >= {1, 15, 16, 17, T - 1, T, T + 1, 2 * T + 16, 3 * T - 1, 200 * 328, 1024 * 2048}
    # the launch count is about log2(n / T) + 1; nothing to do for an empty tensor
    k = _native.kernels()
    assert k.fls_dequant_fp8_launches(T) == 1 and k.fls_dequant_fp8_launches(T + 16) == 2
    assert 15 <= k.fls_dequant_fp8_launches(8192 * 28672) <= 20
    assert k.fls_dequant_fp8(None, 0, None, 0, 1, None) == 0


@gpu
@needs_gpu
def test_dequant_refusals():
    from flexible_llm_sharding_amd import _native
    from flexible_llm_sharding_amd.ops import get_ops
    ops, k = get_ops(DEV), _native.kernels()
    region = torch.zeros(2 * 64, dtype=torch.uint8, device=DEV)
    s = torch.ones(8, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError):
        ops.dequant_fp8(region, 60, s[:1], 0, 60)                # region is not 2 bytes per weight
    with pytest.raises(ValueError):
        ops.dequant_fp8(region, 64, s[:3], 1, 8)                 # 8 rows need 8 scales
    with pytest.raises(TypeError):
        ops.dequant_fp8(region, 64, s[:1].cpu(), 0, 64)
    with pytest.raises(TypeError):
        ops.dequant_fp8(region, 64, s[:1].half(), 0, 64)
    assert k.fls_dequant_fp8(region.data_ptr() + 1, 32, s.data_ptr(), 0, 32, None) != 0   # odd address
    assert k.fls_dequant_fp8(region.data_ptr(), 64, s.data_ptr(), 1, 7, None) != 0        # 64 % 7
    assert k.fls_dequant_fp8(region.data_ptr(), 64, s.data_ptr(), 3, 8, None) != 0        # no such kind
    assert k.fls_dequant_fp8(region.data_ptr(), 64, None, 0, 64, None) != 0
    torch.cuda.synchronize()
    assert not region.any()


# ---------------------------------------------------------------------- engine
PRESETS = {"tiny": "channel", "tiny-qwen2": "tensor", "tiny-phi3": "block128", "tiny-mixtral": "channel"}
_PAIRS = {}


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    """(cfg, fp8 dir, twin dir, tokenizer, prompts, the twin's scores per lnps) per preset, built once."""
    root = tmp_path_factory.mktemp("fp8_gpu")

    def get(name):
        if name not in _PAIRS:
            from flexible_llm_sharding_amd.utils.tokenizer import load_tokenizer
            cfg, q, twin = fr.make_pair(root, name, PRESETS[name])
            _PAIRS[name] = (cfg, q, twin, load_tokenizer(q), fr.prompts_for(cfg, 4), {})
        return _PAIRS[name]
    return get


def _twin_scores(p, lnps, **kw):
    """The twin's scores through the ordinary FileLayerSource, once per (lnps, cap)."""
    from flexible_llm_sharding_amd.engine import ShardedRunner
    from flexible_llm_sharding_amd.runtime.stream import FileLayerSource
    cfg, q, twin, tok, prompts, cache = p
    key = (lnps, tuple(sorted(kw.items())))
    if key not in cache:
        r = ShardedRunner(cfg, FileLayerSource(cfg, twin), DEV, tok, layer_num_per_shard=lnps, **kw)
        cache[key] = r(prompts)
        r.close()
    return cache[key]


def _source(mode, cfg, q):
    from flexible_llm_sharding_amd.runtime.stream import FileLayerSource
    from flexible_llm_sharding_amd.runtime.weights import CompactHostStore
    if mode == "compact":
        return CompactHostStore(FileLayerSource(cfg, q))
    return FileLayerSource(cfg, q, chunk_mb=1, n_chunks=2, direct=mode == "stream_direct")


@gpu
@needs_gpu
@pytest.mark.parametrize("mode,lnps", [(m, l) for m in ("stream", "stream_direct", "compact", "resident")
                                       for l in (1, 3)] + [("piece_pool", 1)])   # (the pool: one layer per shard)
@pytest.mark.parametrize("name", list(PRESETS))
def test_engine_fp8_bitwise_equals_twin(pair, name, mode, lnps):
    from flexible_llm_sharding_amd.engine import ShardedRunner
    from flexible_llm_sharding_amd.runtime.prefetch import PiecePoolPrefetcher
    p = pair(name)
    cfg, q, twin, tok, prompts, _ = p
    kw = {"resident": True} if mode == "resident" else {"max_vram_gb": 40} if mode == "piece_pool" else {}
    # (a capped run plans its own chunks: its twin runs under the same cap)
    want = _twin_scores(p, lnps, **({"max_vram_gb": 40} if mode == "piece_pool" else {}))
    src = _source("compact" if mode == "piece_pool" and name != "tiny" else mode, cfg, q)
    r = ShardedRunner(cfg, src, DEV, tok, layer_num_per_shard=lnps, **kw)
    if mode == "piece_pool":
        assert isinstance(r.prefetcher, PiecePoolPrefetcher)
    first = r(prompts)
    second = r(prompts)                      # slot rotation, re-expansion into a reused slot
    r.close()
    for w, a, b in zip(want, first, second):
        assert a.dtype == np.float16 and np.array_equal(w.view(np.uint16), a.view(np.uint16))
        assert np.array_equal(w.view(np.uint16), b.view(np.uint16))
    assert src.fp8_tensors() if hasattr(src, "fp8_tensors") else src.files.fp8_tensors()


@gpu
@needs_gpu
def test_generation_fp8_bitwise(pair):
    """num_gen_token = 3, resident weights, decode graphs: tokens and every step's scores equal the twin's."""
    import topk_ref as tr
    from flexible_llm_sharding_amd.runtime.stream import FileLayerSource
    cfg, q, twin, tok, prompts, _ = pair("tiny")
    runs = {}
    for tag, path in (("fp8", q), ("twin", twin)):
        runs[tag] = tr.generate((cfg, tok, prompts, FileLayerSource(cfg, path)), DEV, num_gen=3)
    a, b = runs["fp8"], runs["twin"]
    assert a.updated == b.updated and len(a.scores) == len(b.scores)
    for x, y in zip(a.scores, b.scores):
        assert x.shape[1] == 3 and np.array_equal(x.view(np.uint16), y.view(np.uint16))
    for sa, sb in zip(a.tokens, b.tokens):
        assert all(np.array_equal(u, v) for u, v in zip(sa, sb))
    assert a.stats[-1].get("graph_replays", 0) >= 1


@gpu
@needs_gpu
def test_fp8_moves_half_the_bytes(pair):
    from flexible_llm_sharding_amd.engine import ShardedRunner
    from flexible_llm_sharding_amd.models.layout import layer_layout
    from flexible_llm_sharding_amd.runtime.stream import FileLayerSource
    from flexible_llm_sharding_amd.runtime.weights import CompactHostStore
    cfg, q, twin, tok, prompts, _ = pair("tiny")
    names, dec = cfg.layer_names(), fr.decoder_names(cfg)
    src = FileLayerSource(cfg, q, chunk_mb=1, n_chunks=2)
    files = sum(src.plan(n).file_bytes for n in names)
    assert files == sum(fr.file_tensor_bytes(q, n) for n in names)
    # (two slots: the engine then prefetches nothing of the next call, so one call is one pass)
    r = ShardedRunner(cfg, src, DEV, tok, layer_num_per_shard=1, n_slots=2)
    r(prompts)
    torch.cuda.synchronize()
    st = src.stats()
    # one pass reads and copies exactly the files' tensor bytes
    assert int(st["h2d_bytes"]) == files and src.read_bytes == files == int(st["read_bytes"])
    r.close()
    # the compact store pins every tensor at a 16-byte aligned offset: sum of align16(bytes)
    store = CompactHostStore(FileLayerSource(cfg, q))
    a16 = lambda n: (n + 15) // 16 * 16                          # noqa: E731
    assert store.COMPACT_ALIGN == 16
    assert store.total_bytes == sum(a16(r_.numel * r_.src_es) for n in names for r_ in store.plan(n).runs)
    assert files <= store.total_bytes < files + 16 * sum(len(store.plan(n).runs) for n in names)
    # decoder layers only (tiny's fp16 embedding and head dominate a tiny model)
    image = sum(layer_layout(cfg, "decoder").nbytes for _ in dec)
    dec_files = sum(src.plan(n).file_bytes for n in dec)
    dec_pinned = sum(store.buffers[n].numel() for n in dec)
    assert dec_files < 0.6 * image and dec_pinned < 0.6 * image
    store.close()
