"""GPTQ / AWQ checkpoints on an MI355X: ``fls_repack_w4`` + ``fls_dequant_w4z`` equal gptq.dequantize in
every bit, in place, inside the tensor's region; a run on such a checkpoint equals the run on its fp16
twin in every bit and moves about a quarter of the bytes."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import int4_ref as ir  # noqa: E402

from flexible_llm_sharding_amd import gptq  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]
DEV = torch.device("cuda", 0)
# one word column and the tail launch only; both tile edges ragged; N = TAIL exactly; several segments with
# groups across their boundaries and three tiles along `out`; per channel with more than 64 word rows
SHAPES = [(8, 32, 32), (72, 96, 32), (64, 128, 128), (136, 320, 64), (520, 1024, 1024)]


@pytest.mark.parametrize("base_off", [0, 2])                       # (2: the path with 2-byte accesses)
@pytest.mark.parametrize("out,inn,g", SHAPES)
@pytest.mark.parametrize("layout", gptq.LAYOUTS)
def test_dequant_gptq_equals_host(layout, out, inn, g, base_off):
    from flexible_llm_sharding_amd.ops import get_ops
    n, G, gen = out * inn, inn // g, torch.Generator().manual_seed(out + inn)
    qshape = (inn // 8, out) if layout == "gptq" else (inn, out // 8)
    qweight = torch.randint(-2 ** 31, 2 ** 31, qshape, generator=gen, dtype=torch.int64).to(torch.int32)
    qzeros = torch.randint(-2 ** 31, 2 ** 31, (G, out // 8), generator=gen, dtype=torch.int64).to(torch.int32)
    # normal scales of both signs; every eighth subnormal, every eleventh large enough to overflow at |u - z| >= 2
    scales = (torch.rand(G, out, generator=gen) - 0.5).to(torch.float16)
    scales.view(-1)[::8] = 2.0 ** -20
    scales.view(-1)[::11] = -40000.0
    want = gptq.dequantize(qweight, qzeros, scales, layout).reshape(-1)
    assert bool(torch.isinf(want).any()) and gptq.layout_of(qshape, scales.shape) == layout
    host = torch.full((2 * n,), 0x5A, dtype=torch.uint8)
    gptq.land(host, qweight, scales, qzeros, g)
    buf = torch.full((512 + base_off + 2 * n + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    start = (-buf.data_ptr()) % 256 + 256 + base_off
    for _ in range(2):                                             # (again: into a region that holds old output)
        buf[start:start + 2 * n].copy_(host.to(DEV))
        get_ops(DEV).dequant_gptq(buf[start:start + 2 * n], out, inn, g, layout)
        torch.cuda.synchronize()
        back = buf.cpu()
        got = back[start:start + 2 * n].clone().view(torch.float16)
        assert bool((back[:start] == 0xA5).all()) and bool((back[start + 2 * n:] == 0xA5).all())
        bad = torch.nonzero(got.view(torch.int16) != want.view(torch.int16)).reshape(-1)[:8]
        assert bad.numel() == 0, [(int(i) // inn, int(i) % inn, float(got[i]), float(want[i])) for i in bad]


def test_refused_arguments():
    from flexible_llm_sharding_amd import _native
    k = _native.kernels()
    region = torch.full((2 * 8 * 64,), 0x5A, dtype=torch.uint8, device=DEV)
    p = region.data_ptr()
    for args in ((None, 8, 64, 32, 0), (p + 1, 8, 64, 32, 0), (p, 12, 64, 32, 0), (p, 8, 48, 16, 0), (p, 8, 64, 48, 1),
                 (p, 8, 64, 32, 2)):                                 # null, odd address, out % 8, in % 32, in % g, layout
        assert k.fls_repack_w4(*args, None) != 0
    assert k.fls_dequant_w4z(None, 512, 32, None) != 0 and k.fls_dequant_w4z(p + 1, 512, 32, None) != 0
    assert k.fls_dequant_w4z(p, 512, 48, None) != 0 and k.fls_dequant_w4z(None, 0, 32, None) == 0
    torch.cuda.synchronize()
    assert bool((region == 0x5A).all())


# ---------------------------------------------------------------------- engine
@pytest.fixture(scope="module", params=gptq.LAYOUTS)
def pair(request, tmp_path_factory):
    """(cfg, checkpoint dir, twin dir, tokenizer, prompts, layout) of the tiny preset at g = 128."""
    from flexible_llm_sharding_amd.config import preset
    from flexible_llm_sharding_amd.utils.synthetic import write_synthetic_checkpoint
    from flexible_llm_sharding_amd.utils.tokenizer import load_tokenizer
    root = tmp_path_factory.mktemp("gptq_gpu")
    cfg, q, twin = preset("tiny"), str(root / "q"), str(root / "twin")
    write_synthetic_checkpoint(cfg, q, seed=3, std=0.05, quantize=request.param, int4_group=128)
    gptq.write_twin(q, twin)
    yield cfg, q, twin, load_tokenizer(q), ir.prompts_for(cfg, 4), request.param
    torch.cuda.set_per_process_memory_fraction(1.0, DEV)            # (the max_vram_gb case's cap is lifted)


def _scores(pair, path, **kw):
    """(two calls' scores, memory plan, source) of a run on ``path``; the second call re-expands into a reused slot."""
    from flexible_llm_sharding_amd.engine import ShardedRunner
    from flexible_llm_sharding_amd.runtime.stream import FileLayerSource
    cfg, tok, prompts = pair[0], pair[3], pair[4]
    files = FileLayerSource(cfg, path, chunk_mb=1, n_chunks=2)
    r = ShardedRunner(cfg, files, DEV, tok, layer_num_per_shard=1, **kw)
    out, plan = list(r(prompts)) + list(r(prompts)), r.vram_plan
    r.close()
    return out, plan, files


def _same(a, b) -> bool:
    return len(a) == len(b) and all(np.array_equal(x.view(np.uint16), y.view(np.uint16)) for x, y in zip(a, b))


@pytest.mark.parametrize("mode", ["stream", "resident", "max_vram_gb"])
def test_engine_bitwise_equals_twin(pair, mode):
    cfg, q, twin, layout = pair[0], pair[1], pair[2], pair[5]
    cap = {"max_vram_gb": 40} if mode == "max_vram_gb" else {}
    want, want_plan, _ = _scores(pair, twin, **cap)
    got, plan, files = _scores(pair, q, resident=mode == "resident", **cap)
    assert _same(want, got)
    if cap:                                     # no tables, no arena: a capped run plans exactly as on the twin
        assert all(plan[k] == want_plan[k] for k in ("token_budget", "mlp_chunk", "attn_rows", "qkv_chunk"))
    assert files.tensors()[layout] == 7 * cfg.num_hidden_layers and files.scale_arena_bytes() == 0


def test_generation_bitwise(pair):
    """Two generated tokens: tokens and every step's scores equal the twin's."""
    import topk_ref as tr
    from flexible_llm_sharding_amd.runtime.stream import FileLayerSource
    cfg, q, twin, tok, prompts = pair[:5]
    a, b = (tr.generate((cfg, tok, prompts, FileLayerSource(cfg, path)), DEV, num_gen=2) for path in (q, twin))
    assert a.updated == b.updated and _same(a.scores, b.scores) and a.scores[0].shape[1] == 2
    assert all(np.array_equal(u, v) for sa, sb in zip(a.tokens, b.tokens) for u, v in zip(sa, sb))


def test_moves_a_quarter_of_the_bytes(pair):
    """At g = 128 a weight moves N / 2 + 2 N / g + N / 2g bytes, 0.26 of the twin's 2 N: at most 0.3."""
    from flexible_llm_sharding_amd.engine import ShardedRunner
    from flexible_llm_sharding_amd.runtime.stream import FileLayerSource
    cfg, q, twin, tok, prompts = pair[:5]
    src, tsrc = FileLayerSource(cfg, q, chunk_mb=1, n_chunks=2), FileLayerSource(cfg, twin)
    for n in ir.decoder_names(cfg):
        runs = [r_ for r_ in src.plan(n).runs if r_.lands_repacked]
        rest = sum(r_.file_nbytes for r_ in src.plan(n).runs if not r_.lands_repacked)
        moved, twin_moved = src.plan(n).file_bytes - rest, tsrc.plan(n).file_bytes - rest
        assert len(runs) == 7 and twin_moved == 2 * sum(r_.numel for r_ in runs) and moved <= 0.3 * twin_moved
    # (two slots: the engine then prefetches nothing of the next call, so one call is one pass)
    r = ShardedRunner(cfg, src, DEV, tok, layer_num_per_shard=1, n_slots=2)
    r(prompts)
    torch.cuda.synchronize()
    st = src.stats()
    assert int(st["h2d_bytes"]) == src.read_bytes == int(st["read_bytes"]) == src.file_bytes()
    r.close()
