"""MXFP4 checkpoints on an MI355X: ``fls_dequant_mxfp4`` equals mxfp4.dequantize in every bit for every
(nibble, scale byte) pair in every position of a thread's load, in place, inside the tensor's region;
a run on an MXFP4 checkpoint equals the run on its fp16 twin in every bit and moves N/2 + N/32 bytes."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import int4_ref as ir  # noqa: E402

from flexible_llm_sharding_amd import mxfp4  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]
DEV = torch.device("cuda", 0)
T = mxfp4.TAIL
ALL = 256 * 32 * 32                    # one block per (e, rotation): every pair in every nibble position


def _run_kernel(ops, packed, scale, n: int, base_off: int):
    """In place ``base_off`` bytes past a 256-byte aligned address, between canaries: (fp16 bits, canaries intact)."""
    host = torch.full((2 * n,), 0x5A, dtype=torch.uint8)
    mxfp4.land(host, packed.reshape(-1), scale.reshape(-1), n, 32, 1)
    buf = torch.full((512 + base_off + 2 * n + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    start = (-buf.data_ptr()) % 256 + 256 + base_off
    buf[start:start + 2 * n].copy_(host.to(DEV))
    ops.dequant_mxfp4(buf[start:start + 2 * n], n)
    torch.cuda.synchronize()
    back = buf.cpu()
    ok = bool((back[:start] == 0xA5).all()) and bool((back[start + 2 * n:] == 0xA5).all())
    return back[start:start + 2 * n].clone().view(torch.int16), ok


@pytest.mark.parametrize("base_off", [0, 2])                       # (2: the scalar path)
@pytest.mark.parametrize("n", [32, T - 32, T, T + 32, 5 * T + 64, ALL])
def test_dequant_mxfp4_equals_host(n, base_off):
    from flexible_llm_sharding_amd import _native
    from flexible_llm_sharding_amd.ops import get_ops
    ops, k = get_ops(DEV), _native.kernels()
    assert k.fls_dequant_mxfp4_tail() == T and k.fls_dequant_mxfp4_launches(n) == len(mxfp4.schedule(n, 32, 1))
    # block b holds the pair (b * 2731) % 8192 = e * 32 + r (2731 is odd: 8192 blocks hold every pair once);
    # its element p holds nibble (p + r) % 16
    idx = (torch.arange(n // 32) * 2731) % 8192
    u = (torch.arange(32)[None, :] + (idx % 32)[:, None]) % 16
    packed, scale = mxfp4.pack(u.to(torch.uint8)), (idx // 32).to(torch.uint8).reshape(-1, 1)
    want = mxfp4.dequantize(packed, scale, (n // 32, 32)).reshape(-1).view(torch.int16)
    got, intact = _run_kernel(ops, packed, scale, n, base_off)
    bad = torch.nonzero(got != want).reshape(-1)[:8]
    assert intact and bad.numel() == 0, [(int(i), int(scale[i // 32]), hex(int(got[i]) & 0xFFFF)) for i in bad]
    again, intact = _run_kernel(ops, packed, scale, n, base_off)
    assert intact and torch.equal(again, got)


def test_dequant_mxfp4_refusals():
    from flexible_llm_sharding_amd import _native
    k = _native.kernels()
    region = torch.full((2 * 128,), 0x5A, dtype=torch.uint8, device=DEV)
    p = region.data_ptr()
    assert k.fls_dequant_mxfp4(None, 128, None) != 0                        # a null pointer
    assert k.fls_dequant_mxfp4(p + 1, 64, None) != 0                        # an odd region address
    assert k.fls_dequant_mxfp4(p, 48, None) != 0                            # n % 32
    assert k.fls_dequant_mxfp4(None, 0, None) == 0
    torch.cuda.synchronize()
    assert bool((region == 0x5A).all())


# ---------------------------------------------------------------------- engine
@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    """(cfg, mxfp4 dir, twin dir, tokenizer, prompts) of the tiny preset; the --max_vram_gb case's cap is lifted after."""
    from flexible_llm_sharding_amd.config import preset
    from flexible_llm_sharding_amd.utils.synthetic import write_synthetic_checkpoint
    from flexible_llm_sharding_amd.utils.tokenizer import load_tokenizer
    root = tmp_path_factory.mktemp("mxfp4_gpu")
    cfg, q, twin = preset("tiny"), str(root / "q"), str(root / "twin")
    write_synthetic_checkpoint(cfg, q, seed=3, std=0.05, quantize="mxfp4")
    mxfp4.write_twin(q, twin)
    yield cfg, q, twin, load_tokenizer(q), ir.prompts_for(cfg, 4)
    torch.cuda.set_per_process_memory_fraction(1.0, DEV)


def _scores(pair, path, host=False, **kw):
    """(two calls' scores, memory plan, source) of a run on ``path``; the second call re-expands into a reused slot."""
    from flexible_llm_sharding_amd.engine import ShardedRunner
    from flexible_llm_sharding_amd.runtime.stream import FileLayerSource
    from flexible_llm_sharding_amd.runtime.weights import CompactHostStore
    cfg, _, _, tok, prompts = pair
    files = FileLayerSource(cfg, path, chunk_mb=1, n_chunks=2)
    r = ShardedRunner(cfg, CompactHostStore(files) if host else files, DEV, tok, layer_num_per_shard=1, **kw)
    out, plan = list(r(prompts)) + list(r(prompts)), r.vram_plan
    r.close()
    return out, plan, files


def _same(a, b) -> bool:
    return len(a) == len(b) and all(np.array_equal(x.view(np.uint16), y.view(np.uint16)) for x, y in zip(a, b))


@pytest.mark.parametrize("mode", ["stream", "host", "resident", "max_vram_gb"])
def test_engine_mxfp4_bitwise_equals_twin(pair, mode):
    cfg, q, twin = pair[:3]
    cap = {"max_vram_gb": 40} if mode == "max_vram_gb" else {}
    want, want_plan, _ = _scores(pair, twin, **cap)
    got, plan, files = _scores(pair, q, host=mode == "host", resident=mode == "resident", **cap)
    assert _same(want, got)
    if cap:                                     # no table arena: a capped run plans exactly as on the twin
        assert all(plan[k] == want_plan[k] for k in ("token_budget", "mlp_chunk", "attn_rows", "qkv_chunk"))
    assert files.mxfp4_tensors() == 7 * cfg.num_hidden_layers and files.scale_arena_bytes() == 0


def test_generation_mxfp4_bitwise(pair):
    """Two generated tokens: tokens and every step's scores equal the twin's."""
    import topk_ref as tr
    from flexible_llm_sharding_amd.runtime.stream import FileLayerSource
    cfg, q, twin, tok, prompts = pair
    a, b = (tr.generate((cfg, tok, prompts, FileLayerSource(cfg, path)), DEV, num_gen=2) for path in (q, twin))
    assert a.updated == b.updated and _same(a.scores, b.scores) and a.scores[0].shape[1] == 2
    assert all(np.array_equal(u, v) for sa, sb in zip(a.tokens, b.tokens) for u, v in zip(sa, sb))


def test_mxfp4_lora_bitwise_equals_twin(pair, tmp_path):
    """--lora on the MXFP4 base (merged after the expansion, on every landing) equals --lora on its twin."""
    from flexible_llm_sharding_amd import lora
    cfg, q, twin = pair[:3]
    adapter = lora.LoraAdapter.load(cfg, lora.write_synthetic_adapter(cfg, str(tmp_path / "adapter"), r=4, seed=1))
    assert _same(_scores(pair, twin, lora=adapter)[0], _scores(pair, q, lora=adapter)[0])


def test_mxfp4_moves_a_quarter_of_the_bytes(pair):
    from flexible_llm_sharding_amd.engine import ShardedRunner
    from flexible_llm_sharding_amd.runtime.stream import FileLayerSource
    cfg, q, twin, tok, prompts = pair
    src, tsrc = FileLayerSource(cfg, q, chunk_mb=1, n_chunks=2), FileLayerSource(cfg, twin)
    want = 0
    for n in cfg.layer_names():
        N = sum(r_.numel for r_ in src.plan(n).runs if r_.is_mxfp4)
        rest = sum(r_.file_nbytes for r_ in src.plan(n).runs if not r_.is_mxfp4)
        assert tsrc.plan(n).file_bytes == 2 * N + rest and src.plan(n).file_bytes == N // 2 + N // 32 + rest
        want += N // 2 + N // 32 + rest
    # (two slots: the engine then prefetches nothing of the next call, so one call is one pass)
    r = ShardedRunner(cfg, src, DEV, tok, layer_num_per_shard=1, n_slots=2)
    r(prompts)
    torch.cuda.synchronize()
    st = src.stats()
    assert int(st["h2d_bytes"]) == want == src.read_bytes == int(st["read_bytes"]) == src.file_bytes()
    r.close()
