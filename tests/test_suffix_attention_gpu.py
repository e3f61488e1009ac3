"""--suffix_attention bidirectional on the GPU: kernel against fp32 torch under the rule's mask, isolation, engine."""
import numpy as np
import pytest
import torch
from attention_rows import _tps
from flexible_llm_sharding_amd.embed import layer_names
from flexible_llm_sharding_amd.engine import ShardedRunner
from flexible_llm_sharding_amd.ops import get_ops
from flexible_llm_sharding_amd.runtime.batch import pack_prompts
from flexible_llm_sharding_amd.runtime.stream import FileLayerSource
from test_embed_gpu import model  # noqa: F401  (the tiny checkpoint and its prompts)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
# one-row suffixes, several suffixes in an item, a suffix ending on a key tile, suffixes straddling items and tiles
PROMPTS = [(lp, s) for lp in (1, 64, 100) for s in [(1,), (2, 1, 3), (63, 1, 64, 65), (130,), (70, 3, 130)]]


def _case(nh, nkv, hd, mode, q_block):
    b = pack_prompts(_tps(PROMPTS), list(range(len(PROMPTS))), mode, q_block=q_block, suffix_bidirectional=True)
    qkv = torch.randn(b.num_tokens, (nh + 2 * nkv) * hd, generator=torch.Generator().manual_seed(3))
    mask, sfx, t = torch.zeros(b.num_tokens, b.num_tokens, dtype=torch.bool), [], 0
    for lp, s in PROMPTS:          # the rule: the prefix as --prefix_attention says, the whole own suffix, nothing else
        p0, t = t, t + lp
        mask[p0:t, p0:t] = torch.ones(lp, lp, dtype=torch.bool).tril() if mode == "causal" else True
        for n in s:
            mask[t:t + n, p0:p0 + lp] = mask[t:t + n, t:t + n] = True
            qkv[t + n - 1, nh * hd:(nh + nkv) * hd] *= 6.0     # a large score at the last key: maxima after the diagonal
            sfx.append((t, t + n))
            t += n
    return b, qkv.to(torch.float16), mask, sfx


def _run(b, qkv, nh, nkv, hd):
    m = b.device_tensors(DEV)
    return get_ops(DEV).attention(qkv.to(DEV), m["work"], nh, nkv, hd, q_block=b.q_block, seg_lo=m["seg_lo"],
                                  seg_hi=m["seg_hi"]).cpu()


@pytest.mark.parametrize("mode", ["bidirectional", "causal"])
@pytest.mark.parametrize("q_block", [64, 128])
@pytest.mark.parametrize("nh,nkv,hd", [(4, 1, 64), (2, 2, 64), (4, 1, 96), (2, 2, 96), (4, 1, 128), (2, 2, 128)])
def test_kernel_matches_fp32_masked_attention(nh, nkv, hd, q_block, mode):
    """Tolerance: tests/test_kernels_gpu.py::test_attention_multi_suffix_items (5e-3 of the norm)."""
    b, qkv, mask, _ = _case(nh, nkv, hd, mode, q_block)
    T, x = b.num_tokens, qkv.float()
    q, k, v = (x[:, a * hd:c * hd].view(T, -1, hd) for a, c in ((0, nh), (nh, nh + nkv), (nh + nkv, nh + 2 * nkv)))
    k, v = (u.repeat_interleave(nh // nkv, dim=1) for u in (k, v))
    s = (torch.einsum("qhd,khd->hqk", q, k) * hd ** -0.5).masked_fill(~mask[None], float("-inf"))
    ref = torch.einsum("hqk,khd->qhd", torch.softmax(s, -1), v).reshape(T, nh * hd)
    y = _run(b, qkv, nh, nkv, hd).float()
    assert torch.isfinite(y).all() and ((y - ref).norm() / ref.norm()).item() < 5e-3


@pytest.mark.parametrize("q_block", [64, 128])
def test_other_suffixes_do_not_move_a_bit(q_block):
    b, qkv, _, sfx = _case(4, 1, 128, "bidirectional", q_block)
    y = _run(b, qkv, 4, 1, 128)
    for a, e in (sfx[-2], sfx[6]):             # the 3 of a (70, 3, 130) and the 64 of a (63, 1, 64, 65)
        other, rows = qkv.clone(), torch.ones(b.num_tokens, dtype=torch.bool)
        other[a:e] = torch.randn(e - a, qkv.shape[1], generator=torch.Generator().manual_seed(9)).to(torch.float16)
        rows[a:e] = False
        z = _run(b, other, 4, 1, 128)
        assert torch.equal(y[rows].view(torch.int16), z[rows].view(torch.int16)) and (y[a:e] != z[a:e]).any(dim=1).all()


def test_engine_embeds_bidirectionally(model):  # noqa: F811
    """Bound: tests/test_embed_gpu.py's, twice the error E of the causal ``last`` rows against the same reference."""
    d, cfg, tok, prompts, sd, state = model

    def emb(dev, pooling, attn, **kw):
        src = state["store"] if dev == DEV else FileLayerSource(cfg, d, names=layer_names(cfg, "embed"))
        r = ShardedRunner(cfg, src, dev, tok, score_mode="embed", embed_pooling=pooling, embed_normalize=False,
                          suffix_attention=attn, **kw)
        out = np.concatenate(r(prompts))
        r.close()
        return out
    E = float(np.abs(emb(DEV, "last", "causal") - emb("cpu", "last", "causal")).max())
    want, causal = emb("cpu", "mean", "bidirectional"), emb(DEV, "mean", "causal")
    whole, capped = emb(DEV, "mean", "bidirectional"), emb(DEV, "mean", "bidirectional", max_vram_gb=40)
    torch.cuda.set_per_process_memory_fraction(1.0, DEV)            # (lift the capped run's allocator limit)
    print(f"E {E:.3g}; errors {np.abs(whole - want).max():.3g} {np.abs(capped - want).max():.3g}")
    for got in (whole, capped):
        assert np.abs(got - want).max() <= 2 * E and np.abs(got - causal).max() > 2 * E
    assert np.abs(emb(DEV, "last", "bidirectional") - emb(DEV, "last", "causal")).max() > 2 * E
