"""--suffix_attention bidirectional without a GPU: torch backend and oracle against HF under the rule's 4-D mask,
the flag's default and refusals, the packer's seg_hi and widened range 1."""
import numpy as np
import pytest
import torch
from attention_rows import _tps
from flexible_llm_sharding_amd.engine import ShardedRunner
from flexible_llm_sharding_amd.models.reference import reference_embeddings
from flexible_llm_sharding_amd.runtime.batch import pack_prompts, visible_keys
from flexible_llm_sharding_amd.runtime.stream import FileLayerSource
from flexible_llm_sharding_amd.utils.cli import parse_args
from flexible_llm_sharding_amd.utils.tokenizer import tokenize_prompts
from test_embed_cpu import ATOL_HF, ATOL_ORACLE, _runner, model  # noqa: F401  (the tiny checkpoint and its prompts)


@pytest.mark.parametrize("mode", ["bidirectional", "causal"])
def test_torch_backend_and_oracle_match_hf_under_the_mask(model, mode):  # noqa: F811
    """Bounds: tests/test_embed_cpu.py's (2e-3 against HF on unit vectors, 1e-4 against the oracle)."""
    transformers = pytest.importorskip("transformers")
    d, cfg, tok, sd, prompts = model
    hf = transformers.LlamaModel(transformers.LlamaConfig(
        hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size, num_attention_heads=cfg.num_attention_heads,
        num_key_value_heads=cfg.num_key_value_heads, num_hidden_layers=cfg.num_hidden_layers, vocab_size=cfg.vocab_size,
        rms_norm_eps=cfg.rms_norm_eps, rope_theta=cfg.rope_theta, max_position_embeddings=cfg.max_position_embeddings,
        tie_word_embeddings=False)).float().eval()
    hf.load_state_dict({k[len("model."):]: v.float() for k, v in sd.items() if k.startswith("model.")})
    kw = dict(embed_pooling="mean", prefix_attention=mode, suffix_attention="bidirectional")
    got, causal = _runner(model, **kw)(prompts), _runner(model, **dict(kw, suffix_attention="causal"))(prompts)
    ref = reference_embeddings(cfg, sd, tok, prompts, "mean", 0, True, mode, suffix_attention="bidirectional")
    for pi, tp in enumerate(tokenize_prompts(tok, prompts, 4096)):
        assert np.abs(got[pi] - ref[pi]).max() <= ATOL_ORACLE and np.abs(got[pi] - causal[pi]).max() > 10 * ATOL_HF
        for si, u in enumerate(tp.suffixes):
            Lp, L = len(tp.prefix), len(tp.prefix) + len(u)
            see = torch.ones(L, L, dtype=torch.bool)             # a suffix row: the prefix and its whole suffix
            see[:Lp] = torch.ones(Lp, L, dtype=torch.bool).tril() if mode == "causal" else torch.arange(L) < Lp
            mask = torch.zeros(L, L).masked_fill(~see, torch.finfo(torch.float32).min)[None, None]
            with torch.no_grad():
                hs = hf(torch.tensor([tp.prefix + u]), attention_mask=mask).last_hidden_state[0, Lp:]
            want = torch.nn.functional.normalize(hs.mean(0), dim=0, eps=1e-12).numpy()
            assert np.abs(got[pi][si] - want).max() <= ATOL_HF


@pytest.mark.parametrize("extra", [[], ["--score_mode", "loglik"], ["--score_mode", "embed", "--sliding_window_mode", "apply"]])
def test_flag_default_and_refusals(model, extra):  # noqa: F811
    d, cfg, tok, sd, prompts = model
    base = ["--prompt_pickle", "p", "--output_file", "o"]
    assert parse_args(base + extra[:2]).suffix_attention == "causal"
    with pytest.raises(ValueError, match="--suffix_attention"):
        parse_args(base + extra + ["--suffix_attention", "bidirectional"])
    with pytest.raises(ValueError, match="--suffix_attention"):
        ShardedRunner(cfg, FileLayerSource(cfg, d), "cpu", tok, suffix_attention="bidirectional",
                      **dict(zip(("score_mode", "sliding_window_mode"), extra[1::2])))


def test_packer_emits_seg_hi_and_widened_range_1():
    tps = _tps([(10, (70, 3, 130))])
    b, c = pack_prompts(tps, [0], q_block=64, suffix_bidirectional=True), pack_prompts(tps, [0], q_block=64)
    assert b.seg_hi.dtype == np.int32 and b.seg_hi.tolist() == [10] * 10 + [80] * 70 + [83] * 3 + [213] * 130
    # items of suffix rows [10, 74) [74, 138) [138, 202) [202, 213): range 1 = [min seg_lo, max seg_hi) of their rows
    assert b.work[1:, 6:].tolist() == [[10, 70], [10, 203], [83, 130], [83, 130]]
    assert visible_keys(b.work, b.seg_lo, 83, seg_hi=b.seg_hi) == [(0, 0, 9), (1, 83, 212)]
    assert c.seg_hi is None and "seg_hi" not in c.host_meta() and np.array_equal(b.work_last, c.work_last)
    for f in ("ids", "positions", "seg_lo", "last_idx", "prompt_rows", "prompt_items", "prompt_scored"):
        assert np.array_equal(getattr(b, f), getattr(c, f)), f
    assert np.array_equal(b.work[:, :7], c.work[:, :7]) and c.work[1:, 7].tolist() == [64, 128, 119, 130]
    with pytest.raises(ValueError, match="suffix_bidirectional"):
        pack_prompts(tps, [0], suffix_bidirectional=True, window=8)
