"""Pooled embeddings (``score_mode="embed"``) on the CPU backend: packing, the kernel cases'
own properties, ``pool_rows`` of the torch backend, the engine against ``reference_embeddings``
and HF transformers, refused combinations, the CLI, data parallel, a model directory without a
head and the converter on a checkpoint without the ``model.`` prefix.

Tolerances are those of tests/test_engine_cpu.py: 1e-4 absolute against the fp32 oracle
(test_engine_matches_oracle), 2e-3 against HF (test_causal_prefix_matches_hf_transformers, whose
RoPE tables are not fp16-rounded).  The embeddings' entries are of order 1 (unnormalised) or
1 / sqrt(D) (normalised), like the probabilities those bounds were set for or larger."""
import json
import os
import pickle
import shutil
import socket
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import embed_ref as er  # noqa: E402

from flexible_llm_sharding_amd.config import preset  # noqa: E402
from flexible_llm_sharding_amd.embed import EmbedParams, layer_names  # noqa: E402
from flexible_llm_sharding_amd.engine import ShardedRunner  # noqa: E402
from flexible_llm_sharding_amd.models.reference import reference_embeddings  # noqa: E402
from flexible_llm_sharding_amd.ops import get_ops  # noqa: E402
from flexible_llm_sharding_amd.runtime.batch import pack_prompts  # noqa: E402
from flexible_llm_sharding_amd.runtime.stream import FileLayerSource  # noqa: E402
from flexible_llm_sharding_amd.utils.cli import parse_args  # noqa: E402
from flexible_llm_sharding_amd.utils.layer_format import layer_of_param, split_into_layers  # noqa: E402
from flexible_llm_sharding_amd.utils.safetensors_io import load_file, save_file  # noqa: E402
from flexible_llm_sharding_amd.utils.synthetic import (load_full_state_dict, synthetic_layer_state_dict,  # noqa: E402
                                                       write_synthetic_checkpoint)
from flexible_llm_sharding_amd.utils.tokenizer import (TokenizedPrompt, load_tokenizer, synthetic_word,  # noqa: E402
                                                       tokenize_prompts, write_synthetic_tokenizer)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL_ORACLE = 1e-4        # tests/test_engine_cpu.py::test_engine_matches_oracle
ATOL_HF = 2e-3            # tests/test_engine_cpu.py::test_causal_prefix_matches_hf_transformers
SHAPES = [(20, [1, 2, 9]), (12, [5, 3, 4]), (30, [7]), (9, [6, 2])]


# ------------------------------------------------------------------ packing
def _tp(prefix, suffixes):
    return TokenizedPrompt(list(prefix), [list(s) for s in suffixes], max(len(s) for s in suffixes),
                           [len(s) - 1 for s in suffixes])


def test_pack_pool_by_hand():
    long = list(range(100, 165))
    a = _tp([1, 5, 6], [[7], [8, 9], long])          # rows 0-2 prefix, 3 | 4 5 | 6..70
    b = _tp([1, 4], [[11, 12, 13]])                  # rows 71-72 prefix, 73 74 75
    m = pack_prompts([a, b], [0, 1], "bidirectional", pool="mean")
    assert m.last_idx.tolist() == [3, 4, 5] + list(range(6, 71)) + [73, 74, 75] and m.last_idx.dtype == np.int32
    assert m.seg_start.tolist() == [0, 1, 3, 68, 71] and m.seg_start.dtype == np.int32
    assert m.prompt_scored.tolist() == [[0, 68], [68, 71]]
    assert m.device_tensors("cpu")["seg_start"].tolist() == [0, 1, 3, 68, 71]
    # no prefix row is pooled
    assert not {0, 1, 2, 71, 72} & set(m.last_idx.tolist())
    la = pack_prompts([a, b], [0, 1], "bidirectional", pool="last")
    d = pack_prompts([a, b], [0, 1], "bidirectional")
    assert la.seg_start.tolist() == [0, 1, 2, 3, 4] and d.seg_start is None and "seg_start" not in d.host_meta()
    for f in ("ids", "positions", "work", "seg_lo", "last_idx", "work_last", "prompt_rows", "prompt_items", "prompt_scored"):
        assert np.array_equal(getattr(la, f), getattr(d, f)), f
        if f not in ("last_idx", "prompt_scored"):
            assert np.array_equal(getattr(m, f), getattr(d, f)), f
    with pytest.raises(ValueError, match="no token"):
        pack_prompts([TokenizedPrompt([1, 2], [[7], []], 1, [0, -1])], [0], pool="mean")
    with pytest.raises(ValueError, match="loglik"):
        pack_prompts([a], [0], pool="mean", loglik=True)
    with pytest.raises(ValueError, match="kv_cached"):
        pack_prompts([a], [0], pool="mean", prefix_offsets=[0], kv_cached=True)


# ------------------------------------------------------------------ the kernel cases, without a GPU
CASES = er.kernel_cases()
TAU = er.group_tau(CASES)


def test_kernel_cases_cover_the_issue_and_discriminate():
    """Every shape the kernel takes another path at is a case, tau > 0 in every group, and in
    every case dropping a segment's last row, or taking the next segment's first row into it,
    moves that segment's float64 oracle output by >= 4 tau (an all-zero segment cannot move by
    losing a zero row: it is only held to the second property)."""
    assert {c.H for c in CASES} >= {64, 520, 4096, 8192}
    assert set(er.RAGGED) == {1, 2, 63, 64, 65, 300}
    for H in (520, 4096):
        assert {c.D for c in CASES if c.H == H} >= {1, 7, 8, H - 8, H}
    assert {c.normalize for c in CASES} == {True, False}
    assert any(c.ld > c.H and c.ld % 8 == 0 for c in CASES) and any(c.ld % 8 for c in CASES)
    assert any(c.offset % 8 for c in CASES) and any(c.gather for c in CASES)
    assert any(0 in c.lens[1:-1] for c in CASES) and any(c.zero for c in CASES)
    assert any(np.abs(c.x.astype(np.float32)).min() == er.F16_MAX for c in CASES)
    n_drop = n_take = 0
    for c in CASES:
        tau = TAU[c.group]
        assert tau > 0, c.group
        for i, v in c.drop_last_effect().items():
            if i not in c.zero:
                assert v >= er.SEPARATION * tau, (c.name, "drop", i, v, tau)
                n_drop += 1
        for i, v in c.take_next_effect().items():
            assert v >= er.SEPARATION * tau, (c.name, "take", i, v, tau)
            n_take += 1
    assert n_drop >= 4 * len(CASES) - 2 and n_take >= 2 * len(CASES)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_torch_pool_rows_matches_fp64(case):
    """The torch backend's ``pool_rows`` (the CPU path) on the case's rows in float32.  Its bound
    is the case group's tau plus the error of torch's own summation order, bounded by n x 2^-24
    per unit of the largest partial sum (n <= 300 rows; the norm adds D more terms of relative
    2^-24 each, far below that)."""
    ops = get_ops(torch.device("cpu"))
    x = torch.from_numpy(case.x.astype(np.float32))
    ss = torch.from_numpy(case.seg_start)
    idx = None
    if case.gather:
        perm = np.random.default_rng(1).permutation(x.shape[0])
        stored = torch.empty_like(x)
        stored[perm] = x
        x, idx = stored, torch.from_numpy(perm.astype(np.int32))
    got = ops.pool_rows(x, ss, case.D, case.normalize, row_idx=idx)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(case.lens), case.D)
    ref = case.ref()
    scale = float(np.abs(case.x.astype(np.float64)).max()) if not case.normalize else 1.0
    bound = TAU[case.group] + max(case.lens) * 2.0 ** -24 * scale
    assert float(np.abs(got.numpy().astype(np.float64) - ref).max()) <= bound
    empty = [i for i, n in enumerate(case.lens) if n == 0]
    assert all((got[i] == 0).all() for i in empty)


def test_pool_rows_refuses_a_bad_dim():
    ops = get_ops(torch.device("cpu"))
    x, ss = torch.zeros(3, 8), torch.tensor([0, 3], dtype=torch.int32)
    for d in (-1, 9, True):
        with pytest.raises(ValueError, match="dim"):
            ops.pool_rows(x, ss, d)


# ------------------------------------------------------------------ engine vs the oracle
@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("embed_model"))
    cfg = preset("tiny")
    write_synthetic_checkpoint(cfg, d, seed=1, std=0.15)
    tok = load_tokenizer(d)
    rng = np.random.default_rng(5)

    def words(n):
        return " ".join(synthetic_word(int(i)) for i in rng.integers(3, cfg.vocab_size, n))

    prompts = [(words(lp - 1), tuple(words(n) for n in lens)) for lp, lens in SHAPES]
    tps = tokenize_prompts(tok, prompts, 4096)
    assert [[len(u) for u in tp.suffixes] for tp in tps] == [lens for _, lens in SHAPES]
    return d, cfg, tok, load_full_state_dict(cfg, d), prompts


def _runner(model, **kw):
    d, cfg, tok, sd, prompts = model
    return ShardedRunner(cfg, FileLayerSource(cfg, d, names=layer_names(cfg, "embed")), "cpu", tok, score_mode="embed", **kw)


_REF = {}


def _ref(model, pooling, dim, normalize, mode):
    key = (pooling, dim, normalize, mode)
    if key not in _REF:
        d, cfg, tok, sd, prompts = model
        _REF[key] = reference_embeddings(cfg, sd, tok, prompts, pooling, dim, normalize, mode)
    return _REF[key]


@pytest.mark.parametrize("pooling", ["last", "mean"])
@pytest.mark.parametrize("mode", ["bidirectional", "causal"])
@pytest.mark.parametrize("dim,normalize,kw", [(0, True, {}), (0, False, {"layer_num_per_shard": 3}),
                                              (24, True, {"token_budget": 40}), (7, False, {"storage_location": "disk"})])
def test_engine_embed_matches_oracle(model, tmp_path, pooling, mode, dim, normalize, kw):
    d, cfg, tok, sd, prompts = model
    r = _runner(model, embed_pooling=pooling, embed_dim=dim, embed_normalize=normalize, prefix_attention=mode,
                disk_folder=str(tmp_path), **kw)
    out = r(prompts)
    assert r.stats["micro_batches"] >= (2 if "token_budget" in kw else 1)
    ref = _ref(model, pooling, dim, normalize, mode)
    D = dim or cfg.hidden_size
    for o, rf, (_, lens) in zip(out, ref, SHAPES):
        assert o.dtype == np.float32 and o.shape == (len(lens), D) == rf.shape
        assert np.abs(o - rf).max() <= ATOL_ORACLE, np.abs(o - rf).max()
        if normalize:
            assert np.allclose(np.linalg.norm(o.astype(np.float64), axis=1), 1.0, atol=1e-5)
    assert r.score_d2h_bytes == 4 * D * sum(len(lens) for _, lens in SHAPES)
    assert "lm_head" not in r.names and r.names[-1] == "model.norm"
    # the oracle tells the poolings, the attentions and a shifted window apart by far more than the bound
    other = _ref(model, "mean" if pooling == "last" else "last", dim, normalize, mode)
    multi = [i for i, (_, lens) in enumerate(SHAPES) if max(lens) > 1]
    assert all(np.abs(ref[i] - other[i]).max() > 20 * ATOL_ORACLE for i in multi)
    out2 = r(prompts)                                  # a second call starts clean
    assert all(np.array_equal(a, b) for a, b in zip(out, out2))
    r.ctx.pool_chunk = 5                               # the norm phase in chunks of whole suffixes: the same bits
    assert all(np.array_equal(a, b) for a, b in zip(out, r(prompts)))
    r.close()


def test_mean_through_a_pruned_last_layer_agrees(model):
    """``set_mean_variant(True)`` (the last layer pruned to the suffix rows, the variant the
    profile compares): the same embeddings within the oracle bound, in one and several micro-batches."""
    d, cfg, tok, sd, prompts = model
    ref = _ref(model, "mean", 0, False, "bidirectional")
    for kw in ({}, {"token_budget": 40}):
        r = _runner(model, embed_pooling="mean", embed_normalize=False, **kw)
        r.set_mean_variant(True)
        out = r(prompts)
        assert all(o.shape == q.shape and np.abs(o - q).max() <= ATOL_ORACLE for o, q in zip(out, ref))
        r.set_mean_variant(False)
        assert all(np.abs(o - q).max() <= ATOL_ORACLE for o, q in zip(r(prompts), ref))
    with pytest.raises(ValueError, match="mean"):
        _runner(model).set_mean_variant(True)
    a = pack_prompts([_tp([1, 5, 6], [[7], [8, 9]])], [0], pool="last", score_rows=[[1, 2]])
    assert a.last_idx.tolist() == [3, 4, 5] and a.seg_start.tolist() == [0, 1, 3]


def test_last_is_the_row_the_head_scores(model):
    """``last``, unnormalised, D = H, through the checkpoint's head and a softmax: the next-token
    mode's distribution (to fp16 rounding of the returned scores)."""
    d, cfg, tok, sd, prompts = model
    emb = _runner(model, embed_normalize=False)(prompts)
    nt = ShardedRunner(cfg, FileLayerSource(cfg, d), "cpu", tok)(prompts)
    head = sd["lm_head.weight"].float()
    for e, s in zip(emb, nt):
        p = torch.softmax(torch.from_numpy(e) @ head.t(), -1).numpy()
        assert np.abs(p - s[:, 0].astype(np.float32)).max() <= 2.0 ** -11 + 1e-6


def test_embed_matches_hf_llama_model(model):
    """prefix_attention="causal": HF ``LlamaModel.last_hidden_state`` on prefix + suffix ids (the
    final norm applied), its last row and the mean of the suffix's rows, L2-normalised.  The bound
    is the existing HF test's 2e-3, which is absolute on values in [0, 1] (probabilities) and covers
    the engine's fp16-rounded RoPE tables against HF's fp32 ones — a relative perturbation.  The
    normalised embeddings it is applied to lie in [-1, 1]; raw hidden rows reach 2 to 3 here and
    would need the bound scaled by their size."""
    transformers = pytest.importorskip("transformers")
    d, cfg, tok, sd, prompts = model
    hf_cfg = transformers.LlamaConfig(
        hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
        num_attention_heads=cfg.num_attention_heads, num_key_value_heads=cfg.num_key_value_heads,
        num_hidden_layers=cfg.num_hidden_layers, vocab_size=cfg.vocab_size, rms_norm_eps=cfg.rms_norm_eps,
        rope_theta=cfg.rope_theta, max_position_embeddings=cfg.max_position_embeddings,
        tie_word_embeddings=False)
    hf = transformers.LlamaModel(hf_cfg).float().eval()
    hf.load_state_dict({k[len("model."):]: v.float() for k, v in sd.items() if k.startswith("model.")})
    got = {p: _runner(model, embed_pooling=p, prefix_attention="causal")(prompts) for p in ("last", "mean")}
    unit = lambda v: torch.nn.functional.normalize(v, dim=0, eps=1e-12).numpy()     # noqa: E731
    for pi, tp in enumerate(tokenize_prompts(tok, prompts, 4096)):
        for si, u in enumerate(tp.suffixes):
            with torch.no_grad():
                hs = hf(torch.tensor([tp.prefix + u])).last_hidden_state[0, len(tp.prefix):]
            assert np.abs(got["last"][pi][si] - unit(hs[-1])).max() <= ATOL_HF
            assert np.abs(got["mean"][pi][si] - unit(hs.mean(0))).max() <= ATOL_HF


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("kw,flag", [({"hip_graphs": True}, "--hip_graphs"),
                                     ({"prefix_kv_cache": True}, "--prefix_kv_cache"),
                                     ({"suffix_kv_cache": True}, "--suffix_kv_cache"),
                                     ({"resume_dir": "ck"}, "--resume_dir"),
                                     ({"score_top_k": 4}, "--score_top_k"),
                                     ({"embed_dim": 257}, "--embed_dim"),
                                     ({"embed_dim": -1}, "--embed_dim"),
                                     ({"embed_pooling": "max"}, "--embed_pooling")])
def test_runner_refuses(model, kw, flag):
    with pytest.raises(ValueError, match=flag):
        _runner(model, **kw)


def test_runner_refuses_sampling_model_parallel_and_stray_flags(model):
    from flexible_llm_sharding_amd.parallel.comm import Comm
    from flexible_llm_sharding_amd.sampling import SamplingParams
    d, cfg, tok, sd, prompts = model
    assert cfg.hidden_size == 256
    with pytest.raises(ValueError, match="--do_sample"):
        _runner(model, sampling=SamplingParams(temperature=0.7))
    with pytest.raises(ValueError, match="model parallel"):
        _runner(model, comm=Comm(0, 2))
    for kw, flag in (({"embed_pooling": "mean"}, "--embed_pooling"), ({"embed_dim": 8}, "--embed_dim"),
                     ({"embed_normalize": False}, "--embed_normalize")):
        for mode in ("next_token", "loglik"):
            with pytest.raises(ValueError, match=f"{flag} needs --score_mode embed"):
                ShardedRunner(cfg, FileLayerSource(cfg, d), "cpu", tok, score_mode=mode, **kw)
    r = _runner(model)
    with pytest.raises(ValueError, match="embed"):
        r.run_tokenized(r.tokenize(prompts), drafts=[[[] for _ in s] for _, s in prompts])


def test_mean_of_an_empty_suffix_raises(model):
    with pytest.raises(ValueError, match="no token to pool"):
        _runner(model, embed_pooling="mean")([("wd we wf", ("wg wh", ""))])
    assert _runner(model)([("wd we wf", ("wg wh", ""))])[0].shape == (2, 256)      # last: as the default mode


@pytest.mark.parametrize("extra,flag", [(["--num_gen_token", "2"], "--num_gen_token"),
                                        (["--do_sample"], "--do_sample"),
                                        (["--temperature", "0.5"], "--temperature"),
                                        (["--top_k", "5"], "--top_k"),
                                        (["--top_p", "0.5"], "--top_p"),
                                        (["--score_top_k", "4"], "--score_top_k"),
                                        (["--lookup_decoding", "2"], "--lookup_decoding"),
                                        (["--hip_graphs"], "--hip_graphs"),
                                        (["--prefix_kv_cache", "true"], "--prefix_kv_cache"),
                                        (["--suffix_kv_cache", "true"], "--suffix_kv_cache"),
                                        (["--resume_dir", "ck"], "--resume_dir"),
                                        (["--embed_dim", "-3"], "--embed_dim")])
def test_cli_refuses(extra, flag):
    base = ["--prompt_pickle", "p", "--output_file", "o"]
    with pytest.raises(ValueError, match=flag):
        parse_args(base + ["--score_mode", "embed"] + extra)


@pytest.mark.parametrize("extra,flag", [(["--embed_pooling", "mean"], "--embed_pooling"), (["--embed_dim", "8"], "--embed_dim"),
                                        (["--embed_normalize", "false"], "--embed_normalize"),
                                        (["--embed_normalize", "true"], "--embed_normalize")])
def test_cli_refuses_embed_flags_without_the_mode(extra, flag):
    base = ["--prompt_pickle", "p", "--output_file", "o"]
    for mode in ([], ["--score_mode", "loglik"]):
        with pytest.raises(ValueError, match=f"{flag} needs --score_mode embed"):
            parse_args(base + mode + extra)
    a = parse_args(base + ["--score_mode", "embed"] + extra)
    from flexible_llm_sharding_amd.api import resolve_prefix_kv_cache, resolve_suffix_kv_cache
    assert a.score_mode == "embed" and not resolve_prefix_kv_cache(a) and not resolve_suffix_kv_cache(a)
    d = parse_args(base + ["--score_mode", "embed"])
    assert EmbedParams.from_args(d) == EmbedParams("last", 0, True)
    assert parse_args(base).score_mode == "next_token"


def test_build_runner_refuses_model_parallel_and_a_dim_past_h(model):
    from flexible_llm_sharding_amd.api import build_runner
    from flexible_llm_sharding_amd.parallel.comm import Comm
    d, cfg, tok, sd, prompts = model
    base = ["--prompt_pickle", "p", "--output_file", "o", "--score_mode", "embed", "--model_path", d]
    with pytest.raises(ValueError, match="model parallel"):
        build_runner(parse_args(base), cfg, "cpu", Comm(0, 2), tok)
    with pytest.raises(ValueError, match="--embed_dim"):
        build_runner(parse_args(base + ["--embed_dim", str(cfg.hidden_size + 1)]), cfg, "cpu", Comm(0, 1), tok)


# ------------------------------------------------------------------ CLI, batches, data parallel
def _main(tmp_path, d, prompts, *extra):
    pp = tmp_path / "prompts.pkl"
    pickle.dump(prompts, open(pp, "wb"))
    out, mj = tmp_path / "emb.pkl", tmp_path / "metrics.json"
    env = dict(os.environ, PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--model_path", d, "--prompt_pickle", str(pp),
                        "--output_file", str(out), "--score_mode", "embed", "--metrics_json", str(mj),
                        "--disk_folder", str(tmp_path / "spill"), *extra],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    return p, out, mj


def test_main_embed_end_to_end(model, tmp_path):
    """main.py with --num_batch 2: the file format, the prompts written back unchanged, the metrics."""
    d, cfg, tok, sd, prompts = model
    p, out, mj = _main(tmp_path, d, prompts, "--embed_pooling", "mean", "--embed_dim", "24", "--num_batch", "2",
                       "--prefix_attention", "causal")
    assert p.returncode == 0, p.stderr[-3000:]
    res = pickle.load(open(out, "rb"))
    assert set(res) == {"embeddings", "pooling", "dim", "normalized"}
    assert (res["pooling"], res["dim"], res["normalized"]) == ("mean", 24, True)
    ref = _ref(model, "mean", 24, True, "causal")
    assert len(res["embeddings"]) == len(prompts)
    for o, rf in zip(res["embeddings"], ref):
        assert o.dtype == np.float32 and o.shape == rf.shape and np.abs(o - rf).max() <= ATOL_ORACLE
    assert pickle.load(open(tmp_path / "prompts_updated.pkl", "rb")) == list(prompts)
    m = json.load(open(mj))
    assert (m["score_mode"], m["embed_pooling"], m["embed_dim"], m["embed_normalize"]) == ("embed", "mean", 24, True)
    # --num_batch 2 equals one batch, prompt by prompt
    one = _runner(model, embed_pooling="mean", embed_dim=24, prefix_attention="causal", token_budget=1)(prompts)
    two = _runner(model, embed_pooling="mean", embed_dim=24, prefix_attention="causal", token_budget=1)
    from flexible_llm_sharding_amd.api import run_all
    from flexible_llm_sharding_amd.parallel.comm import Comm
    got = run_all(SimpleNamespace(data_parallel=False, num_batch=2), two, Comm(0, 1), prompts)
    assert len(got) == len(one) and all(np.array_equal(a, b) for a, b in zip(got, one))


def test_headless_directory(model, tmp_path):
    """A model directory without lm_head.safetensors: embed mode loads and runs it (through
    main.py too, with both weight caches), the other modes refuse it as before."""
    d, cfg, tok, sd, prompts = model
    hd = str(tmp_path / "headless")
    shutil.copytree(d, hd)
    os.remove(os.path.join(hd, "lm_head.safetensors"))
    want = _runner(model, embed_pooling="mean")(prompts)
    r = ShardedRunner(cfg, FileLayerSource(cfg, hd, names=layer_names(cfg, "embed")), "cpu", tok, score_mode="embed",
                      embed_pooling="mean")
    assert all(np.array_equal(a, b) for a, b in zip(r(prompts), want))
    for cache in ("host", "stream"):
        p, out, mj = _main(tmp_path, hd, prompts, "--embed_pooling", "mean", "--weight_cache", cache)
        assert p.returncode == 0, p.stderr[-3000:]
        got = pickle.load(open(out, "rb"))["embeddings"]
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
    with pytest.raises(FileNotFoundError, match="missing layer files"):
        FileLayerSource(cfg, hd)
    from flexible_llm_sharding_amd.api import build_runner
    from flexible_llm_sharding_amd.parallel.comm import Comm
    base = ["--prompt_pickle", "p", "--output_file", "o", "--model_path", hd]
    for mode in ("next_token", "loglik"):
        with pytest.raises(FileNotFoundError, match="missing layer files"):
            build_runner(parse_args(base + ["--score_mode", mode]), cfg, "cpu", Comm(0, 1), tok)
    build_runner(parse_args(base + ["--score_mode", "embed"]), cfg, "cpu", Comm(0, 1), tok).close()


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, path, prompts, out_dir):
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    torch.set_num_threads(1)
    from flexible_llm_sharding_amd.api import run_all
    from flexible_llm_sharding_amd.config import ModelConfig
    from flexible_llm_sharding_amd.parallel.comm import Comm
    comm = Comm.from_env("cpu", timeout_s=120)
    cfg = ModelConfig.from_pretrained(path)
    tok = load_tokenizer(path)
    # one prompt per micro-batch on every rank and on the single rank: the same GEMM shapes
    kw = dict(token_budget=1, score_mode="embed", embed_pooling="mean", embed_dim=24)
    names = layer_names(cfg, "embed")
    r = ShardedRunner(cfg, FileLayerSource(cfg, path, names=names), "cpu", tok, comm=comm, data_parallel=True, **kw)
    got = run_all(SimpleNamespace(data_parallel=True, num_batch=1), r, comm, prompts)
    if rank == 0:
        want = ShardedRunner(cfg, FileLayerSource(cfg, path, names=names), "cpu", tok, **kw)(prompts)
        with open(os.path.join(out_dir, "dp.pkl"), "wb") as f:
            pickle.dump((got, want), f)
    else:
        assert got == []
    comm.destroy()


def test_data_parallel_equals_one_rank(model, tmp_path):
    """Two gloo ranks, each embedding its slice; rank 0 gathers the float32 arrays as objects:
    exactly the one-rank result, in prompt order."""
    d, cfg, tok, sd, prompts = model
    mp.start_processes(_dp_worker, args=(2, _port(), d, list(prompts), str(tmp_path)), nprocs=2, start_method="spawn",
                       join=True)
    got, want = pickle.load(open(tmp_path / "dp.pkl", "rb"))
    assert len(got) == len(want) == len(prompts)
    for a, b, (_, lens) in zip(got, want, SHAPES):
        assert a.dtype == np.float32 and a.shape == (len(lens), 24) and np.array_equal(a, b)


# ------------------------------------------------------------------ the converter
def test_converter_adds_the_model_prefix(tmp_path):
    """An ``AutoModel.save_pretrained`` checkpoint (embed_tokens.weight, layers.N.*, norm.weight; no
    head, untied): its layer files are byte for byte those of the prefixed twin, there is no head
    file, and the result runs in embed mode."""
    assert layer_of_param("layers.0.self_attn.q_proj.weight") == "model.layers.0"
    assert layer_of_param("embed_tokens.weight") == "model.embed_tokens" and layer_of_param("norm.weight") == "model.norm"
    assert layer_of_param("model.layers.3.mlp.up_proj.weight") == "model.layers.3" and layer_of_param("lm_head.weight") == "lm_head"
    cfg = preset("tiny")
    sd = {}
    for n in layer_names(cfg, "embed"):
        sd.update(synthetic_layer_state_dict(cfg, n, seed=2))
    outs = {}
    for kind in ("prefixed", "bare"):
        src = tmp_path / f"src_{kind}"
        src.mkdir()
        cfg.save(str(src))
        write_synthetic_tokenizer(str(src), cfg.vocab_size)
        save_file({(k[len("model."):] if kind == "bare" else k): v for k, v in sd.items()}, str(src / "model.safetensors"))
        outs[kind] = tmp_path / f"layers_{kind}"
        written = split_into_layers(str(src), str(outs[kind]), verbose=False)
        assert sorted(written) == sorted(layer_names(cfg, "embed"))
        assert not (outs[kind] / "lm_head.safetensors").exists()
    for n in layer_names(cfg, "embed"):
        a, b = (open(outs[k] / f"{n}.safetensors", "rb").read() for k in ("prefixed", "bare"))
        assert a == b, n
        assert all(layer_of_param(k) == n and torch.equal(v, sd[k])
                   for k, v in load_file(str(outs["bare"] / f"{n}.safetensors")).items())
    tok = load_tokenizer(str(outs["bare"]))
    r = ShardedRunner(cfg, FileLayerSource(cfg, str(outs["bare"]), names=layer_names(cfg, "embed")), "cpu", tok,
                      score_mode="embed")
    out = r([("wd we wf", ("wg wh", "wi"))])
    assert out[0].shape == (2, cfg.hidden_size) and np.isfinite(out[0]).all()
