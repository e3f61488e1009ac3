"""Continuation log-likelihood scoring (``score_mode="loglik"``) on the CPU backend: packing,
the engine against ``reference_logliks`` and HF transformers, consistency with the next-token
mode, refused combinations, the CLI and data parallel.

Tolerances are the probability tolerances of tests/test_engine_cpu.py (1e-4 against the oracle,
2e-3 against HF) carried to logs as ``atol_p / p_min`` (to first order d log p = dp / p), with
``p_min`` the smallest oracle target probability of the case, computed in the test.  The model is
written with std = 0.15 and the suffix tokens are ones the oracle finds likely
(tests/loglik_ref.py ``likely_prompts``): p_min ~ 0.02-0.03, tolerance ~ 4e-3, per-token spread
of the oracle 2.5-3.3 (>= 20 x the tolerance, asserted)."""
import os
import pickle
import socket
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loglik_ref as lr  # noqa: E402

from flexible_llm_sharding_amd.config import preset  # noqa: E402
from flexible_llm_sharding_amd.engine import ShardedRunner  # noqa: E402
from flexible_llm_sharding_amd.models.reference import reference_logliks  # noqa: E402
from flexible_llm_sharding_amd.runtime.batch import pack_prompts  # noqa: E402
from flexible_llm_sharding_amd.runtime.stream import FileLayerSource  # noqa: E402
from flexible_llm_sharding_amd.utils.cli import parse_args  # noqa: E402
from flexible_llm_sharding_amd.utils.synthetic import load_full_state_dict, write_synthetic_checkpoint  # noqa: E402
from flexible_llm_sharding_amd.utils.tokenizer import TokenizedPrompt, load_tokenizer, tokenize_prompts  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL_P_ORACLE = 1e-4      # tests/test_engine_cpu.py::test_engine_matches_oracle
ATOL_P_HF = 2e-3          # tests/test_engine_cpu.py::test_causal_prefix_matches_hf_transformers
SHAPES = [(20, [1, 2, 9]), (12, [5, 3, 4]), (30, [7]), (9, [6, 2])]


# ------------------------------------------------------------------ packing
def _tp(prefix, suffixes):
    return TokenizedPrompt(list(prefix), [list(s) for s in suffixes], max(len(s) for s in suffixes),
                           [len(s) - 1 for s in suffixes])


def test_pack_loglik_pairs_by_hand():
    """Two prompts; suffix lengths 1, 2 and 65; the second prompt has a single suffix."""
    long = list(range(100, 165))
    a = _tp([1, 5, 6], [[7], [8, 9], long])          # rows 0-2 prefix, 3 | 4 5 | 6..70
    b = _tp([1, 4], [[11, 12, 13]])                  # rows 71-72 prefix, 73 74 75
    p = pack_prompts([a, b], [0, 1], "bidirectional", loglik=True)
    assert p.num_tokens == 76
    want_rows = [2] + [2, 4] + [2] + list(range(6, 70)) + [72, 73, 74]
    want_tgt = [7] + [8, 9] + long + [11, 12, 13]
    assert p.last_idx.tolist() == want_rows and p.last_idx.dtype == np.int32
    assert p.targets.tolist() == want_tgt and p.targets.dtype == np.int32
    assert p.n_scored == 1 + 2 + 65 + 3
    assert p.prompt_scored.tolist() == [[0, 68], [68, 71]]
    # the last row of each suffix scores nothing
    assert not {3, 5, 70, 75} & set(p.last_idx.tolist())
    meta = p.device_tensors("cpu")
    assert meta["targets"].tolist() == want_tgt and meta["last_pos"].tolist() == p.positions[p.last_idx].tolist()
    assert "targets" in p.host_meta()
    # prompt-aligned attention groups carry each prompt's pairs, group-relative
    g = p.attn_groups(10)
    assert [x["last_local"].tolist() for x in g] == [want_rows[:68], [1, 2, 3]]


def test_pack_default_is_unchanged():
    a = _tp([1, 5, 6], [[7], [8, 9], list(range(100, 165))])
    b = _tp([1, 4], [[11, 12, 13]])
    for kw in ({}, {"window": 4}):
        x = pack_prompts([a, b], [0, 1], "causal", **kw)
        y = pack_prompts([a, b], [0, 1], "causal", loglik=False, **kw)
        assert x.targets is None and y.targets is None and "targets" not in y.host_meta()
        for f in ("ids", "positions", "work", "seg_lo", "last_idx", "work_last", "prompt_rows", "prompt_items",
                  "prompt_scored", "r0_lo", "r0_item", "r0_item_last"):
            u, v = getattr(x, f), getattr(y, f)
            assert (u is None and v is None) or (u.dtype == v.dtype and np.array_equal(u, v)), f
        assert x.segments == y.segments and x.last_segments == y.last_segments
        # and everything but the scored-pair arrays is the same with loglik=True
        z = pack_prompts([a, b], [0, 1], "causal", loglik=True, **kw)
        for f in ("ids", "positions", "work", "seg_lo", "prompt_rows", "prompt_items", "r0_lo", "r0_item"):
            u, v = getattr(x, f), getattr(z, f)
            assert (u is None and v is None) or np.array_equal(u, v), f


def test_pack_loglik_refusals():
    a = _tp([1, 5, 6], [[7], [8, 9]])
    with pytest.raises(ValueError, match="kv_cached"):
        pack_prompts([a], [0], loglik=True, prefix_offsets=[0], kv_cached=True)
    with pytest.raises(ValueError, match="suffix_keep"):
        pack_prompts([a], [0], loglik=True, prefix_offsets=[0], kv_cached=True, suffix_rows=[[0, 64]],
                     suffix_keep=[[0, 1]])
    with pytest.raises(ValueError, match="no token"):
        pack_prompts([TokenizedPrompt([1, 2], [[7], []], 1, [0, -1])], [0], loglik=True)


def test_kernel_cases_cover_the_edges_and_discriminate():
    """The kernel cases of tests/test_loglik_gpu.py, checked where no GPU is needed: every edge
    column (by formula) is some row's spike and some row's target; no row excluded, leaving a
    row's spike column out of its logsumexp moves lp by >= 4 tau; tau > 0 in every group."""
    cases = lr.kernel_cases()
    tau = lr.group_tau(cases)
    sp, tg = set(), set()
    for c in cases:
        for r in range(len(c.targets)):
            sp.update(lr.edge_kinds(c.V, int(c.spikes[r])))
            tg.update(lr.edge_kinds(c.V, int(c.targets[r])))
        assert tau[c.group] > 0
        assert c.spike_effect().min() >= lr.SEPARATION * tau[c.group], (c.name, c.spike_effect().min(), tau)
    assert sp == set(range(8)) and tg == set(range(8)), (sp, tg)
    assert {(c.V, c.vec) for c in cases} >= {(8, True), (1000, True), (2056, True), (32000, True), (32003, False),
                                             (151936, True), (2056, False)}


def test_memory_plan_charges_the_norm_state():
    """plan_for_vram(scored_rows=n): the final norm's [n, H] state on top of the hidden states."""
    from flexible_llm_sharding_amd.runtime.memplan import SLACK, plan_for_vram
    cfg = preset("llama2-7b", num_hidden_layers=4)
    kw = dict(total_tokens=16128, max_prompt_rows=1344, overhead=int(0.9e9), fused_norm=True)
    base = plan_for_vram(cfg, int(6e9), **kw)
    same = plan_for_vram(cfg, int(6e9), scored_rows=0, **kw)
    more = plan_for_vram(cfg, int(6e9), scored_rows=3840, **kw)
    assert base == same
    assert more[:4] == base[:4] and more[4] - base[4] == int(SLACK * 2 * 3840 * cfg.hidden_size)
    # a tight cap: the charge shrinks the plan instead of overshooting it
    tight = base[4] + 1000
    small = plan_for_vram(cfg, int(tight / (1 - 0.012)) + 1, scored_rows=3840, **kw)
    assert small[4] <= tight and small[:4] != base[:4]


# ------------------------------------------------------------------ engine vs the oracle
@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("loglik_model"))
    cfg = preset("tiny")
    write_synthetic_checkpoint(cfg, d, seed=1, std=0.15)
    return d, cfg, load_tokenizer(d), load_full_state_dict(cfg, d)


_CASES = {}


def _case(model, mode):
    """Prompts built for ``mode`` with the oracle alone, their targets, the oracle's [L, V] rows and
    per-token lp (computed once per mode, shared, never modified)."""
    if mode not in _CASES:
        d, cfg, tok, sd = model
        prompts = lr.likely_prompts(cfg, sd, tok, mode, SHAPES, seed=3)
        targets = [tp.suffixes for tp in tokenize_prompts(tok, prompts, 4096)]
        assert [[len(u) for u in t] for t in targets] == [lens for _, lens in SHAPES]
        dists = reference_logliks(cfg, sd, tok, prompts, mode, dists=True)
        ref = reference_logliks(cfg, sd, tok, prompts, mode)
        for dp, rp, tp in zip(dists, ref, targets):
            for dd, rr, u in zip(dp, rp, tp):
                assert rr.dtype == np.float64 and np.array_equal(rr, dd[np.arange(len(u)), u])
        _CASES[mode] = (prompts, targets, dists, ref)
    return _CASES[mode]


def _flat(per_prompt):
    return np.concatenate([np.asarray(x, dtype=np.float64) for p in per_prompt for x in p])


def _tol(ref, atol_p):
    """atol_p / p_min, and the check that the oracle's per-token spread is >= 20 x that."""
    lp = _flat(ref)
    tol = atol_p / float(np.exp(lp.min()))
    return tol, float(lp.max() - lp.min())


def _check(out, runner, ref, targets, tol):
    for o, per, rp, tp in zip(out, runner.last_token_logprobs, ref, targets):
        assert o.shape == (len(tp), 3) and o.dtype == np.float32
        assert len(per) == len(tp)
        for s, (lp, rf, u) in enumerate(zip(per, rp, tp)):
            assert lp.dtype == np.float32 and lp.shape == (len(u),)
            assert np.abs(lp - rf).max() <= tol, (np.abs(lp - rf).max(), tol)
            assert o[s, 0] == np.float32(lp.astype(np.float64).sum()) and o[s, 1] == len(u)


@pytest.mark.parametrize("mode,lnps,storage,budget,head_chunk",
                         [(m, l, s, 100000, 0) for m in ("bidirectional", "causal") for l in (1, 3)
                          for s in ("cpu", "disk")]
                         + [("causal", 1, "cpu", 40, 0), ("bidirectional", 2, "cpu", 100000, 5)])
def test_engine_loglik_matches_oracle(model, tmp_path, mode, lnps, storage, budget, head_chunk):
    d, cfg, tok, sd = model
    prompts, targets, dists, ref = _case(model, mode)
    tol, spread = _tol(ref, ATOL_P_ORACLE)
    assert spread >= 20 * tol, (spread, tol)
    r = ShardedRunner(cfg, FileLayerSource(cfg, d), "cpu", tok, layer_num_per_shard=lnps, storage_location=storage,
                      disk_folder=str(tmp_path), token_budget=budget, prefix_attention=mode, score_mode="loglik")
    r.ctx.head_chunk = head_chunk
    out = r(prompts)
    assert r.stats["micro_batches"] >= (2 if budget == 40 else 1)
    n_pairs = sum(len(u) for t in targets for u in t)
    assert head_chunk < n_pairs
    _check(out, r, ref, targets, tol)
    # the greedy flag: every target the oracle's clear argmax <=> all-greedy
    for o, dp, tp in zip(out, dists, targets):
        for s, (dd, u) in enumerate(zip(dp, tp)):
            top2 = np.sort(dd, axis=1)[:, -2:]
            if (top2[:, 1] - top2[:, 0] > 10 * tol).all():           # no near-ties: the flag is decided
                assert o[s, 2] == float((dd.argmax(1) == np.asarray(u)).all())
    # discrimination, from the oracle alone: targets taken one position late
    sums = np.asarray([x.sum() for rp in ref for x in rp])
    moved = np.abs(np.concatenate(lr.shifted_sums(dists, targets)) - sums) >= lr.SEPARATION * tol
    assert moved.mean() >= 0.9, moved
    # a second call starts clean
    out2 = r(prompts)
    assert all(np.array_equal(a, b) for a, b in zip(out, out2))


def test_loglik_matches_hf_transformers(model):
    """prefix_attention="causal": per-token lp == log_softmax of HF LlamaForCausalLM logits on the
    prefix + suffix ids, gathered at the targets (the standard causal-LM log-likelihood)."""
    transformers = pytest.importorskip("transformers")
    d, cfg, tok, sd = model
    prompts, targets, dists, ref = _case(model, "causal")
    hf_cfg = transformers.LlamaConfig(
        hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
        num_attention_heads=cfg.num_attention_heads, num_key_value_heads=cfg.num_key_value_heads,
        num_hidden_layers=cfg.num_hidden_layers, vocab_size=cfg.vocab_size, rms_norm_eps=cfg.rms_norm_eps,
        rope_theta=cfg.rope_theta, max_position_embeddings=cfg.max_position_embeddings,
        tie_word_embeddings=False)
    hf = transformers.LlamaForCausalLM(hf_cfg).float().eval()
    hf.load_state_dict({k: v.float() for k, v in sd.items()}, strict=False)
    r = ShardedRunner(cfg, FileLayerSource(cfg, d), "cpu", tok, prefix_attention="causal", score_mode="loglik")
    r(prompts)
    tps = tokenize_prompts(tok, prompts, 4096)
    want = []
    for tp in tps:
        per = []
        for u in tp.suffixes:
            ids = torch.tensor([tp.prefix + u])
            with torch.no_grad():
                lsm = torch.log_softmax(hf(ids).logits[0].double(), -1)
            Lp = len(tp.prefix)
            per.append(lsm[torch.arange(Lp - 1, Lp - 1 + len(u)), torch.tensor(u)].numpy())
        want.append(per)
    tol = ATOL_P_HF / float(np.exp(_flat(want).min()))
    err = np.abs(_flat(r.last_token_logprobs) - _flat(want)).max()
    assert err <= tol, (err, tol)


def test_loglik_agrees_with_next_token_mode(model):
    """For a suffix u, the next-token mode on the suffixes u[:1] .. u[:L-1] returns the fp16
    probability of u[t] after u[:t]; its log agrees with loglik's lp[t], t >= 1, within 2^-10 (the
    fp16 rounding of the returned probability, <= 2^-11 relative) + the engine tolerance.  Targets
    have probability >= 2^-14 (normal fp16)."""
    d, cfg, tok, sd = model
    prompts, targets, dists, ref = _case(model, "bidirectional")
    tol, _ = _tol(ref, ATOL_P_ORACLE)
    assert np.exp(_flat(ref).min()) >= 2.0 ** -14
    ll = ShardedRunner(cfg, FileLayerSource(cfg, d), "cpu", tok, score_mode="loglik")
    ll(prompts)
    nt = ShardedRunner(cfg, FileLayerSource(cfg, d), "cpu", tok)
    checked = 0
    for pi, ((prefix, sufs), tp) in enumerate(zip(prompts, targets)):
        for si, (s, u) in enumerate(zip(sufs, tp)):
            words = s.split()
            if len(u) < 2:
                continue
            scores = nt([(prefix, tuple(" ".join(words[:t]) for t in range(1, len(u))))])[0]
            for t in range(1, len(u)):
                p = float(scores[t - 1, 0, u[t]])
                assert abs(np.log(p) - float(ll.last_token_logprobs[pi][si][t])) <= 2.0 ** -10 + tol
                checked += 1
    assert checked == sum(len(u) - 1 for t in targets for u in t)


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("kw,flag", [({"hip_graphs": True}, "--hip_graphs"),
                                     ({"prefix_kv_cache": True}, "--prefix_kv_cache"),
                                     ({"suffix_kv_cache": True}, "--suffix_kv_cache"),
                                     ({"resume_dir": "ck"}, "--resume_dir")])
def test_runner_refuses(model, kw, flag):
    d, cfg, tok, sd = model
    with pytest.raises(ValueError, match=flag):
        ShardedRunner(cfg, FileLayerSource(cfg, d), "cpu", tok, score_mode="loglik", **kw)
    ShardedRunner(cfg, FileLayerSource(cfg, d), "cpu", tok, **kw).close()       # the default mode takes it


def test_runner_refuses_model_parallel_and_bad_mode(model):
    from flexible_llm_sharding_amd.parallel.comm import Comm
    d, cfg, tok, sd = model
    with pytest.raises(ValueError, match="model parallel"):
        ShardedRunner(cfg, FileLayerSource(cfg, d), "cpu", tok, score_mode="loglik", comm=Comm(0, 2))
    with pytest.raises(ValueError, match="score_mode"):
        ShardedRunner(cfg, FileLayerSource(cfg, d), "cpu", tok, score_mode="sum")


@pytest.mark.parametrize("extra,flag", [(["--num_gen_token", "2"], "--num_gen_token"),
                                        (["--hip_graphs"], "--hip_graphs"),
                                        (["--prefix_kv_cache", "true"], "--prefix_kv_cache"),
                                        (["--suffix_kv_cache", "true"], "--suffix_kv_cache"),
                                        (["--resume_dir", "ck"], "--resume_dir")])
def test_cli_refuses(extra, flag):
    base = ["--prompt_pickle", "p", "--output_file", "o"]
    with pytest.raises(ValueError, match=flag):
        parse_args(base + ["--score_mode", "loglik"] + extra)
    assert parse_args(base + extra).score_mode == "next_token"
    a = parse_args(base + ["--score_mode", "loglik"])          # the auto K/V caches resolve to off
    from flexible_llm_sharding_amd.api import resolve_prefix_kv_cache, resolve_suffix_kv_cache
    assert a.score_mode == "loglik" and not resolve_prefix_kv_cache(a) and not resolve_suffix_kv_cache(a)


def test_build_runner_refuses_model_parallel(model):
    from flexible_llm_sharding_amd.api import build_runner
    from flexible_llm_sharding_amd.parallel.comm import Comm
    d, cfg, tok, sd = model
    a = parse_args(["--prompt_pickle", "p", "--output_file", "o", "--score_mode", "loglik", "--model_path", d])
    with pytest.raises(ValueError, match="model parallel"):
        build_runner(a, cfg, "cpu", Comm(0, 2), tok)


def test_empty_suffix_raises(model):
    d, cfg, tok, sd = model
    r = ShardedRunner(cfg, FileLayerSource(cfg, d), "cpu", tok, score_mode="loglik")
    with pytest.raises(ValueError, match="no token"):
        r([("wd we wf", ("wg wh", ""))])
    with pytest.raises(ValueError, match="token id"):
        r.run_tokenized([TokenizedPrompt([1, 5], [[7, cfg.vocab_size]], 2, [1])])
    assert len(ShardedRunner(cfg, FileLayerSource(cfg, d), "cpu", tok)([("wd we wf", ("wg wh", ""))])) == 1


# ------------------------------------------------------------------ CLI and data parallel
def test_main_loglik_end_to_end(model, tmp_path):
    d, cfg, tok, sd = model
    prompts, targets, dists, ref = _case(model, "causal")
    pp = tmp_path / "prompts.pkl"
    pickle.dump(prompts, open(pp, "wb"))
    out = tmp_path / "scores.pkl"
    env = dict(os.environ, PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--model_path", d, "--prompt_pickle", str(pp),
                        "--output_file", str(out), "--score_mode", "loglik", "--prefix_attention", "causal",
                        "--num_batch", "2", "--disk_folder", str(tmp_path / "spill")],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    res = pickle.load(open(out, "rb"))
    tol, _ = _tol(ref, ATOL_P_ORACLE)
    assert len(res["scores"]) == len(res["token_logprobs"]) == len(prompts)
    for o, per, rp, tp in zip(res["scores"], res["token_logprobs"], ref, targets):
        assert o.shape == (len(tp), 3) and o.dtype == np.float32
        for s, (lp, rf) in enumerate(zip(per, rp)):
            assert lp.dtype == np.float32 and np.abs(lp - rf).max() <= tol
            assert o[s, 0] == np.float32(lp.astype(np.float64).sum()) and o[s, 1] == len(rf)
    assert pickle.load(open(tmp_path / "prompts_updated.pkl", "rb")) == list(prompts)


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
    kw = dict(token_budget=1, score_mode="loglik")
    r = ShardedRunner(cfg, FileLayerSource(cfg, path), "cpu", tok, comm=comm, data_parallel=True, **kw)
    args = SimpleNamespace(data_parallel=True, num_batch=1)
    got = run_all(args, r, comm, prompts)
    if rank == 0:
        one = ShardedRunner(cfg, FileLayerSource(cfg, path), "cpu", tok, **kw)
        want = one(prompts)
        with open(os.path.join(out_dir, "dp.pkl"), "wb") as f:
            pickle.dump((got, r.last_token_logprobs, want, one.last_token_logprobs), f)
    else:
        assert got == []
    comm.destroy()


def test_data_parallel_equals_one_rank(model, tmp_path):
    """Two gloo ranks, each scoring its slice; rank 0 gathers the [n_s, 3] arrays and the per-token
    values as objects: exactly the one-rank results (float32, not rounded to fp16 on the way)."""
    d, cfg, tok, sd = model
    prompts, targets, dists, ref = _case(model, "bidirectional")
    mp.start_processes(_dp_worker, args=(2, _port(), d, list(prompts), str(tmp_path)), nprocs=2, start_method="spawn",
                       join=True)
    got, got_tok, want, want_tok = pickle.load(open(tmp_path / "dp.pkl", "rb"))
    assert len(got) == len(want) == len(prompts)
    for a, b in zip(got, want):
        assert a.dtype == np.float32 and np.array_equal(a, b)
    for pa, pb in zip(got_tok, want_tok):
        assert len(pa) == len(pb) and all(x.dtype == np.float32 and np.array_equal(x, y) for x, y in zip(pa, pb))
