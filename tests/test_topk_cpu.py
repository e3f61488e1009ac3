"""Compact next-token scores without a GPU: the host implementation against the oracle of
tests/topk_ref.py, the torch backend through the engine, the command-line flag and its refusals,
and runs of ``main.py`` (one rank, two batches, two gloo ranks data and model parallel) against
the same run without the flag."""
import argparse
import json
import os
import pickle
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topk_ref as tr  # noqa: E402

from flexible_llm_sharding_amd import topk  # noqa: E402
from flexible_llm_sharding_amd.utils.cli import check_top_k, parse_args  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = tr.kernel_cases()
CPU = torch.device("cpu")


# ------------------------------------------------------------------ the host implementation
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_host_topk_equals_oracle(case):
    ids, vals = topk.topk_rows(case.scores, case.K)
    wi, wv = case.want()
    assert ids.dtype == np.int32 and vals.dtype == np.uint16
    assert np.array_equal(ids, wi) and np.array_equal(vals, wv), case.name
    if case.picked is not None:
        assert np.array_equal(topk.picked_keys(case.scores, case.picked), case.want_picked()), case.name


def test_torch_backend_topk_rows_equals_oracle():
    from flexible_llm_sharding_amd.ops import get_ops
    ops = get_ops(CPU)
    for case in [c for c in CASES if c.V <= 2056][:6]:
        picked = None if case.picked is None else torch.from_numpy(case.picked)
        ids, vals, pv = ops.topk_rows(torch.from_numpy(case.scores), case.K, picked=picked)
        wi, wv = case.want()
        assert ids.dtype == torch.int32 and vals.dtype == torch.float16
        assert np.array_equal(ids.numpy(), wi) and np.array_equal(vals.numpy().view(np.uint16), wv), case.name
        if picked is None:
            assert pv is None
        else:
            assert np.array_equal(pv.numpy().view(np.uint16), case.want_picked())
    x = torch.zeros(2, 8, dtype=torch.float16)
    for K in (0, 9, -1):
        with pytest.raises(ValueError):
            ops.topk_rows(x, K)
    with pytest.raises(TypeError):
        ops.topk_rows(x, 2, picked=torch.zeros(3, dtype=torch.int32))


def test_host_topk_checks_its_arguments():
    s = np.zeros((2, 8), dtype=np.float16)
    with pytest.raises(TypeError):
        topk.topk_rows(s.astype(np.float32), 2)
    with pytest.raises(TypeError):
        topk.topk_rows(s[0], 2)
    for K in (0, 9, -3, 1.5):
        with pytest.raises(ValueError):
            topk.topk_rows(s, K)
    with pytest.raises(ValueError):
        topk.topk_rows(np.zeros((1, 2048), dtype=np.float16), 1025)
    with pytest.raises(ValueError):
        topk.picked_keys(s, np.zeros(3, dtype=np.int32))
    ids, vals = topk.topk_rows(s, 8)
    assert ids.tolist() == [list(range(8))] * 2 and not vals.any()
    packed = topk.pack(ids, vals)
    assert packed.dtype == topk.TOPK_DTYPE == np.dtype([("id", "<i4"), ("p", "<f2")]) and packed.shape == (2, 8)


# ------------------------------------------------------------------ flags
BASE = ["--prompt_pickle", "p", "--output_file", "o"]


def test_cli_parses_the_flag():
    assert parse_args(BASE).score_top_k == 0
    assert parse_args(BASE + ["--score_top_k", "20", "--num_gen_token", "3"]).score_top_k == 20
    assert parse_args(BASE + ["--score_top_k", "1024"]).score_top_k == 1024
    # one rank, one batch: the device draws from the full row, the combination works
    a = parse_args(BASE + ["--score_top_k", "5", "--do_sample", "--top_k", "40"])
    assert (a.score_top_k, a.do_sample) == (5, True)


@pytest.mark.parametrize("extra", [["--score_top_k", "-1"], ["--score_top_k", "1025"],
                                   ["--score_top_k", "5", "--score_mode", "loglik"],
                                   ["--score_top_k", "5", "--do_sample", "--num_batch", "2"]])
def test_cli_refuses(extra):
    with pytest.raises(ValueError, match="--score_top_k"):
        parse_args(BASE + extra)


def test_sampling_on_several_ranks_is_refused():
    args = argparse.Namespace(score_top_k=5, do_sample=True, num_batch=1, score_mode="next_token")
    check_top_k(args, 1)
    with pytest.raises(ValueError, match="--score_top_k"):
        check_top_k(args, 2)
    check_top_k(argparse.Namespace(score_top_k=5, do_sample=False, num_batch=2), 2)


def test_runner_refuses(tiny_model):
    from flexible_llm_sharding_amd.engine import ShardedRunner
    from flexible_llm_sharding_amd.runtime.stream import FileLayerSource
    path, cfg = tiny_model
    for kw in ({"score_top_k": cfg.vocab_size + 1}, {"score_top_k": -1}, {"score_top_k": 1025},
               {"score_top_k": 5, "score_mode": "loglik"}):
        with pytest.raises(ValueError, match="--score_top_k"):
            ShardedRunner(cfg, FileLayerSource(cfg, path), "cpu", None, **kw)


# ------------------------------------------------------------------ the engine on the torch backend
@pytest.fixture(scope="module")
def setup(tiny_model):
    return tr.engine_setup(tiny_model)


_FULL = {}


def _full(setup, name, **kw):
    if name not in _FULL:
        _FULL[name] = tr.generate(setup, CPU, **kw)
    return _FULL[name]


@pytest.mark.parametrize("K", [1, 20])
def test_engine_compact_scores_equal_oracle_on_full_scores(setup, K):
    full = _full(setup, "gen", num_gen=3)
    got = tr.generate(setup, CPU, top_k=K, num_gen=3)
    tr.check_compact_run(full, got, K)
    rows = sum(len(p[1]) for p in setup[2])
    assert all(b == rows * (6 * K + 6) for b in got.d2h), got.d2h


def test_engine_scoring_pass_and_streamed_weights(setup):
    """One scoring pass, and a generation whose weights are not resident (the pass through
    ``Outputs.start`` on the D2H stream)."""
    tr.check_compact_run(_full(setup, "score", num_gen=1), tr.generate(setup, CPU, top_k=20, num_gen=1), 20)
    kw = dict(num_gen=2, resident=False, prefix_kv_cache=False, suffix_kv_cache=False)
    tr.check_compact_run(_full(setup, "streamed", **kw), tr.generate(setup, CPU, top_k=5, **kw), 5)


def test_engine_sampled_tokens_equal_the_sampled_run(setup):
    sp = dict(temperature=0.8, top_k=50, top_p=0.95, seed=5)
    full = _full(setup, "sampled", num_gen=3, sampling=sp)
    got = tr.generate(setup, CPU, top_k=20, num_gen=3, sampling=sp)
    tr.check_compact_run(full, got, 20)
    assert any((o["id"][:, :, 0] != t).any() for o, t in zip(got.scores, got.record["token_ids"]))


def test_num_batch_two_gives_the_one_batch_result(setup):
    """Two batches: the runner's own tokens cover the last batch only, so the greedy token and its
    probability come from the first ranked entry."""
    full = _full(setup, "gen", num_gen=3)
    got = tr.generate(setup, CPU, top_k=20, num_gen=3, num_batch=2)
    tr.check_compact_run(full, got, 20, per_call_tokens=False)
    one = tr.generate(setup, CPU, top_k=20, num_gen=3)
    for a, b in zip(got.scores, one.scores):
        assert np.array_equal(a, b)
    for key in ("token_ids", "token_probs"):
        assert all(np.array_equal(a, b) for a, b in zip(got.record[key], one.record[key]))


# ------------------------------------------------------------------ main.py
NUM_GEN = 3
K_MAIN = 7


def _prompts(cfg):
    from flexible_llm_sharding_amd.utils.synthetic import synthetic_prompts
    return synthetic_prompts(5, 15, 3, 4, cfg.vocab_size, seed=4, vary=True)


def _argv(path, pp, out, extra=()):
    return ["--model_path", path, "--prompt_pickle", str(pp), "--output_file", str(out), "--num_gen_token",
            str(NUM_GEN), "--num_gpus", "0"] + list(extra)


def _env():
    return dict(os.environ, PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="1")


@pytest.fixture(scope="module")
def main_full(tiny_model, tmp_path_factory):
    """main.py without the flag, in process: (prompts, prompt file, scores, bytes of _updated.pkl)."""
    from flexible_llm_sharding_amd.api import main
    path, cfg = tiny_model
    d = tmp_path_factory.mktemp("topk_main")
    prompts = _prompts(cfg)
    pp, out = d / "prompts.pkl", d / "full.pkl"
    pickle.dump(prompts, open(pp, "wb"))
    assert main(_argv(path, pp, out)) == 0
    return prompts, pp, pickle.load(open(out, "rb")), open(d / "prompts_updated.pkl", "rb").read(), d


def _check_file(prompts, full_scores, got, K=K_MAIN):
    assert set(got) == {"k", "top_ids", "top_probs", "token_ids", "token_probs"} and got["k"] == K
    assert all(len(got[k]) == len(prompts) for k in ("top_ids", "top_probs", "token_ids", "token_probs"))
    for p, ((_, sufs), f) in enumerate(zip(prompts, full_scores)):
        n_s = len(sufs)
        ti, tp, ki, kp = got["top_ids"][p], got["top_probs"][p], got["token_ids"][p], got["token_probs"][p]
        assert ti.dtype == np.int32 and ti.shape == (n_s, NUM_GEN, K)
        assert tp.dtype == np.float16 and tp.shape == (n_s, NUM_GEN, K)
        assert ki.dtype == np.int64 and ki.shape == (n_s, NUM_GEN)
        assert kp.dtype == np.float16 and kp.shape == (n_s, NUM_GEN)
        for t in range(NUM_GEN):
            ids, vals = tr.ref_topk(f[:, t, :], K)
            assert np.array_equal(ti[:, t], ids) and np.array_equal(tp[:, t].view(np.uint16), vals), (p, t)
            assert np.array_equal(ki[:, t], np.argmax(f[:, t, :].view(np.uint16), axis=-1)), (p, t)
            assert np.array_equal(kp[:, t].view(np.uint16), tr.ref_picked(f[:, t, :], ki[:, t])), (p, t)


def test_main_writes_the_compact_file(tiny_model, main_full):
    """In process, one rank: keys, dtypes and shapes as documented, every entry the oracle on the
    full run's scores; ``_updated.pkl`` byte-equal; ``--metrics_json`` holds the flag."""
    from flexible_llm_sharding_amd.api import main
    path, cfg = tiny_model
    prompts, pp, full, updated, d = main_full
    out, mj = d / "compact.pkl", d / "m.json"
    assert main(_argv(path, pp, out, ["--score_top_k", str(K_MAIN), "--metrics_json", str(mj)])) == 0
    _check_file(prompts, full, pickle.load(open(out, "rb")))
    assert open(d / "prompts_updated.pkl", "rb").read() == updated
    assert json.load(open(mj))["score_top_k"] == K_MAIN


def test_main_two_batches(tiny_model, main_full):
    from flexible_llm_sharding_amd.api import main
    path, cfg = tiny_model
    prompts, pp, full, updated, d = main_full
    out = d / "compact_b2.pkl"
    assert main(_argv(path, pp, out, ["--score_top_k", str(K_MAIN), "--num_batch", "2"])) == 0
    _check_file(prompts, full, pickle.load(open(out, "rb")))
    assert open(d / "prompts_updated.pkl", "rb").read() == updated


@pytest.mark.parametrize("mode", ["data_parallel", "model_parallel"])
def test_main_two_ranks_give_the_one_rank_result(tiny_model, main_full, tmp_path, mode):
    """Two gloo ranks: the structured arrays travel by gather_object (data parallel: every rank's
    prompts; model parallel: the rank owning lm_head supplies them)."""
    path, cfg = tiny_model
    prompts, _, full, updated, _ = main_full
    pp, out = tmp_path / "prompts.pkl", tmp_path / "out.pkl"
    pickle.dump(prompts, open(pp, "wb"))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    extra = ["--score_top_k", str(K_MAIN)] + (["--data_parallel"] if mode == "data_parallel" else [])
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "main.py")] + _argv(path, pp, out, extra)
    r = subprocess.run(cmd, cwd=str(tmp_path), env=_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    _check_file(prompts, full, pickle.load(open(out, "rb")))
    got = pickle.load(open(tmp_path / "prompts_updated.pkl", "rb"))
    assert [tuple(u) for u in got] == [tuple(u) for u in pickle.loads(updated)]
