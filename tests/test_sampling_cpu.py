"""Sampled generation without a GPU: the host sampler against the oracle of
tests/sampling_ref.py, the weight table, the distribution of the draws, the command-line flags, and
runs of ``main.py`` replayed from their output file and the seed alone."""
import json
import os
import pickle
import socket
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_ref as sr  # noqa: E402

from flexible_llm_sharding_amd import sampling  # noqa: E402
from flexible_llm_sharding_amd.utils.cli import parse_args  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sr.kernel_cases()
_TABLES = {}


def _table(T):
    if T not in _TABLES:
        _TABLES[T] = sampling.weight_table(T)
    return _TABLES[T]


# ------------------------------------------------------------------ the host sampler
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_sample_tokens_equals_oracle(case):
    got = sampling.sample_tokens(case.scores, _table(case.T), case.top_k, case.P, case.draws)
    assert got.dtype == np.int64 and np.array_equal(got, case.want()), case.name


def test_top_k_one_and_p_one_are_argmax():
    n = 0
    for case in CASES:
        bits = case.scores.view(np.uint16)
        if (bits > sr.ONE).any():
            continue                          # (np.argmax would take a NaN or a value above 1)
        am = np.argmax(case.scores, axis=-1)
        # P = 1 alone keeps one token when the largest weight is >= 2^-16 of the row's sum (tau =
        # ceil(S_k / 65536)): every row here but the flat one wider than 65,536 columns
        w = sr.ref_weights(bits, case.T)
        one = w.max(axis=1) * np.uint64(65536) >= w.sum(axis=1, dtype=np.uint64)
        assert one.all() or case.name == "flat_V151936_T0.7", case.name
        # (T < 1 rounds the weight of the smallest subnormals to 0: such a row has nothing to draw)
        some = (w.max(axis=1) > 0) | (bits.max(axis=1) == 0)
        assert some.all() or case.name == "sparse_T0.7_p", case.name
        for k, P, rows in ((1, 65536, some), (0, 1, one & some), (1, 1, some)):
            assert np.array_equal(sampling.sample_tokens(case.scores, _table(case.T), k, P, case.draws)[rows], am[rows])
            assert np.array_equal(sr.ref_tokens(case.scores, case.T, k, P, case.draws)[rows], am[rows])
        n += case.family == "ties"
    assert n == 3                             # ties at the maximum included: the first index


def test_weight_table():
    t1 = sampling.weight_table(1.0)
    p = np.arange(0x3C01, dtype=np.uint16).view(np.float16).astype(np.float64)
    assert t1.dtype == np.uint32 and t1.shape == (0x3C01,)
    assert np.array_equal(t1.astype(np.float64), p * 2.0 ** 30)          # exact at T = 1
    for T in (0.5, 0.7, 1.5, 2.0):
        t = sampling.weight_table(T)
        assert t[0] == 0 and t[-1] == 1 << 30 and (np.diff(t.astype(np.int64)) >= 0).all(), T
        assert np.array_equal(t.astype(np.uint64), sr.ref_weights(np.arange(0x3C01, dtype=np.uint16), T))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="temperature"):
            sampling.weight_table(bad)
    assert [sampling.top_p_units(x) for x in (1.0, 0.5, 1e-9, 0.95)] == [65536, 32768, 1, sr.ref_P(0.95)]


def test_draws_follow_the_definition():
    d = sampling.draws(7, [3, 10], [2, 3], 5)
    want = [sr.ref_draw(7, 3, 0, 5), sr.ref_draw(7, 3, 1, 5), sr.ref_draw(7, 10, 0, 5), sr.ref_draw(7, 10, 1, 5),
            sr.ref_draw(7, 10, 2, 5)]
    assert d.dtype == np.uint64 and d.tolist() == want
    # splitmix64's published first outputs from state 0 (the generator adds its increment first)
    assert sampling.splitmix64(0) == 0xE220A8397B1DCDAF
    assert len({sr.ref_draw(0, p, s, t) for p in range(8) for s in range(8) for t in range(8)}) == 512


def test_distribution_chi_square():
    """8,192 draws from consecutive (p, s, t) keys on one V = 97 row, on the oracle alone (the
    sampler and the kernel inherit it through the equality tests).  Tokens whose expected count is
    >= 5 are compared; the others are left out, so the counts kept are not bound by a total and
    the statistic has one degree of freedom per token kept.  Bound: dof + 4 sqrt(2 dof), four
    standard deviations of a chi-square variable above its mean."""
    rng = np.random.default_rng(5)
    x = rng.standard_normal(97) * 1.5
    row = (np.exp(x) / np.exp(x).sum()).astype(np.float16)
    keys = [(p, s, t) for p in range(32) for s in range(16) for t in range(16)]
    assert len(keys) == 8192
    toks = np.asarray([sr.ref_token(row, 1.0, 0, 65536, sr.ref_draw(1234, p, s, t)) for p, s, t in keys])
    w = sr.ref_weights(row.view(np.uint16), 1.0).astype(np.float64)
    exp = w / w.sum() * len(keys)
    keep = exp >= 5
    obs = np.bincount(toks, minlength=97).astype(np.float64)
    chi2 = float(((obs[keep] - exp[keep]) ** 2 / exp[keep]).sum())
    dof = int(keep.sum())
    print(f"chi2 {chi2:.1f} at dof {dof}")
    assert dof >= 30 and chi2 <= dof + 4 * np.sqrt(2 * dof), (chi2, dof)


def test_sample_tokens_checks_its_arguments():
    s = np.zeros((2, 8), dtype=np.float16)
    d = np.zeros(2, dtype=np.uint64)
    with pytest.raises(TypeError):
        sampling.sample_tokens(s.astype(np.float32), _table(1.0), 0, 65536, d)
    with pytest.raises(ValueError):
        sampling.sample_tokens(s, _table(1.0), 0, 65536, d[:1])
    with pytest.raises(ValueError):
        sampling.sample_tokens(s, _table(1.0), 0, 0, d)
    with pytest.raises(ValueError, match="vocabular"):
        sampling.sample_tokens(np.zeros((1, 1 << 18), dtype=np.float16), _table(1.0), 0, 65536, d[:1])
    assert sampling.sample_tokens(s, _table(1.0), 0, 65536, d).tolist() == [0, 0]


# ------------------------------------------------------------------ flags
BASE = ["--prompt_pickle", "p", "--output_file", "o"]


def test_cli_parses_the_sampling_flags():
    a = parse_args(BASE)
    assert (a.do_sample, a.temperature, a.top_k, a.top_p, a.seed) == (False, 1.0, 0, 1.0, 0)
    assert sampling.SamplingParams.from_args(a) is None
    a = parse_args(BASE + ["--do_sample", "--temperature", "0.8", "--top_k", "50", "--top_p", "0.95", "--seed", "3",
                           "--num_gen_token", "1"])
    sp = sampling.SamplingParams.from_args(a)
    assert sp == sampling.SamplingParams(0.8, 50, 0.95, 3) and sp.P == sr.ref_P(0.95)
    assert sp.as_dict() == {"do_sample": True, "temperature": 0.8, "top_k": 50, "top_p": 0.95, "seed": 3}
    assert parse_args(BASE + ["--do_sample", "true"]).do_sample is True


@pytest.mark.parametrize("extra,flag", [(["--temperature", "0.8"], "--temperature"), (["--top_k", "5"], "--top_k"),
                                        (["--top_p", "0.9"], "--top_p"),
                                        (["--do_sample", "--score_mode", "loglik"], "--score_mode loglik"),
                                        (["--do_sample", "--temperature", "0"], "--temperature"),
                                        (["--do_sample", "--temperature", "-1"], "--temperature"),
                                        (["--do_sample", "--top_k", "-1"], "--top_k"),
                                        (["--do_sample", "--top_p", "0"], "--top_p"),
                                        (["--do_sample", "--top_p", "1.5"], "--top_p")])
def test_cli_refuses(extra, flag):
    with pytest.raises(ValueError, match=flag):
        parse_args(BASE + extra)


def test_runner_refuses_sampling_in_loglik(tiny_model):
    from flexible_llm_sharding_amd.engine import ShardedRunner
    from flexible_llm_sharding_amd.runtime.stream import FileLayerSource
    path, cfg = tiny_model
    with pytest.raises(ValueError, match="--do_sample"):
        ShardedRunner(cfg, FileLayerSource(cfg, path), "cpu", None, score_mode="loglik",
                      sampling=sampling.SamplingParams())


# ------------------------------------------------------------------ main.py, replayed
NUM_GEN = 3
FLAGS = {"temperature": 0.9, "top_k": 40, "top_p": 0.9}


def _prompts(cfg):
    from flexible_llm_sharding_amd.utils.synthetic import synthetic_prompts
    return synthetic_prompts(5, 15, 3, 4, cfg.vocab_size, seed=4, vary=True)


def _argv(path, pp, out, seed, extra=()):
    return ["--model_path", path, "--prompt_pickle", str(pp), "--output_file", str(out), "--num_gen_token",
            str(NUM_GEN), "--do_sample", "--temperature", str(FLAGS["temperature"]), "--top_k", str(FLAGS["top_k"]),
            "--top_p", str(FLAGS["top_p"]), "--seed", str(seed), "--num_gpus", "0"] + list(extra)


def _replay(path, prompts, scores, updated, seed):
    """From the output file alone: tok_t = oracle(scores[:, t, :], draw(seed, p, s, t)), and the
    updated prompts are suffix + decode(tokens)."""
    from flexible_llm_sharding_amd.utils.tokenizer import load_tokenizer
    tok = load_tokenizer(path)
    P = sr.ref_P(FLAGS["top_p"])
    assert len(scores) == len(prompts) == len(updated)
    tokens = []
    for p, ((pre, sufs), o) in enumerate(zip(prompts, scores)):
        assert o.shape[:2] == (len(sufs), NUM_GEN) and o.dtype == np.float16
        assert updated[p][0] == pre
        for s, sf in enumerate(sufs):
            t = [sr.ref_token(o[s, t], FLAGS["temperature"], FLAGS["top_k"], P, sr.ref_draw(seed, p, s, t))
                 for t in range(NUM_GEN)]
            assert updated[p][1][s] == sf + tok.decode(t), (p, s, t)
            tokens.append(t)
    return tokens


def _env():
    return dict(os.environ, PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="1")


def test_main_sampled_run_replays(tiny_model, tmp_path):
    """main.py on the torch backend, --num_batch 2 (the draws take the prompt-file index, not the
    index inside a batch): replayed from the output file; --metrics_json holds the parameters."""
    path, cfg = tiny_model
    prompts = _prompts(cfg)
    pp, out, mj = tmp_path / "prompts.pkl", tmp_path / "scores.pkl", tmp_path / "m.json"
    pickle.dump(prompts, open(pp, "wb"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py")] + _argv(path, pp, out, 17, [
        "--num_batch", "2", "--metrics_json", str(mj)]), cwd=str(tmp_path), env=_env(), capture_output=True, text=True,
        timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    _replay(path, prompts, pickle.load(open(out, "rb")), pickle.load(open(tmp_path / "prompts_updated.pkl", "rb")), 17)
    assert json.load(open(mj))["sampling"] == {"do_sample": True, "seed": 17, **FLAGS}


def test_same_seed_same_run_other_seed_other_run(tiny_model, tmp_path):
    """In process, one batch (the runner's own tokens through ops.sample_rows): the same seed
    twice gives identical files, a second seed different tokens; both replay."""
    from flexible_llm_sharding_amd.api import main
    path, cfg = tiny_model
    prompts = _prompts(cfg)
    pp = tmp_path / "prompts.pkl"
    pickle.dump(prompts, open(pp, "wb"))
    runs = {}
    for name, seed in (("a", 17), ("b", 17), ("c", 18)):
        out = tmp_path / f"{name}.pkl"
        assert main(_argv(path, pp, out, seed)) == 0
        runs[name] = (pickle.load(open(out, "rb")), pickle.load(open(tmp_path / "prompts_updated.pkl", "rb")))
    toks = {n: _replay(path, prompts, runs[n][0], runs[n][1], 17 if n != "c" else 18) for n in runs}
    assert runs["a"][1] == runs["b"][1] and all(np.array_equal(x, y) for x, y in zip(runs["a"][0], runs["b"][0]))
    assert toks["a"] == toks["b"] and toks["a"] != toks["c"] and runs["a"][1] != runs["c"][1]
    # the first step's scores do not depend on the seed; no sampling flag changes a score
    assert all(np.array_equal(x[:, 0], y[:, 0]) for x, y in zip(runs["a"][0], runs["c"][0]))


def test_main_data_parallel_sampled_run_replays(tiny_model, tmp_path):
    """Two gloo ranks, --data_parallel: rank 0 samples on the host from the gathered scores, with
    the prompt-file index of every prompt; replayed from the output file."""
    path, cfg = tiny_model
    prompts = _prompts(cfg)
    pp, out = tmp_path / "prompts.pkl", tmp_path / "dp.pkl"
    pickle.dump(prompts, open(pp, "wb"))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "main.py")] + _argv(path, pp, out, 17, [
               "--data_parallel"])
    r = subprocess.run(cmd, cwd=str(tmp_path), env=_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    updated = pickle.load(open(tmp_path / "prompts_updated.pkl", "rb"))
    _replay(path, prompts, pickle.load(open(out, "rb")), [tuple(u) for u in updated], 17)
