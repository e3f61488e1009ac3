"""Prompt-lookup speculative generation (``--lookup_decoding``) on the torch backend: the drafter
against a brute-force oracle, ``verify_rows`` against plain loops, the refusals, and generation end
to end — the same tokens, updated prompts and scores as the run without the flag, in fewer calls,
for an oracle drafter, drafters wrong at a chosen position, the real drafter and a suffix that
finishes early."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lookup_ref as lr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ drafter
def test_lookup_draft_equals_brute_force():
    from flexible_llm_sharding_amd.lookup import lookup_draft
    rng = np.random.default_rng(0)
    seen_n = set()
    for it in range(400):
        L = int(rng.integers(0, 40))
        t = rng.integers(0, 5, size=L)
        n_max, d = int(rng.integers(1, 9)), int(rng.integers(0, 17))
        got = lookup_draft(t, n_max, d)
        assert got.dtype == np.int64 and got.tolist() == lr.ref_draft(t, n_max, d), (t.tolist(), n_max, d)
        seen_n.add(len(got))
    assert 0 in seen_n and max(seen_n) >= 8
    # no match at all
    assert lookup_draft([1, 2, 3, 4], 3, 4).tolist() == []
    # a match only at n = 1 (the 2- and 3-grams ending the text occur nowhere else)
    assert lookup_draft([7, 1, 9, 2, 1], 3, 4).tolist() == [9, 2, 1]
    # the latest occurrence wins, not the first
    assert lookup_draft([1, 2, 5, 1, 2, 6, 1, 2], 2, 1).tolist() == [6]
    # the longest n-gram wins over a later shorter one
    assert lookup_draft([3, 1, 2, 8, 9, 2, 7, 1, 2], 2, 2).tolist() == [8, 9]
    # the only other occurrence is the text's end itself: nothing follows it, no draft
    assert lookup_draft([4, 5, 6], 2, 4).tolist() == []
    # an overlapping occurrence one token before the end is followed by one token
    assert lookup_draft([1, 1, 1], 2, 4).tolist() == [1]
    # d limits the draft; the function does not change its input
    t = np.array([1, 2, 3, 4, 1, 2])
    assert lookup_draft(t, 3, 2).tolist() == [3, 4] and t.tolist() == [1, 2, 3, 4, 1, 2]
    assert lookup_draft([], 3, 4).tolist() == [] and lookup_draft([1], 3, 4).tolist() == []


# ------------------------------------------------------------------ verify_rows
@pytest.mark.parametrize("case", [c for c in lr.kernel_cases() if c.V <= 2056], ids=lambda c: c.name)
def test_verify_rows_torch_equals_loops(case):
    from flexible_llm_sharding_amd.lookup import verify_rows
    from flexible_llm_sharding_amd.ops import get_ops
    ops = get_ops(torch.device("cpu"))
    tok, accept, keep, n_kept = ops.verify_rows(torch.from_numpy(case.scores), torch.from_numpy(case.row_start),
                                                torch.from_numpy(case.draft))
    wt, wa, wk = case.want()
    assert tok.dtype == accept.dtype == keep.dtype == n_kept.dtype == torch.int32
    assert np.array_equal(tok.numpy(), wt) and np.array_equal(accept.numpy(), wa)
    assert int(n_kept) == len(wk) and np.array_equal(keep.numpy()[:len(wk)], wk)
    ht, ha, hk = verify_rows(case.scores, case.row_start, case.draft)            # the host definition
    assert np.array_equal(ht, wt) and np.array_equal(ha, wa) and np.array_equal(hk, wk)


def test_host_verify_rows_on_every_case_and_the_cases_cover_the_edges():
    """``lookup.verify_rows`` (the host definition) equals the loops on every kernel case, V = 32000
    included; and, from the oracle, the cases hold the shapes, layouts and accepted counts the kernel
    test needs."""
    from flexible_llm_sharding_amd.lookup import verify_rows
    cases = lr.kernel_cases()
    for c in cases:
        for got, want in zip(verify_rows(c.scores, c.row_start, c.draft), c.want()):
            assert got.dtype == np.int32 and np.array_equal(got, want), c.name
    assert {c.V for c in cases} >= {97, 2056, 32000}
    assert any(len(c.row_start) == 301 for c in cases)
    rows = {int(n) for c in cases for n in np.diff(c.row_start)}
    assert rows >= set(range(1, 18))
    assert any(c.ld > c.V and c.ld % 8 == 0 for c in cases) and any(c.ld % 8 for c in cases if c.ld)
    assert any(c.offset == 1 for c in cases)
    for c in cases:
        tok, accept, keep = c.want()
        n = np.diff(c.row_start)
        for a, cnt, kind in zip(accept, n, c.want_accept):
            assert a == {"zero": 0, "mid": (cnt - 1) // 2, "all": cnt - 1}[kind], (c.name, a, cnt, kind)
        assert len(keep) == int(accept.sum()) + len(accept)
        bits = c.scores.view(np.uint16)
        zero = np.flatnonzero((bits == 0).all(axis=1))
        assert (tok[zero] == 0).all()
        if c.scores.shape[0] >= 17:
            assert zero.size > 0
            tied = [r for r in range(bits.shape[0]) if (bits[r] == bits[r].max()).sum() > 1 and bits[r].max() > 0]
            assert tied and all(tok[r] == np.flatnonzero(bits[r] == bits[r].max())[0] for r in tied)
    kinds = {(k, int(cnt)) for c in cases for k, cnt in zip(c.want_accept, np.diff(c.row_start)) if cnt >= 3}
    assert {k for k, _ in kinds} == {"zero", "mid", "all"}


# ------------------------------------------------------------------ refusals
def _args(*extra):
    from flexible_llm_sharding_amd.utils.cli import parse_args
    return parse_args(["--prompt_pickle", "p.pkl", "--output_file", "o.pkl", "--num_gen_token", "4"] + list(extra))


def test_flags_default_off_and_parse():
    a = _args()
    assert a.lookup_decoding == 0 and a.lookup_ngram == 3
    a = _args("--lookup_decoding", "16", "--lookup_ngram", "8")
    assert a.lookup_decoding == 16 and a.lookup_ngram == 8


@pytest.mark.parametrize("extra,flag", [
    (["--lookup_decoding", "17"], "--lookup_decoding"),
    (["--lookup_decoding", "-1"], "--lookup_decoding"),
    (["--lookup_decoding", "4", "--lookup_ngram", "0"], "--lookup_ngram"),
    (["--lookup_decoding", "4", "--lookup_ngram", "9"], "--lookup_ngram"),
    (["--lookup_ngram", "9"], "--lookup_ngram"),
    (["--lookup_decoding", "4", "--do_sample"], "--do_sample"),
    (["--lookup_decoding", "4", "--hip_graphs"], "--hip_graphs"),
    (["--lookup_decoding", "4", "--suffix_kv_cache", "false"], "--suffix_kv_cache"),
    (["--lookup_decoding", "4", "--exact_reuse", "false"], "--exact_reuse"),
    (["--lookup_decoding", "4", "--num_batch", "2"], "--num_batch"),
    (["--lookup_decoding", "4", "--num_gpus", "2"], "more than one GPU"),
])
def test_refusals_name_the_flag(extra, flag):
    with pytest.raises(ValueError, match=flag) as e:
        _args(*extra)
    assert "--lookup" in str(e.value)


def test_refusals_loglik_and_ranks():
    import argparse

    from flexible_llm_sharding_amd.utils.cli import check_lookup
    ns = argparse.Namespace(lookup_decoding=4, lookup_ngram=3, score_mode="loglik")
    with pytest.raises(ValueError, match="--score_mode loglik"):
        check_lookup(ns)
    ns = argparse.Namespace(lookup_decoding=4, lookup_ngram=3)
    check_lookup(ns, world=1)
    with pytest.raises(ValueError, match="more than one GPU"):
        check_lookup(ns, world=2)


def test_runner_refuses_drafts_without_row_exact_calls(tiny_model):
    from flexible_llm_sharding_amd.engine import ShardedRunner
    setup = lr.engine_setup(tiny_model)
    cfg, tok, prompts, src = setup
    r = ShardedRunner(cfg, src, "cpu", tok, prefix_kv_cache=False)
    tps = r.tokenize(prompts)
    with pytest.raises(ValueError, match="row-exact"):
        r.run_tokenized(tps, drafts=[[[] for _ in tp.suffixes] for tp in tps])
    r.close()
    r = ShardedRunner(cfg, src, "cpu", tok, prefix_kv_cache=True, suffix_kv_cache=True)
    with pytest.raises(ValueError, match="does not end with its draft"):
        r.run_tokenized(tps, drafts=[[[5] for _ in tp.suffixes] for tp in tps])
    r.close()


# ------------------------------------------------------------------ packing
def test_score_rows_of_one_is_todays_packing(tiny_model):
    """The default count of 1 packs byte for byte what the call without ``score_rows`` packs, and
    a larger count scores the suffix's trailing rows with one single-query item each."""
    from flexible_llm_sharding_amd.runtime.batch import pack_prompts
    from flexible_llm_sharding_amd.utils.tokenizer import tokenize_prompts
    cfg, tok, prompts, _ = lr.engine_setup(tiny_model)
    tps = tokenize_prompts(tok, prompts)
    ones = [[1] * tp.n_suffix for tp in tps]
    for kw in ({}, {"window": 5}, {"single_suffix_items": True}):
        a = pack_prompts(tps, [0, 1], **kw)
        b = pack_prompts(tps, [0, 1], score_rows=ones, **kw)
        for k, v in a.host_meta().items():
            assert v.dtype == b.host_meta()[k].dtype and np.array_equal(v, b.host_meta()[k]), k
        assert a.last_segments == b.last_segments
    counts = [[min(3, len(s)) for s in tp.suffixes] for tp in tps]
    c = pack_prompts(tps, [0, 1], score_rows=counts)
    a = pack_prompts(tps, [0, 1])
    assert c.n_scored == sum(map(sum, counts)) and c.work_last.shape[0] == c.n_scored
    want = [int(last) - k + 1 + i for last, k in zip(a.last_idx, [x for row in counts for x in row]) for i in range(k)]
    assert c.last_idx.tolist() == want
    assert all(sg.q_len == 1 and sg.q_start == r for sg, r in zip(c.last_segments, want))
    with pytest.raises(ValueError, match="score_rows"):
        pack_prompts(tps, [0, 1], score_rows=[[len(s) + 1 for s in tp.suffixes] for tp in tps])


# ------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def world(tiny_model):
    """(setup, the plain run, the continuation table), once: prompts whose plain continuation
    holds only ordinary words (a generated special token does not re-tokenize as one word)."""
    for seed in range(21, 29):
        setup = lr.engine_setup(tiny_model, seed)
        plain = lr.generate(setup, "cpu")
        if not lr.has_special(plain):
            return setup, plain, lr.continuation_table(setup, plain)
    raise AssertionError("no prompt seed gives a continuation of ordinary words")


def _same_outputs(plain, got):
    """The comparison of test_engine_cpu.py::test_prefix_kv_cache_generation_exact."""
    assert got.updated == plain.updated
    assert len(got.scores) == len(plain.scores)
    for a, b, ta, tb in zip(plain.scores, got.scores, plain.tokens, got.tokens):
        assert a.shape == b.shape and a.dtype == b.dtype
        assert np.abs(a.astype(np.float32) - b.astype(np.float32)).max() < 1e-5
        assert np.array_equal(ta, tb)


def test_plain_run_is_untouched_by_the_flag_off(world):
    setup, plain, _ = world
    assert plain.stats == {} and len(plain.calls) == lr.NUM_GEN and not any(c["drafted"] for c in plain.calls)
    assert all(s.shape == (3, lr.NUM_GEN, setup[0].vocab_size) for s in plain.scores)


def test_oracle_drafter_two_calls(world):
    setup, plain, table = world
    got = lr.generate(setup, "cpu", lookup=lr.D, drafter=lr.oracle_drafter(table))
    _same_outputs(plain, got)
    n_sfx = sum(len(p[1]) for p in setup[2])
    assert got.stats["lookup_calls"] == -(-lr.NUM_GEN // (lr.D + 1)) == 2 == len(got.calls)
    assert got.stats["lookup_dropped_roundtrip"] == 0 and got.stats["lookup_retokenized"] == 0
    assert got.stats["lookup_drafted"] == got.stats["lookup_accepted"] == n_sfx * (lr.NUM_GEN - 2)
    assert [c["rows"] for c in got.calls] == [n_sfx * 5, n_sfx * 3] == [c["kept"] for c in got.calls]
    assert [c["accept"] for c in got.calls] == [[4] * n_sfx, [2] * n_sfx] == [c["n_draft"] for c in got.calls]


@pytest.mark.parametrize("j", [0, 2, 3])
def test_drafter_wrong_at_position(world, j):
    setup, plain, table = world
    got = lr.generate(setup, "cpu", lookup=lr.D, drafter=lr.wrong_at(table, j, setup[0].vocab_size))
    _same_outputs(plain, got)
    n_sfx = sum(len(p[1]) for p in setup[2])
    assert got.stats["lookup_dropped_roundtrip"] == 0
    assert got.stats["lookup_accepted"] < got.stats["lookup_drafted"]
    # the first call drafts 4 tokens per suffix and accepts exactly the j before the wrong one
    assert got.calls[0]["rows"] == n_sfx * 5 and got.calls[0]["kept"] == n_sfx * (j + 1)
    # j = 0: every draft fails at once, a token per call; j = 2: 3 + 3 + 2 tokens (the last call's one
    # draft token has no position 2); j = 3: 4 + 4 (the second call drafts only 3)
    assert got.stats["lookup_calls"] == {0: lr.NUM_GEN, 2: 3, 3: 2}[j]


def test_all_wrong_drafter_accepts_nothing(world):
    setup, plain, table = world
    got = lr.generate(setup, "cpu", lookup=lr.D, drafter=lr.all_wrong(table, setup[0].vocab_size))
    _same_outputs(plain, got)
    assert got.stats["lookup_accepted"] == 0 and got.stats["lookup_drafted"] > 0
    assert got.stats["lookup_calls"] == lr.NUM_GEN
    # (the last call has no room for a draft: the plain path)
    assert [c["drafted"] for c in got.calls] == [True] * (lr.NUM_GEN - 1) + [False]
    assert all(c["kept"] == 6 for c in got.calls if c["drafted"])


def test_real_drafter_on_a_prefix_that_holds_the_continuation(world):
    setup, plain, _ = world
    prompts = lr.repeat_prompts(setup, plain)
    plain2 = lr.generate(setup, "cpu", prompts=prompts)
    got = lr.generate(setup, "cpu", lookup=lr.D, prompts=prompts)
    _same_outputs(plain2, got)
    assert got.stats["lookup_drafted"] > 0 and 0 <= got.stats["lookup_accepted"] <= got.stats["lookup_drafted"]
    assert got.stats["lookup_calls"] <= lr.NUM_GEN
    print("real drafter:", got.stats)


def test_suffix_that_finishes_early_rides_along(world):
    setup, plain, table = world
    got = lr.generate(setup, "cpu", lookup=lr.D, drafter=lr.only_first_suffix(table, setup))
    _same_outputs(plain, got)
    # suffix 0 of each prompt is done after two calls; the others take one token per call
    assert got.stats["lookup_calls"] == lr.NUM_GEN
    assert got.stats["lookup_drafted"] == got.stats["lookup_accepted"] == 2 * (lr.NUM_GEN - 2)
    assert [c["drafted"] for c in got.calls] == [True, True] + [False] * (lr.NUM_GEN - 2)
    assert got.calls[0]["n_draft"] == [4, 0, 0, 4, 0, 0] == got.calls[0]["accept"]      # runner.last_accept


def test_score_top_k_with_lookup(world):
    setup, plain, table = world
    full = lr.generate(setup, "cpu", top_k=5)
    got = lr.generate(setup, "cpu", top_k=5, lookup=lr.D, drafter=lr.wrong_at(table, 2, setup[0].vocab_size))
    assert got.updated == full.updated == plain.updated
    for a, b in zip(full.scores, got.scores):
        assert a.dtype == b.dtype and a.shape == b.shape == (3, lr.NUM_GEN, 5)
        assert np.array_equal(a["id"], b["id"])
        assert np.abs(a["p"].astype(np.float32) - b["p"].astype(np.float32)).max() < 1e-5
    for k in ("token_ids", "token_probs"):
        assert all(x.shape == y.shape and x.dtype == y.dtype for x, y in zip(full.record[k], got.record[k]))
    assert all(np.array_equal(x, y) for x, y in zip(full.record["token_ids"], got.record["token_ids"]))


def test_main_cli_same_files(world, tiny_model, tmp_path):
    """main.py --num_gen_token 8 --lookup_decoding 4: the same _updated.pkl, tokens and scores as
    without the flag, and the metrics name the lookup counters."""
    setup, plain, _ = world
    path, cfg = tiny_model
    prompts = lr.repeat_prompts(setup, plain)
    env = dict(os.environ, PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    outs = {}
    for name, extra in (("plain", []), ("lookup", ["--lookup_decoding", "4", "--lookup_ngram", "2"])):
        d = tmp_path / name
        d.mkdir()
        pickle.dump(prompts, open(d / "p.pkl", "wb"))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--model_path", path, "--prompt_pickle",
                            str(d / "p.pkl"), "--output_file", str(d / "s.pkl"), "--num_gen_token", "8",
                            "--metrics_json", str(d / "m.json")] + extra, cwd=str(d), env=env, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        outs[name] = (pickle.load(open(d / "p_updated.pkl", "rb")), pickle.load(open(d / "s.pkl", "rb")),
                      json.load(open(d / "m.json")))
    assert outs["plain"][0] == outs["lookup"][0]
    for a, b in zip(outs["plain"][1], outs["lookup"][1]):
        assert a.shape == b.shape == (3, 8, cfg.vocab_size) and a.dtype == b.dtype == np.float16
        assert np.array_equal(np.argmax(a, -1), np.argmax(b, -1))
        assert np.abs(a.astype(np.float32) - b.astype(np.float32)).max() < 1e-5
    m = outs["lookup"][2]
    assert m["lookup_decoding"] == 4 and m["lookup_ngram"] == 2
    for k in ("lookup_calls", "lookup_drafted", "lookup_accepted", "lookup_dropped_roundtrip", "lookup_retokenized"):
        assert isinstance(m[k], int), k
    assert 1 <= m["lookup_calls"] <= 8 and m["lookup_drafted"] > 0
    assert "lookup_calls" not in outs["plain"][2]
