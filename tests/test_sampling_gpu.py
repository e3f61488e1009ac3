"""Sampled generation on an MI355X: the ``fls_sample_rows`` kernel equals the oracle of
tests/sampling_ref.py token for token, and the engine's device tokens equal the oracle applied to
the scores it returns, through decode graphs, the speculative step, eager steps and a capped run.

Everything is integer-exact, so every comparison is an equality.  The cases are built once in
tests/sampling_ref.py; a CPU-only test here checks from the oracle alone that they discriminate."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_ref as sr  # noqa: E402

CASES = sr.kernel_cases()


def test_cases_discriminate():
    """CPU only.  Three deliberate mistakes of the oracle each change expected tokens in the
    families built to catch them (a family such as the all-invalid rows cannot tell them apart):
    a wrong tie order in the tie, flat and random families; ``>`` for ``>=`` at tau in the tau
    family; ranking by weight instead of bits in the equal-weight family.  The flat rows expect
    exactly the column each draw was made for, and the shapes the issue lists are all present."""
    changed = {}
    for c in CASES:
        for m in ("tie_order", "tau_gt", "by_weight"):
            changed[(c.family, m)] = changed.get((c.family, m), 0) + int((c.want(m) != c.want()).sum())
    for fam, m in (("ties", "tie_order"), ("flat", "tie_order"), ("random", "tie_order"), ("tau", "tau_gt"),
                   ("equal_weight", "by_weight")):
        assert changed[(fam, m)] > 0, (fam, m, changed)
    for c in CASES:
        if c.family == "flat":
            cols = list(range(c.V)) if len(c.scores) == c.V else sr.edge_columns(c.V)
            assert c.want().tolist() == cols, c.name
            assert {0, 7, 8, c.V - 1} <= set(cols)
        if c.name == "tau_unit_P49152":        # tau on the boundary keeps two tokens, one unit above keeps three
            assert c.want()[0] == 9 and [x for x in CASES if x.name == "tau_unit_P49153"][0].want()[0] == 8
            assert [x for x in CASES if x.name == "tau_unit_P49151"][0].want()[0] == 9
        if c.family == "invalid":              # rows 0-6 choose a valid entry, row 7 has none
            bits = c.scores.view(np.uint16)[np.arange(7), c.want()[:7]]
            assert ((bits >= 1) & (bits <= sr.ONE)).all() and c.want()[7] == 0
    assert {c.V for c in CASES} >= {97, 2056, 32000, 151936}
    assert any(c.ld > c.V for c in CASES) and any(c.offset for c in CASES) and any(len(c.scores) == 300 for c in CASES)
    lo, hi = sr.equal_weight_bits(0.7)
    assert lo != hi and sr.ref_weights(np.array([lo, hi]), 0.7)[0] == sr.ref_weights(np.array([lo, hi]), 0.7)[1] > 0


gpu = pytest.mark.gpu
HAVE_GPU = torch.cuda.is_available()
needs_gpu = pytest.mark.skipif(not HAVE_GPU, reason="no GPU")
DEV = torch.device("cuda", 0)


# ------------------------------------------------------------------ kernel
_TABLES = {}


def _table(T):
    from flexible_llm_sharding_amd.sampling import weight_table
    if T not in _TABLES:
        _TABLES[T] = torch.from_numpy(weight_table(T).view(np.int32)).to(DEV)
    return _TABLES[T]


def _on_gpu(case: sr.Case) -> torch.Tensor:
    """The case's rows on the device with its row stride and base offset; everything around the
    rows holds 1.0, which a read outside a row would turn into a wrong token."""
    rows, V = case.scores.shape
    ld = case.ld or V
    flat = torch.ones(rows * ld + 8, dtype=torch.float16, device=DEV)
    view = flat[case.offset:case.offset + rows * ld].view(rows, ld)[:, :V]
    view.copy_(torch.from_numpy(case.scores).to(DEV))
    assert view.data_ptr() % 16 == (2 * case.offset) % 16
    return view


@gpu
@needs_gpu
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_sample_rows_equals_oracle(case):
    from flexible_llm_sharding_amd.ops import get_ops
    ops = get_ops(DEV)
    draws = torch.from_numpy(case.draws.view(np.int64)).to(DEV)
    got = ops.sample_rows(_on_gpu(case), _table(case.T), draws, case.top_k, case.P)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    want = case.want()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (case.name, bad[:8], got[bad[:8]], want[bad[:8]])


@gpu
@needs_gpu
def test_top_k_one_and_p_one_are_argmax():
    from flexible_llm_sharding_amd.ops import get_ops
    ops = get_ops(DEV)
    for case in [c for c in CASES if c.family in ("ties", "random") and c.V <= 2056][:8]:
        x = _on_gpu(case)
        draws = torch.from_numpy(case.draws.view(np.int64)).to(DEV)
        am = ops.argmax_rows(x).cpu().numpy()
        assert np.array_equal(am, np.argmax(case.scores, axis=-1))
        for k, P in ((1, 65536), (0, 1), (1, 1)):
            assert np.array_equal(ops.sample_rows(x, _table(case.T), draws, k, P).cpu().numpy(), am), (case.name, k, P)


@gpu
@needs_gpu
def test_sample_rows_checks_its_arguments():
    from flexible_llm_sharding_amd.ops import get_ops
    ops = get_ops(DEV)
    x = torch.zeros(2, 64, dtype=torch.float16, device=DEV)
    d = torch.zeros(2, dtype=torch.int64, device=DEV)
    t = _table(1.0)
    with pytest.raises(TypeError):
        ops.sample_rows(x.float(), t, d, 0, 65536)
    with pytest.raises(TypeError):
        ops.sample_rows(x, t[:100], d, 0, 65536)
    with pytest.raises(TypeError):
        ops.sample_rows(x, t, d[:1], 0, 65536)
    with pytest.raises(TypeError):
        ops.sample_rows(x, t, d.cpu(), 0, 65536)
    with pytest.raises(ValueError):
        ops.sample_rows(x, t, d, 0, 0)
    with pytest.raises(ValueError):
        ops.sample_rows(x, t, d, -1, 65536)
    assert ops.sample_rows(x, t, d, 0, 65536).tolist() == [0, 0]


# ------------------------------------------------------------------ engine
NUM_GEN = 4
PARAMS = dict(temperature=0.8, top_k=50, top_p=0.95)


@pytest.fixture(scope="module")
def setup(tiny_model):
    from flexible_llm_sharding_amd.runtime.weights import HostStore
    from flexible_llm_sharding_amd.utils.synthetic import synthetic_prompts
    from flexible_llm_sharding_amd.utils.tokenizer import load_tokenizer
    path, cfg = tiny_model
    tok = load_tokenizer(path)
    prompts = synthetic_prompts(3, 40, 3, 12, cfg.vocab_size, seed=21, vary=True)
    prompts[1] = (prompts[1][0], prompts[1][1][:2])             # 3, 2 and 3 suffixes
    return cfg, tok, prompts, HostStore.from_model_path(cfg, path)


def _generate(setup, seed=5, sample=True, env=None, **kw):
    """One generation of NUM_GEN tokens -> (scores, updated prompts, per-step device tokens,
    per-step stats, spec_dropped)."""
    from flexible_llm_sharding_amd.api import generation_loop
    from flexible_llm_sharding_amd.engine import ShardedRunner
    from flexible_llm_sharding_amd.parallel.comm import Comm
    from flexible_llm_sharding_amd.sampling import SamplingParams
    cfg, tok, prompts, src = setup

    class Recording(ShardedRunner):
        def __call__(self, ps):
            out = super().__call__(ps)
            self.seen.append(([None if t is None else t.copy() for t in self.last_tokens], dict(self.stats)))
            return out

    flags = dict(PARAMS, **{k: kw.pop(k) for k in list(kw) if k in PARAMS})
    args = argparse.Namespace(num_gen_token=NUM_GEN, data_parallel=False, num_batch=1, do_sample=sample, seed=seed,
                              **(flags if sample else {}))
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        base = dict(layer_num_per_shard=1, prefix_kv_cache=True, suffix_kv_cache=True, resident=True)
        base.update(kw)
        r = Recording(cfg, src, DEV, tok, sampling=SamplingParams.from_args(args), **base)
        r.seen = []
        scores, updated = generation_loop(args, r, Comm(), tok, prompts)
        assert r._spec is None
        seen, dropped = r.seen, r.spec_dropped
        r.close()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    return scores, updated, [s[0] for s in seen], [s[1] for s in seen], dropped


def _oracle_tokens(scores, seed, flags=PARAMS):
    """[step][prompt] -> [n_s] tokens: the oracle on the returned scores with the draws of (seed, p, s, t)."""
    P = sr.ref_P(flags["top_p"])
    return [[np.asarray([sr.ref_token(o[s, t], flags["temperature"], flags["top_k"], P, sr.ref_draw(seed, p, s, t))
                         for s in range(o.shape[0])]) for p, o in enumerate(scores)] for t in range(NUM_GEN)]


def _check_run(setup, scores, updated, dev_tokens, seed):
    cfg, tok, prompts, _ = setup
    assert len(dev_tokens) == NUM_GEN
    want = _oracle_tokens(scores, seed)
    for t in range(NUM_GEN):
        for p, w in enumerate(want[t]):
            assert dev_tokens[t][p] is not None and np.array_equal(dev_tokens[t][p][:, 0], w), (t, p)
    for p, (pre, sufs) in enumerate(prompts):
        assert updated[p][0] == pre
        for s, sf in enumerate(sufs):
            assert updated[p][1][s] == sf + tok.decode([int(want[t][p][s]) for t in range(NUM_GEN)])


CONFIGS = {"default": {}, "no_spec": {"env": {"FLS_SPEC_DECODE": "0"}}, "no_suffix_reuse": {"suffix_kv_cache": False},
           "capped": {"resident": False, "max_vram_gb": 40}}


@gpu
@needs_gpu
@pytest.mark.parametrize("config", list(CONFIGS))
def test_engine_tokens_equal_oracle_on_returned_scores(setup, config):
    """(a) every step's device tokens == the oracle on that step's returned scores; the updated
    prompts are suffix + decode(those tokens)."""
    scores, updated, dev_tokens, stats, _ = _generate(setup, seed=5, **CONFIGS[config])
    _check_run(setup, scores, updated, dev_tokens, 5)
    assert all(o.shape[1] == NUM_GEN for o in scores)
    if config == "default":
        assert stats[-1].get("graph_replays", 0) >= 1


@gpu
@needs_gpu
def test_sampled_speculative_steps_hold(setup):
    """(b) decode graphs + the speculative step: from the third step on every step was computed
    speculatively from the sampled ids (``_launch_spec`` swallows exceptions, so a broken sampled
    speculation would otherwise go unnoticed).  A speculation assumes that re-tokenizing suffix +
    decode(token) appends exactly that token, which the synthetic tokenizer gives for every token
    but the three special ones: the first seed whose run samples none of them is the one checked."""
    for seed in range(6):
        scores, updated, dev_tokens, stats, dropped = _generate(setup, seed=seed)
        if all(int(t.min()) >= 3 for step in dev_tokens for t in step):
            break
    else:
        pytest.fail("every seed sampled a special token")
    _check_run(setup, scores, updated, dev_tokens, seed)
    print("speculative per step:", [s.get("speculative") for s in stats], "dropped", dropped)
    assert [s["speculative"] for s in stats[2:]] == [1.0] * (NUM_GEN - 2)
    assert dropped == 0


@gpu
@needs_gpu
def test_top_k_one_equals_greedy_run(setup):
    """(c) --do_sample --top_k 1: scores bitwise equal and prompts equal to the greedy run."""
    s0, u0, t0, _, _ = _generate(setup, sample=False)
    s1, u1, t1, _, _ = _generate(setup, seed=9, top_k=1)
    assert u0 == u1
    for a, b in zip(s0, s1):
        assert np.array_equal(a.view(np.uint16), b.view(np.uint16))
    for x, y in zip(t0, t1):
        assert all(np.array_equal(a, b) for a, b in zip(x, y))


@gpu
@needs_gpu
def test_sampled_suffix_reuse_on_and_off_bitwise(setup):
    """(d) sampled runs with suffix K/V reuse on and off: bitwise-equal scores, equal tokens."""
    s0, u0, t0, st0, _ = _generate(setup, seed=11)
    s1, u1, t1, _, _ = _generate(setup, seed=11, suffix_kv_cache=False)
    assert st0[-1]["suffix_tokens_reused"] > 0
    assert u0 == u1
    for a, b in zip(s0, s1):
        assert np.array_equal(a.view(np.uint16), b.view(np.uint16))
    for x, y in zip(t0, t1):
        assert all(np.array_equal(a, b) for a, b in zip(x, y))
    # and another seed does give other tokens
    _, u2, _, _, _ = _generate(setup, seed=12)
    assert u2 != u0
