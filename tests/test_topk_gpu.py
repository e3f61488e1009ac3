"""Compact next-token scores on an MI355X: the ``fls_topk_rows`` kernel equals the oracle of
tests/topk_ref.py entry for entry, and a run with ``score_top_k`` returns exactly the oracle applied
to the full scores of the same run without the flag, with the same tokens and prompts, through
decode graphs, the speculative step, eager steps, a capped run, ``--hip_graphs`` and sampling.

Everything is integer-exact: every comparison is an equality of ids and bit patterns.  The cases
are built once in tests/topk_ref.py; a CPU-only test here checks from the oracle alone that they
discriminate."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topk_ref as tr  # noqa: E402

CASES = tr.kernel_cases()


def test_cases_discriminate():
    """CPU only.  Two deliberate mistakes of the oracle each change the expected output in the
    families built for them: the wrong tie order (index descending) in the tie, scan-boundary,
    flat, all-zero, one-bin and few-non-zero families; invalid patterns ranked by their raw bits
    in the invalid family (and nowhere else: no other family holds one).  The shapes, K values and
    layouts the issue lists are all present, and the consequences of the definition hold."""
    changed = {}
    for c in CASES:
        for m in ("tie_order", "raw_invalid"):
            (wi, wv), (mi, mv) = c.want(), c.want(m)
            diff = (wi != mi).any(axis=1) | (wv != mv).any(axis=1)
            for f, d in zip(c.family, diff):
                changed[(f, m)] = changed.get((f, m), 0) + int(d)
    for fam in ("ties", "scan", "flat", "zero", "onebin", "few"):
        assert changed[(fam, "tie_order")] > 0, (fam, changed)
    assert changed[("invalid", "raw_invalid")] > 0
    assert all(n == 0 for (fam, m), n in changed.items() if m == "raw_invalid" and fam != "invalid")
    assert {c.V for c in CASES} >= {97, 2056, 32000, 151936}
    assert {c.K for c in CASES} >= {1, 2, 5, 64, 1000, 1024, 97}
    assert any(c.K == c.V for c in CASES)
    assert any(c.ld > c.V and c.ld % 8 == 0 for c in CASES) and any(c.ld % 8 for c in CASES)
    assert any(c.offset for c in CASES) and any(len(c.scores) == 300 for c in CASES)
    assert any(c.picked is None for c in CASES)
    for c in CASES:
        ids, vals = c.want()
        assert ids.dtype == np.int32 and vals.dtype == np.uint16 and ids.shape == vals.shape == (len(c.scores), c.K)
        ok = c.valid_rows()
        assert np.array_equal(ids[ok, 0], np.argmax(c.scores[ok].view(np.uint16), axis=1)), c.name
        for r, f in enumerate(c.family):
            if f in ("zero", "flat"):
                assert ids[r].tolist() == list(range(c.K)), (c.name, f)
            if f == "few":                       # the zero-key fill: the lowest free indices, in order
                z = ids[r][vals[r] == 0]
                zero_cols = np.flatnonzero(c.scores[r].view(np.uint16) == 0)
                assert len(z) == c.K - min(c.K, c.V - len(zero_cols)), c.name
                assert np.array_equal(z, zero_cols[:len(z)]), c.name
        if "few" in c.family:
            assert sum(int((vals[r] == 0).any()) for r, f in enumerate(c.family) if f == "few") >= 1, c.name
        if c.picked is not None:
            assert (c.picked >= c.V).any() and (c.picked < 0).any() and 0 in c.picked and c.V - 1 in c.picked


gpu = pytest.mark.gpu
HAVE_GPU = torch.cuda.is_available()
needs_gpu = pytest.mark.skipif(not HAVE_GPU, reason="no GPU")
DEV = torch.device("cuda", 0)


# ------------------------------------------------------------------ kernel
def _on_gpu(case: tr.Case) -> torch.Tensor:
    """The case's rows on the device with its row stride and base offset; everything around the
    rows holds 1.0, which a read outside a row would turn into a wrong first entry."""
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
def test_topk_rows_equals_oracle(case):
    from flexible_llm_sharding_amd.ops import get_ops
    ops = get_ops(DEV)
    x = _on_gpu(case)
    picked = None if case.picked is None else torch.from_numpy(case.picked).to(DEV)
    ids, vals, pv = ops.topk_rows(x, case.K, picked=picked)
    am = ops.argmax_rows(x)
    torch.cuda.synchronize()
    assert ids.dtype == torch.int32 and vals.dtype == torch.float16 and tuple(ids.shape) == tuple(vals.shape)
    ids, vals = ids.cpu().numpy(), vals.cpu().numpy().view(np.uint16)
    wi, wv = case.want()
    bad = np.flatnonzero((ids != wi).any(axis=1) | (vals != wv).any(axis=1))
    assert bad.size == 0, (case.name, bad[:8], [case.family[r] for r in bad[:8]], ids[bad[:2]], wi[bad[:2]])
    if picked is None:
        assert pv is None
    else:
        assert pv.dtype == torch.float16
        assert np.array_equal(pv.cpu().numpy().view(np.uint16), case.want_picked()), case.name
    ok = case.valid_rows()
    assert np.array_equal(ids[ok, 0], am.cpu().numpy()[ok]), case.name


@gpu
@needs_gpu
def test_topk_rows_checks_its_arguments():
    from flexible_llm_sharding_amd import _native
    from flexible_llm_sharding_amd.ops import get_ops
    ops = get_ops(DEV)
    x = torch.zeros(2, 64, dtype=torch.float16, device=DEV)
    p = torch.zeros(2, dtype=torch.int32, device=DEV)
    with pytest.raises(TypeError):
        ops.topk_rows(x.float(), 2)
    with pytest.raises(TypeError):
        ops.topk_rows(x.cpu(), 2)
    with pytest.raises(TypeError):
        ops.topk_rows(x[0], 2)
    with pytest.raises(TypeError):
        ops.topk_rows(x, 2, picked=p[:1])
    with pytest.raises(TypeError):
        ops.topk_rows(x, 2, picked=p.long())
    with pytest.raises(TypeError):
        ops.topk_rows(x, 2, picked=p.cpu())
    for K in (0, -1, 65, 1025):
        with pytest.raises(ValueError):
            ops.topk_rows(x, K)
    ids, vals, pv = ops.topk_rows(x, 3, picked=p)
    assert ids.tolist() == [[0, 1, 2], [0, 1, 2]] and vals.tolist() == [[0, 0, 0]] * 2 and pv.tolist() == [0, 0]
    # the C entry point refuses the same values (no launch), and does nothing for rows <= 0
    k = _native.kernels()
    i32 = torch.zeros(2 * 1100, dtype=torch.int32, device=DEV)
    f16 = torch.zeros(2 * 1100, dtype=torch.float16, device=DEV)
    big = torch.zeros(2, 2048, dtype=torch.float16, device=DEV)

    def call(t, ld, rows, V, K):
        return k.fls_topk_rows(t.data_ptr(), ld, rows, V, K, i32.data_ptr(), f16.data_ptr(), None, None, None)
    assert call(x, 64, 2, 0, 1) != 0 and call(x, 32, 2, 64, 1) != 0 and call(x, 64, 2, 64, 0) != 0
    assert call(x, 64, 2, 64, 65) != 0 and call(big, 2048, 2, 2048, 1025) != 0
    assert call(x, 64, 0, 64, 1) == 0 and call(x, 64, -1, 64, 1) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ engine
SAMPLING = dict(temperature=0.8, top_k=50, top_p=0.95, seed=5)
CONFIGS = {
    "scoring_pass": {"num_gen": 1},
    "default": {},
    "no_spec": {"env": {"FLS_SPEC_DECODE": "0"}},
    "no_suffix_reuse": {"suffix_kv_cache": False},
    "capped": {"resident": False, "max_vram_gb": 40},
    "hip_graphs": {"hip_graphs": True, "prefix_kv_cache": False, "suffix_kv_cache": False},
    "sampled": {"sampling": SAMPLING},
}
_FULL = {}


@pytest.fixture(scope="module")
def setup(tiny_model):
    return tr.engine_setup(tiny_model)


def _full(setup, config):
    """The run without the flag, once per configuration (read-only afterwards)."""
    if config not in _FULL:
        _FULL[config] = tr.generate(setup, DEV, **CONFIGS[config])
    return _FULL[config]


@gpu
@needs_gpu
@pytest.mark.parametrize("K", [1, 20])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_engine_compact_scores_equal_oracle_on_full_scores(setup, config, K):
    """For every prompt and step the returned entries are the oracle applied to the full scores of
    the same run without the flag; ``last_tokens``, the updated prompts and the token
    probabilities equal that run's; speculative steps are held exactly as there."""
    full = _full(setup, config)
    got = tr.generate(setup, DEV, top_k=K, **CONFIGS[config])
    tr.check_compact_run(full, got, K)
    steps = CONFIGS[config].get("num_gen", tr.NUM_GEN)
    assert all(o.shape[1] == steps for o in got.scores)
    assert [s.get("speculative") for s in got.stats] == [s.get("speculative") for s in full.stats]
    assert [s.get("graph_replays") for s in got.stats] == [s.get("graph_replays") for s in full.stats]
    assert got.dropped == full.dropped
    print(config, K, "speculative per step:", [s.get("speculative") for s in got.stats], "dropped", got.dropped,
          "score D2H bytes per step:", got.d2h, "without the flag:", full.d2h)
    if config == "default":
        assert got.stats[-1].get("graph_replays", 0) >= 1
        assert 1.0 in [s.get("speculative") for s in got.stats]
    if config == "sampled":                      # the sampled tokens are not all the first ranked entry
        first = [o["id"][:, :, 0] for o in got.scores]
        assert any((f != t).any() for f, t in zip(first, got.record["token_ids"]))
    # the host never saw a [rows, V] row: the copy is K (id, probability) pairs and one token per row
    rows = sum(len(p[1]) for p in setup[2])
    assert all(b == rows * (6 * K + 6) for b in got.d2h), got.d2h
    assert all(b == rows * (2 * setup[0].vocab_size + 4) for b in full.d2h), full.d2h
