"""Prompt-lookup speculative generation on an MI355X: the ``fls_verify_rows`` kernel equals the
loops of tests/lookup_ref.py entry for entry, and a generation with ``--lookup_decoding`` returns
bit for bit the scores and exactly the tokens of the run without the flag — weights resident,
streamed, under a VRAM cap with host-mode caches and with ``--score_top_k`` — for an oracle drafter,
drafters wrong at a chosen position and the real drafter, copying only the kept rows to the host."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lookup_ref as lr  # noqa: E402

gpu = pytest.mark.gpu
HAVE_GPU = torch.cuda.is_available()
needs_gpu = pytest.mark.skipif(not HAVE_GPU, reason="no GPU")
DEV = torch.device("cuda", 0)
CASES = lr.kernel_cases()


# ------------------------------------------------------------------ kernel
def _on_gpu(case: lr.Case) -> torch.Tensor:
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
def test_verify_rows_equals_loops(case):
    from flexible_llm_sharding_amd.ops import get_ops
    ops = get_ops(DEV)
    x = _on_gpu(case)
    rs, dr = torch.from_numpy(case.row_start).to(DEV), torch.from_numpy(case.draft).to(DEV)
    tok, accept, keep, n_kept = ops.verify_rows(x, rs, dr)
    am = ops.argmax_rows(x)
    torch.cuda.synchronize()
    wt, wa, wk = case.want()
    assert tok.dtype == accept.dtype == keep.dtype == n_kept.dtype == torch.int32
    assert tuple(tok.shape) == (len(wt),) and tuple(accept.shape) == (len(wa),) and tuple(keep.shape) == (len(wt),)
    tok, accept, keep = tok.cpu().numpy(), accept.cpu().numpy(), keep.cpu().numpy()
    bad = np.flatnonzero(tok != wt)
    assert bad.size == 0, (case.name, bad[:8], tok[bad[:8]], wt[bad[:8]])
    assert np.array_equal(tok, am.cpu().numpy()), case.name
    assert np.array_equal(accept, wa), (case.name, np.flatnonzero(accept != wa)[:8])
    assert int(n_kept.item()) == len(wk)
    assert np.array_equal(keep[:len(wk)], wk), case.name


@gpu
@needs_gpu
def test_verify_rows_checks_its_arguments():
    from flexible_llm_sharding_amd import _native
    from flexible_llm_sharding_amd.ops import get_ops
    ops = get_ops(DEV)
    x = torch.zeros(3, 64, dtype=torch.float16, device=DEV)
    rs = torch.tensor([0, 2, 3], dtype=torch.int32, device=DEV)
    dr = torch.tensor([0, -1, -1], dtype=torch.int32, device=DEV)
    for bad in ((x.float(), rs, dr), (x.cpu(), rs, dr), (x[0], rs, dr), (x, rs.long(), dr), (x, rs, dr[:2]),
                (x, rs.cpu(), dr), (x, rs, dr.long())):
        with pytest.raises(TypeError):
            ops.verify_rows(*bad)
    tok, accept, keep, n_kept = ops.verify_rows(x, rs, dr)       # all-zero rows: token 0, the draft of 0 accepted
    assert tok.tolist() == [0, 0, 0] and accept.tolist() == [1, 0] and keep.tolist() == [0, 1, 2] and n_kept.item() == 3
    # the C entry point refuses bad sizes (no launch); a row range outside the rows is cut to them
    k = _native.kernels()
    out = torch.full((16,), -7, dtype=torch.int32, device=DEV)

    def call(ld, rows, V, n):
        return k.fls_verify_rows(x.data_ptr(), ld, rows, V, rs.data_ptr(), n, dr.data_ptr(), out[0:3].data_ptr(),
                                 out[3:5].data_ptr(), out[5:8].data_ptr(), out[8:9].data_ptr(), None)
    assert call(64, 3, 0, 2) != 0 and call(32, 3, 64, 2) != 0 and call(64, -1, 64, 2) != 0 and call(64, 3, 64, -1) != 0
    torch.cuda.synchronize()
    assert (out == -7).all()
    wild = torch.tensor([-5, 2, 900], dtype=torch.int32, device=DEV)
    assert k.fls_verify_rows(x.data_ptr(), 64, 3, 64, wild.data_ptr(), 2, dr.data_ptr(), out[0:3].data_ptr(),
                             out[3:5].data_ptr(), out[5:8].data_ptr(), out[8:9].data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert out[:9].tolist() == [0, 0, 0, 1, 0, 0, 1, 2, 3] and (out[9:] == -7).all()


# ------------------------------------------------------------------ engine
MODES = {
    "resident": {},
    "streamed": {"resident": False},
    "capped_host_caches": {"resident": False, "max_vram_gb": 40},
    # (what --suffix_kv_cache auto gives under a cap: every call recomputes the suffixes and scores
    # their trailing rows in the pruned last layer)
    "capped_prefix_cache_only": {"resident": False, "max_vram_gb": 40, "suffix_kv_cache": False},
    "score_top_k": {"top_k": 5},
}
_WORLD = {}


def _world(tiny_model, mode):
    """(setup, the plain run of this mode, the continuation table), once per mode (read-only
    afterwards); the prompts' plain continuation holds only ordinary words."""
    if mode not in _WORLD:
        for seed in range(21, 29):
            setup = lr.engine_setup(tiny_model, seed)
            plain = lr.generate(setup, DEV, **MODES[mode])
            if not lr.has_special(plain):
                _WORLD[mode] = (setup, plain, lr.continuation_table(setup, plain))
                break
        else:
            raise AssertionError("no prompt seed gives a continuation of ordinary words")
    return _WORLD[mode]


def _bitwise_equal(plain, got, top_k):
    assert got.updated == plain.updated
    assert len(got.scores) == len(plain.scores)
    for a, b, ta, tb in zip(plain.scores, got.scores, plain.tokens, got.tokens):
        assert a.shape == b.shape and a.dtype == b.dtype
        if top_k:
            assert np.array_equal(a["id"], b["id"])
            assert np.array_equal(a["p"].view(np.uint16), b["p"].view(np.uint16))
        else:
            assert np.array_equal(a.view(np.uint16), b.view(np.uint16))
        assert np.array_equal(ta, tb)
    if top_k:
        for k in ("token_ids", "token_probs"):
            for x, y in zip(plain.record[k], got.record[k]):
                assert x.dtype == y.dtype and np.array_equal(x.view(np.uint16) if k == "token_probs" else x,
                                                             y.view(np.uint16) if k == "token_probs" else y)


def _drafter(name, setup, plain, table):
    V = setup[0].vocab_size
    return {"oracle": lambda: lr.oracle_drafter(table), "wrong_at_0": lambda: lr.wrong_at(table, 0, V),
            "wrong_at_2": lambda: lr.wrong_at(table, 2, V), "wrong_at_3": lambda: lr.wrong_at(table, 3, V),
            "all_wrong": lambda: lr.all_wrong(table, V)}[name]()


@gpu
@needs_gpu
@pytest.mark.parametrize("drafter", ["oracle", "wrong_at_0", "wrong_at_2", "wrong_at_3", "all_wrong"])
@pytest.mark.parametrize("mode", list(MODES))
def test_engine_lookup_bitwise_equals_plain(tiny_model, mode, drafter):
    """2 prompts x 3 suffixes of different lengths, 8 tokens, D = 4: scores bitwise equal and
    tokens equal to the plain run of the same mode."""
    setup, plain, table = _world(tiny_model, mode)
    kw = MODES[mode]
    top_k = kw.get("top_k", 0)
    got = lr.generate(setup, DEV, lookup=lr.D, drafter=_drafter(drafter, setup, plain, table), **kw)
    print(mode, drafter, got.stats, got.calls)
    _bitwise_equal(plain, got, top_k)
    V, n_sfx = setup[0].vocab_size, 6
    assert got.stats["lookup_dropped_roundtrip"] == 0
    row_bytes = (6 * top_k + 6) if top_k else (2 * V + 4)       # a row's scores and its token
    _check_calls(got, mode)
    drafted = [c for c in got.calls if c["drafted"]]
    assert drafted and all(c["d2h"] == c["kept"] * row_bytes for c in drafted), got.calls
    assert all(c["graph"] == 0 for c in drafted)                 # drafted calls run eagerly
    if drafter == "oracle":
        assert got.stats["lookup_calls"] == 2 == len(got.calls)
        assert got.stats["lookup_drafted"] == got.stats["lookup_accepted"] == n_sfx * (lr.NUM_GEN - 2)
        assert [c["kept"] for c in got.calls] == [n_sfx * 5, n_sfx * 3] == [c["rows"] for c in got.calls]
    elif drafter == "all_wrong":
        assert got.stats["lookup_accepted"] == 0 and got.stats["lookup_drafted"] > 0
        assert got.stats["lookup_calls"] == lr.NUM_GEN
        assert all(c["kept"] == n_sfx and c["rows"] > c["kept"] for c in drafted)
    else:
        j = int(drafter[-1])
        assert got.calls[0]["rows"] == n_sfx * 5 and got.calls[0]["kept"] == n_sfx * (j + 1)
        assert got.stats["lookup_calls"] == {0: lr.NUM_GEN, 2: 3, 3: 2}[j]


def _check_calls(got, mode):
    """Every drafted call: kept rows, accepted counts (``runner.last_accept``) and D2H bytes agree;
    under a cap the K/V caches were in host memory and staged through HBM."""
    kw = MODES[mode]
    top_k = kw.get("top_k", 0)
    V = 512
    row_bytes = (6 * top_k + 6) if top_k else (2 * V + 4)
    for c in got.calls:
        if c["drafted"]:
            assert all(0 <= a <= n for a, n in zip(c["accept"], c["n_draft"])), c
            assert c["rows"] == sum(c["n_draft"]) + len(c["n_draft"]) and c["kept"] == sum(c["accept"]) + len(c["accept"])
            assert c["d2h"] == c["kept"] * row_bytes and c["graph"] == 0, c
    assert sum(sum(c["accept"]) for c in got.calls if c["drafted"]) == got.stats["lookup_accepted"]
    assert got.stats["lookup_retokenized"] == 0
    if kw.get("max_vram_gb"):
        assert got.cache["host"] and not got.cache["on_device"], got.cache
        assert got.cache["staged_h2d"] > 0 and got.cache["staged_d2h"] > 0, got.cache
        assert got.cache["suffix_reuse"] == kw.get("suffix_kv_cache", True)
    else:
        assert not got.cache["host"] and got.cache["on_device"], got.cache


@gpu
@needs_gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_engine_early_finish_rides_along(tiny_model, mode):
    """Suffix 0 of each prompt is drafted by the oracle and finishes after two calls; the others get
    no draft.  Ragged calls: draft lengths 4 and 0 side by side, then a finished suffix riding along
    (resident: those later calls, without any draft, replay decode graphs)."""
    setup, plain, table = _world(tiny_model, mode)
    kw = MODES[mode]
    got = lr.generate(setup, DEV, lookup=lr.D, drafter=lr.only_first_suffix(table, setup), **kw)
    _bitwise_equal(plain, got, kw.get("top_k", 0))
    _check_calls(got, mode)
    assert got.stats["lookup_calls"] == lr.NUM_GEN and got.stats["lookup_dropped_roundtrip"] == 0
    assert got.stats["lookup_drafted"] == got.stats["lookup_accepted"] == 2 * (lr.NUM_GEN - 2)
    assert [c["drafted"] for c in got.calls] == [True, True] + [False] * (lr.NUM_GEN - 2)
    assert got.calls[0]["n_draft"] == [4, 0, 0, 4, 0, 0] == got.calls[0]["accept"]
    assert got.calls[1]["n_draft"] == [2, 0, 0, 2, 0, 0] == got.calls[1]["accept"]
    if mode == "resident":
        assert got.calls[-1]["graph"] >= 1


@gpu
@needs_gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_engine_real_drafter(tiny_model, mode):
    """The real drafter on prompts whose prefix holds the plain continuation of every suffix: ragged
    draft lengths and accepted counts per suffix, bitwise the plain run of the same prompts and mode."""
    setup, plain, table = _world(tiny_model, mode)
    kw = MODES[mode]
    key = ("repeat", mode)
    if key not in _WORLD:
        prompts = lr.repeat_prompts(setup, plain)
        _WORLD[key] = (prompts, lr.generate(setup, DEV, prompts=prompts, **kw))
    prompts, plain2 = _WORLD[key]
    got = lr.generate(setup, DEV, lookup=lr.D, prompts=prompts, **kw)
    print(mode, "real drafter:", got.stats, [(c["n_draft"], c["accept"]) for c in got.calls if c["drafted"]])
    _bitwise_equal(plain2, got, kw.get("top_k", 0))
    _check_calls(got, mode)
    assert got.stats["lookup_drafted"] > 0 and got.stats["lookup_calls"] <= lr.NUM_GEN
    # the calls are ragged: draft lengths or accepted counts differ between the suffixes of a call
    assert any(len(set(c["n_draft"])) > 1 or len(set(c["accept"])) > 1 for c in got.calls if c["drafted"])


@gpu
@needs_gpu
@pytest.mark.parametrize("V", [97, 49155, 512])
def test_kept_rows_gather_for_any_vocabulary(tiny_model, V):
    """The kept rows of a vocabulary that is no multiple of 8 (Granite: 49,155) cannot go through the
    16-byte row copy: they are gathered all the same, entry for entry."""
    from flexible_llm_sharding_amd.engine import ShardedRunner
    cfg, tok, _, src = lr.engine_setup(tiny_model)
    r = ShardedRunner(cfg, src, DEV, tok, prefix_kv_cache=True, suffix_kv_cache=True, resident=True)
    try:
        x = torch.rand(11, V, device=DEV).half()
        idx = torch.tensor([0, 3, 4, 10, 7], dtype=torch.int32, device=DEV)
        got = r.out.gather_kept(x, idx)
        torch.cuda.synchronize()
        assert tuple(got.shape) == (5, V) and got.is_contiguous()
        assert torch.equal(got.cpu(), x.cpu()[idx.cpu().long()])
    finally:
        r.close()
