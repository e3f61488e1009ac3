"""runtime/outputs.py on the torch backend: the compact scores (``score_top_k``) survive the trip
start -> collect entry for entry, split per prompt; a drafted micro-batch's kept rows go through the
same unpacking; and a new call's results record starts from nothing, whatever the last call left."""
import dataclasses
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topk_ref as tr  # noqa: E402

from flexible_llm_sharding_amd.ops import get_ops  # noqa: E402
from flexible_llm_sharding_amd.runtime.outputs import CallResults, Outputs  # noqa: E402
from flexible_llm_sharding_amd.topk import TOPK_DTYPE  # noqa: E402

CPU = torch.device("cpu")
V = 97
# rows -> suffixes per prompt (5 rows: two prompts with different suffix counts)
SPLITS = {0: [], 1: [1], 5: [2, 3]}


class Batch(SimpleNamespace):
    """The fields of a PackedBatch the output path reads."""

    def device_tensors(self, dev):
        return {"row_start": torch.from_numpy(self.row_start), "draft": torch.from_numpy(self.draft)}


def _batch(n_suffix, **kw):
    # prompt ids in reverse, so a result stored by position instead of by prompt id shows
    return Batch(prompt_ids=list(range(len(n_suffix)))[::-1], n_suffix=list(n_suffix), draft=None, **kw)


def _outputs(K):
    return Outputs("next_token", K, None, None, get_ops(CPU), CPU, lambda: None, None)


def _probs(rows, seed):
    p = torch.rand(rows, V, generator=torch.Generator().manual_seed(seed)).half()
    return p, p.numpy()


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("rows", [0, 1, 5])
def test_compact_scores_round_trip(rows, K):
    out, batch = _outputs(K), _batch(SPLITS[rows])
    probs, f = _probs(rows, 10 * rows + K)
    pend = out.start(batch, probs, 0, None)
    assert [tuple(h.shape) for h in pend.host] == [(rows, K), (rows,), (rows, K), (rows,)]
    assert [h.dtype for h in pend.host] == [torch.int32, torch.int32, torch.float16, torch.float16]
    res = CallResults.begin([None] * len(batch.n_suffix))
    out.collect([pend], res)
    assert res.d2h_bytes == rows * (6 * K + 6)
    r = 0
    for pid, ns in zip(batch.prompt_ids, batch.n_suffix):
        o, tok, pv = res.outputs[pid], res.tokens[pid], res.token_probs[pid]
        assert o.dtype == TOPK_DTYPE and o.shape == (ns, 1, K)
        ids, vals = tr.ref_topk(f[r:r + ns], K)
        assert np.array_equal(o["id"][:, 0, :], ids) and np.array_equal(o["p"][:, 0, :].view(np.uint16), vals)
        assert tok.dtype == np.int64 and tok.shape == (ns, 1)
        assert np.array_equal(tok[:, 0], f[r:r + ns].astype(np.float32).argmax(-1))
        assert pv.dtype == np.float16 and pv.shape == (ns, 1)
        assert np.array_equal(pv[:, 0].view(np.uint16), tr.ref_picked(f[r:r + ns], tok[:, 0]))
        r += ns
    assert r == rows and res.accept == [None] * len(batch.n_suffix) and res.lookup_rows == res.lookup_kept == 0


def _drafted(K):
    """Two prompts (1 and 2 suffixes) scoring 3, 1 and 2 rows: the first suffix's two draft tokens
    are right, the last suffix's one is wrong -> (outputs, batch, the rows' scores, collected)."""
    out = _outputs(K)
    probs, f = _probs(6, 7)
    am = f.astype(np.float32).argmax(-1)
    draft = np.asarray([am[0], am[1], -1, -1, (am[4] + 1) % V, -1], dtype=np.int32)
    batch = _batch([1, 2], row_start=np.asarray([0, 3, 4, 6], dtype=np.int32))
    batch.draft = draft
    res = CallResults.begin([None, None])
    out.collect([out.start(batch, probs, 0, None)], res)
    return batch, f, res


@pytest.mark.parametrize("K", [0, 3])
def test_drafted_rows_share_the_unpacking(K):
    batch, f, res = _drafted(K)
    assert res.lookup_rows == 6 and res.lookup_kept == 5
    assert res.d2h_bytes == (5 * (6 * K + 6) if K else 5 * (2 * V + 4))
    kept = {1: [[0, 1, 2]], 0: [[3], [4]]}             # prompt id -> per suffix its kept rows
    want_accept = {1: [2], 0: [0, 0]}
    for pid, per_sfx in kept.items():
        assert np.array_equal(res.accept[pid], want_accept[pid]) and res.accept[pid].dtype == np.int64
        for s, rows in enumerate(per_sfx):
            o, tok = res.outputs[pid][s], res.tokens[pid][s]
            assert np.array_equal(tok, f[rows].astype(np.float32).argmax(-1)) and tok.dtype == np.int64
            if K:
                ids, vals = tr.ref_topk(f[rows], K)
                assert o.dtype == TOPK_DTYPE and o.shape == (len(rows), K)
                assert np.array_equal(o["id"], ids) and np.array_equal(o["p"].view(np.uint16), vals)
                assert np.array_equal(res.token_probs[pid][s].view(np.uint16), tr.ref_picked(f[rows], tok))
            else:
                assert o.dtype == np.float16 and np.array_equal(o, f[rows])
        if not K:
            assert res.token_probs[pid] is None


def test_a_new_call_resets_every_field():
    """After a drafted call every field of the record holds something; the next call's record
    holds nothing of it, and the runner's public attributes follow the record."""
    from flexible_llm_sharding_amd.engine import ShardedRunner
    _, _, old = _drafted(3)
    old.token_logprobs, old.pair_lens = [[np.zeros(2, np.float32)]] * 2, [[2], [1, 1]]
    blank = CallResults()
    for f in dataclasses.fields(CallResults):
        assert getattr(old, f.name) != getattr(blank, f.name), f.name       # the drafted call set it
    tps = [SimpleNamespace(suffixes=[[1, 2]]), SimpleNamespace(suffixes=[[3], [4, 5, 6]]), SimpleNamespace(suffixes=[])]
    new = CallResults.begin(tps)
    want = {"outputs": [None] * 3, "tokens": [None] * 3, "token_probs": [None] * 3, "accept": [None] * 3,
            "token_logprobs": [], "d2h_bytes": 0, "lookup_rows": 0, "lookup_kept": 0, "pair_lens": None}
    assert {f.name for f in dataclasses.fields(CallResults)} == set(want)
    for name, v in want.items():
        assert getattr(new, name) == v, name
        assert not isinstance(v, list) or all(getattr(new, name) is not getattr(new, o) for o in want if o != name)
    ll = CallResults.begin(tps, loglik=True)
    assert ll.token_logprobs == [None] * 3 and ll.pair_lens == [[2], [1, 3], []]
    runner = SimpleNamespace()
    for res in (old, new):
        assert ShardedRunner._publish(runner, res) is res.outputs
        assert runner.last_tokens is res.tokens and runner.last_token_probs is res.token_probs
        assert runner.last_accept is res.accept and runner.last_token_logprobs is res.token_logprobs
        assert (runner.score_d2h_bytes, runner.lookup_rows, runner.lookup_kept) == (res.d2h_bytes, res.lookup_rows,
                                                                                   res.lookup_kept)
    assert runner.last_accept == [None] * 3 and runner.lookup_rows == runner.lookup_kept == 0
