"""Oracle and cases for the compact next-token scores (``--score_top_k``).

The oracle is written from the definition alone (``flexible_llm_sharding_amd/topk.py``'s docstring)
and shares no code with the package: clamp the keys, take a stable argsort of the negated int32
keys, keep the first K.  ``mutant`` switches on one deliberate mistake, for the test that the cases
discriminate:

* ``"tie_order"``    equal keys ranked by index descending
* ``"raw_invalid"``  bit patterns above 0x3C00 ranked by their raw bits instead of with the zeros

A case is one kernel launch: a matrix of rows from every family (``Case.family[r]`` names row r's),
a K, a device layout (row stride, base offset) and the picked ids.
"""
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

ONE = 0x3C00
INVALID = (0x3C01, 0x7C00, 0x7E00, 0x8000, 0x8400, 0xFFFF)
KS = (1, 2, 5, 64, 1000, 1024)


def ref_keys(bits: np.ndarray, mutant: Optional[str] = None) -> np.ndarray:
    bits = np.asarray(bits, dtype=np.uint16).astype(np.int32)
    return bits if mutant == "raw_invalid" else np.where(bits <= ONE, bits, 0)


def ref_order(scores: np.ndarray, mutant: Optional[str] = None) -> np.ndarray:
    """[rows, V] column indices in rank order (key descending, index ascending)."""
    key = ref_keys(np.ascontiguousarray(scores, dtype=np.float16).view(np.uint16), mutant)
    if mutant == "tie_order":
        V = key.shape[1]
        return V - 1 - np.argsort(-key[:, ::-1], axis=1, kind="stable")
    return np.argsort(-key, axis=1, kind="stable")


def ref_topk(scores: np.ndarray, K: int, mutant: Optional[str] = None, order: Optional[np.ndarray] = None):
    """(ids int32 [rows, K], vals uint16 [rows, K]) of fp16 ``scores`` ([rows, V])."""
    order = ref_order(scores, mutant) if order is None else order
    ids = order[:, :K].astype(np.int32)
    key = ref_keys(np.ascontiguousarray(scores, dtype=np.float16).view(np.uint16), mutant)
    return ids, np.take_along_axis(key, ids.astype(np.int64), axis=1).astype(np.uint16)


def ref_picked(scores: np.ndarray, picked: np.ndarray) -> np.ndarray:
    """uint16 [rows]: the key of entry picked[r] of row r, 0 for an id outside the row."""
    bits = np.ascontiguousarray(scores, dtype=np.float16).view(np.uint16)
    out = np.zeros(len(bits), dtype=np.uint16)
    for r, p in enumerate(np.asarray(picked).tolist()):
        if 0 <= p < bits.shape[1]:
            out[r] = bits[r, p] if bits[r, p] <= ONE else 0
    return out


# ------------------------------------------------------------------ cases
@dataclass
class Case:
    name: str
    scores: np.ndarray            # [rows, V] float16
    K: int
    family: List[str]             # per row
    picked: Optional[np.ndarray] = None   # [rows] int32 (ids outside [0, V) included), or None
    ld: int = 0                   # row stride on the device (0: V)
    offset: int = 0               # elements the device base is moved by (1: no 16-byte alignment)
    _order: dict = field(default_factory=dict)

    @property
    def V(self) -> int:
        return self.scores.shape[1]

    def want(self, mutant: Optional[str] = None):
        if mutant not in self._order:
            self._order[mutant] = ref_order(self.scores, mutant)
        return ref_topk(self.scores, self.K, mutant, self._order[mutant])

    def want_picked(self) -> Optional[np.ndarray]:
        return None if self.picked is None else ref_picked(self.scores, self.picked)

    def valid_rows(self) -> np.ndarray:
        """Rows without a bit pattern above 0x3C00."""
        return ~(self.scores.view(np.uint16) > ONE).any(axis=1)


def _softmax_rows(rng, rows, V, scale):
    x = rng.standard_normal((rows, V)) * scale
    e = np.exp(x - x.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True)).astype(np.float16).view(np.uint16)


def wave_parts(V: int):
    """First column of each wave's contiguous part of a row, in both load widths."""
    starts = set()
    for units, width in ((V // 8, 8), (V, 1)):
        per = -(-units // 4)
        starts.update(min(V - 1, w * per * width) for w in range(4))
    return sorted(starts)


def tie_columns(V: int) -> List[int]:
    """Where the last kept occurrence of the threshold key is put: the row's ends, a lane's
    boundary, and the middle and both sides of the start of every wave part."""
    cols = {0, 7, 8, V - 1}
    for s in wave_parts(V):
        cols.update((s - 1, s, s + (V // 8)))
    return sorted(c for c in cols if 0 <= c < V)


def tie_row(rng, V: int, K: int, last: int, t: int) -> np.ndarray:
    """A row whose K-th ranked entry is the occurrence of key ``t`` at column ``last``: K - need
    entries above ``t``, ``need`` occurrences of ``t`` up to ``last`` and (where columns are left)
    more of them behind it, in every wave part; everything else below ``t``."""
    need = min(K, last + 1, max(1, K - K // 2))
    above = K - need
    row = np.zeros(V, dtype=np.uint16)
    free = np.ones(V, dtype=bool)
    kept = np.append(rng.choice(last, need - 1, replace=False), last).astype(np.int64) if need > 1 else np.array([last])
    free[kept] = False
    behind = np.arange(last + 1, V)
    n_more = min(40, len(behind), V - need - above)
    more = rng.choice(behind, n_more, replace=False) if n_more > 0 else np.array([], dtype=np.int64)
    free[more] = False
    rest = np.flatnonzero(free)
    up = rng.choice(rest, above, replace=False) if above else np.array([], dtype=np.int64)
    free[up] = False
    row[kept] = t
    row[more] = t
    if above:
        row[up] = rng.integers(t + 1, ONE + 1, above) if t < ONE else ONE
    low = np.flatnonzero(free)
    if t > 1 and len(low):
        row[low] = np.where(rng.random(len(low)) < 0.5, 0, rng.integers(1, t, len(low)))
    return row


def family_rows(rng, V: int, K: int, small: bool = False):
    """(bits [rows, V] uint16, family names) for one (V, K): every family of the issue; ``small``
    keeps 8 rows (the large vocabularies)."""
    rows, fam = [], []

    def add(name, r):
        rows.append(np.asarray(r, dtype=np.uint16))
        fam.append(name)

    sm = _softmax_rows(rng, 2, V, 4.0)
    add("random", sm[0])
    add("random", _softmax_rows(rng, 1, V, 1.0)[0])
    add("flat", np.full(V, np.float16(1.0 / V).view(np.uint16)))
    add("zero", np.zeros(V))
    hot = np.zeros(V)
    hot[V // 3] = ONE
    add("onehot", hot)
    few = np.zeros(V, dtype=np.uint16)
    n_few = K - 1 if K > 1 else 0
    few[rng.choice(V, n_few, replace=False)] = rng.integers(1, ONE + 1, n_few)
    add("few", few)
    parts = wave_parts(V)
    add("ties", tie_row(rng, V, K, min(V - 1, parts[-1] + 11), 0x2E66))
    bad = sm[1].copy()
    at = rng.choice(V, min(V, 64), replace=False)
    bad[at] = [INVALID[i % len(INVALID)] for i in range(len(at))]
    bad[0], bad[V - 1] = INVALID[K % 6], INVALID[(K + 1) % 6]
    add("invalid", bad)
    if small:
        return np.stack(rows), fam
    # the remaining families: on the small vocabularies only
    for c in tie_columns(V):
        add("ties", tie_row(rng, V, K, c, int(rng.integers(0x0400, 0x3000))))
    for t in (1, 63, 64, 128, 251):                    # threshold bin on a thread-chunk boundary of the scan
        for b in (ONE - 61 * t + 1, ONE - 61 * t, ONE - 61 * t - 1):
            add("scan", tie_row(rng, V, K, int(rng.integers(V // 2, V)), b))
    add("scan", tie_row(rng, V, K, V - 1, ONE))         # the threshold is 1.0 itself
    add("scan", tie_row(rng, V, K, V // 2, 1))          # ... and the smallest subnormal
    sub = rng.integers(0, 0x400, V).astype(np.uint16)   # zeros and subnormals only
    add("subnormal", sub)
    sub2 = np.zeros(V, dtype=np.uint16)
    n = min(V, K + 7)
    sub2[rng.choice(V, n, replace=False)] = rng.integers(1, 0x400, n)
    add("subnormal", sub2)
    add("invalid", [INVALID[i % len(INVALID)] for i in range(V)])          # nothing valid: ids 0 .. K-1
    only = np.full(V, 0x7E00, dtype=np.uint16)
    only[V // 2] = 0x2000
    add("invalid", only)
    mixed = rng.integers(0, 0x10000, V).astype(np.uint16)                    # any bit pattern at all
    add("invalid", mixed)
    few0 = np.zeros(V, dtype=np.uint16)
    few0[V - 1] = 0x0001
    add("few", few0)
    few_half = np.zeros(V, dtype=np.uint16)
    few_half[rng.choice(V, K // 2, replace=False)] = 0x3000
    add("few", few_half)
    for c in (0, 7, 8, V - 1):
        hot = np.zeros(V)
        hot[c] = 0x0001 if c % 2 else ONE
        add("onehot", hot)
    # K distinct keys (the sort alone): every entry distinct where the keys suffice
    n = min(V, K + 200)
    d = np.zeros(V, dtype=np.uint16)
    d[rng.choice(V, n, replace=False)] = rng.choice(np.arange(1, ONE + 1), n, replace=False)
    add("distinct", d)
    dd = np.zeros(V, dtype=np.uint16)                    # descending and ascending runs
    dd[:n] = np.sort(rng.choice(np.arange(1, ONE + 1), n, replace=False))
    add("distinct", dd)
    add("distinct", dd[::-1])
    # 1,024 candidates (or the whole row) in one bin: the compaction alone
    ob = rng.integers(0, 0x1000, V).astype(np.uint16)
    n = min(V, 1500)
    ob[rng.choice(V, n, replace=False)] = 0x3555
    add("onebin", ob)
    return np.stack(rows), fam


def _picked(rng, rows: int, V: int) -> np.ndarray:
    p = rng.integers(0, V, rows).astype(np.int32)
    for r, v in enumerate((0, V - 1, V, -1, 1 << 30)):
        if r < rows:
            p[r] = v
    return p


_CASES: List[Case] = []


def kernel_cases() -> List[Case]:
    """Built once and shared (the oracle's order is cached on each case); never modified."""
    if _CASES:
        return _CASES
    rng = np.random.default_rng(20240917)
    out: List[Case] = []
    for V, ks, small in ((97, (1, 2, 5, 64, 97), False), (2056, KS, False), (32000, (5, 1024), True),
                         (151936, (1, 64, 1000), True)):
        for i, K in enumerate(ks):
            bits, fam = family_rows(rng, V, K, small)
            picked = None if (i == 1 and not small) else _picked(rng, len(bits), V)
            out.append(Case(f"V{V}_K{K}", bits.view(np.float16), K, fam, picked))
    # layouts: a row stride > V on the vector and the scalar path, a base that breaks 16-byte alignment
    for name, V, K, kw in (("stride_vec", 2056, 5, {"ld": 2056 + 24}), ("stride_scalar", 2056, 64, {"ld": 2056 + 3}),
                           ("stride_V97", 97, 97, {"ld": 128}), ("offset_one", 2056, 1000, {"offset": 1}),
                           ("offset_one_V32000", 32000, 2, {"offset": 1})):
        bits, fam = family_rows(rng, V, K, V > 2056)
        out.append(Case(name, bits.view(np.float16), K, fam, _picked(rng, len(bits), V), **kw))
    # more than one block per CU and a partial last wave of blocks: 300 rows
    bits = _softmax_rows(rng, 300, 2056, 3.0)
    out.append(Case("rows300", bits.view(np.float16), 20, ["random"] * 300, _picked(rng, 300, 2056)))
    _CASES.extend(out)
    return _CASES


# ------------------------------------------------------------------ engine harness
NUM_GEN = 4


def engine_setup(tiny_model):
    """(config, tokenizer, prompts, host weights): the prompts of tests/test_sampling_gpu.py."""
    from flexible_llm_sharding_amd.runtime.weights import HostStore
    from flexible_llm_sharding_amd.utils.synthetic import synthetic_prompts
    from flexible_llm_sharding_amd.utils.tokenizer import load_tokenizer
    path, cfg = tiny_model
    tok = load_tokenizer(path)
    prompts = synthetic_prompts(3, 40, 3, 12, cfg.vocab_size, seed=21, vary=True)
    prompts[1] = (prompts[1][0], prompts[1][1][:2])             # 3, 2 and 3 suffixes
    return cfg, tok, prompts, HostStore.from_model_path(cfg, path)


@dataclass
class Run:
    scores: list                  # per prompt [n_s, steps, V] fp16, or TOPK [n_s, steps, K]
    updated: list
    tokens: list                  # [step][prompt] -> [n_s, 1] int64 (the runner's last_tokens)
    token_probs: list             # [step][prompt] -> [n_s, 1] fp16 or None (last_token_probs)
    stats: list                   # per step
    dropped: int
    record: dict
    d2h: list                     # per step: bytes of scores copied to the host


def generate(setup, device, top_k=0, num_gen=NUM_GEN, sampling=None, env=None, num_batch=1, **kw) -> Run:
    """One generation of ``num_gen`` tokens through api.generation_loop on ``device``."""
    import argparse
    import os

    from flexible_llm_sharding_amd.api import generation_loop
    from flexible_llm_sharding_amd.engine import ShardedRunner
    from flexible_llm_sharding_amd.parallel.comm import Comm
    from flexible_llm_sharding_amd.sampling import SamplingParams
    cfg, tok, prompts, src = setup

    class Recording(ShardedRunner):
        def __call__(self, ps):
            out = super().__call__(ps)
            self.seen.append(([None if t is None else t.copy() for t in self.last_tokens],
                              [None if t is None else t.copy() for t in self.last_token_probs], dict(self.stats),
                              self.score_d2h_bytes))
            return out

    args = argparse.Namespace(num_gen_token=num_gen, data_parallel=False, num_batch=num_batch,
                              do_sample=sampling is not None, **(sampling or {}))
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        base = dict(layer_num_per_shard=1, prefix_kv_cache=True, suffix_kv_cache=True, resident=True)
        base.update(kw)
        r = Recording(cfg, src, device, tok, sampling=SamplingParams.from_args(args), score_top_k=top_k, **base)
        r.seen = []
        rec: dict = {}
        scores, updated = generation_loop(args, r, Comm(), tok, prompts, token_record=rec)
        assert r._spec is None
        seen, dropped = r.seen, r.spec_dropped
        r.close()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    return Run(scores, updated, [s[0] for s in seen], [s[1] for s in seen], [s[2] for s in seen], dropped, rec,
               [s[3] for s in seen])


def check_compact_run(full: Run, got: Run, K: int, per_call_tokens: bool = True) -> None:
    """``got`` (score_top_k = K) against ``full`` (the same run without the flag): every prompt's
    and step's entries are the oracle applied to the full scores; the tokens, their probabilities
    (read from the full scores with the oracle's clamp) and the updated prompts are equal."""
    assert got.updated == full.updated
    assert len(got.scores) == len(full.scores)
    for p, (o, f) in enumerate(zip(got.scores, full.scores)):
        n_s, steps, V = f.shape
        assert o.dtype == np.dtype([("id", "<i4"), ("p", "<f2")]) and o.shape == (n_s, steps, K), (o.dtype, o.shape)
        for t in range(steps):
            ids, vals = ref_topk(f[:, t, :], K)
            assert np.array_equal(o["id"][:, t, :], ids), (p, t)
            assert np.array_equal(o["p"][:, t, :].view(np.uint16), vals), (p, t)
        toks = got.record["token_ids"][p]
        assert toks.dtype == np.int64 and toks.shape == (n_s, steps)
        tp = got.record["token_probs"][p]
        assert tp.dtype == np.float16 and tp.shape == (n_s, steps)
        for t in range(steps):
            assert np.array_equal(tp[:, t].view(np.uint16), ref_picked(f[:, t, :], toks[:, t])), (p, t)
    if per_call_tokens:
        assert len(got.tokens) == len(full.tokens)
        for t, (a, b) in enumerate(zip(got.tokens, full.tokens)):
            for p, (x, y) in enumerate(zip(a, b)):
                assert x is not None and y is not None and np.array_equal(x, y), (t, p)
                assert np.array_equal(got.record["token_ids"][p][:, t:t + 1], x), (t, p)
                assert np.array_equal(got.token_probs[t][p], got.record["token_probs"][p][:, t:t + 1]), (t, p)
