"""Oracles and shared cases of the prompt-lookup decoding tests (tests/test_lookup_cpu.py,
tests/test_lookup_gpu.py): brute-force definitions of the drafter and of the draft verification,
written as plain Python loops and independent of flexible_llm_sharding_amd/lookup.py; the kernel
cases, built once; and the engine harness — prompts, drafters and a recording generation run."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

NUM_GEN = 8
D = 4


# ------------------------------------------------------------------ oracles
def ref_draft(tokens, n_max: int, d: int) -> List[int]:
    """The issue's rule, literally: for n = n_max .. 1 take the last n tokens, find their latest
    earlier occurrence that is followed by at least one token, return up to d tokens after it."""
    t = [int(x) for x in tokens]
    L = len(t)
    if d <= 0:
        return []
    for n in range(n_max, 0, -1):
        if n > L:
            continue
        tail = t[L - n:]
        for start in range(L - n - 1, -1, -1):          # earlier than the tail itself, latest first
            if t[start:start + n] == tail and start + n < L:
                return t[start + n:start + n + d]
    return []


def ref_verify(scores: np.ndarray, row_start, draft):
    """(tok, accept, keep) by plain loops: the greedy id of a row is the first index of its
    largest fp16 bit pattern; a suffix accepts its leading rows whose id equals their draft token;
    rows 0 .. accept of every suffix are kept, in suffix order."""
    bits = np.ascontiguousarray(scores).view(np.uint16)
    R, V = bits.shape
    tok = np.zeros(R, dtype=np.int32)
    for r in range(R):
        best, bi = -1, 0
        row = bits[r].tolist()
        for c in range(V):
            if row[c] > best:
                best, bi = row[c], c
        tok[r] = bi
    n = len(row_start) - 1
    accept = np.zeros(n, dtype=np.int32)
    keep = []
    for i in range(n):
        r0, r1 = int(row_start[i]), int(row_start[i + 1])
        a = 0
        while a < r1 - r0 - 1 and int(tok[r0 + a]) == int(draft[r0 + a]):
            a += 1
        accept[i] = a
        keep += list(range(r0, r0 + a + 1))
    return tok, accept, np.asarray(keep, dtype=np.int32)


# ------------------------------------------------------------------ kernel cases
@dataclass
class Case:
    name: str
    scores: np.ndarray            # [R, V] fp16
    row_start: np.ndarray         # [n_sfx + 1] int32
    draft: np.ndarray             # [R] int32
    ld: int = 0                   # row stride on the device (0: V)
    offset: int = 0               # elements between a 16-byte boundary and the first row
    want_accept: List[str] = field(default_factory=list)     # per suffix: "zero" | "mid" | "all"
    _want: Optional[tuple] = None

    @property
    def V(self) -> int:
        return self.scores.shape[1]

    def want(self):
        if self._want is None:
            self._want = ref_verify(self.scores, self.row_start, self.draft)
        return self._want


def _fast_tok(scores: np.ndarray) -> np.ndarray:
    return np.argmax(scores.view(np.uint16), axis=1).astype(np.int32)      # (numpy: first index on ties)


def _case(name: str, V: int, counts, seed: int, ld: int = 0, offset: int = 0) -> Case:
    """Rows of sparse fp16 probabilities with ties on the maximum and all-zero rows mixed in, and
    per suffix a draft built for an accepted count of 0, a middle one or all (cycling); after the
    first wrong draft token the later ones are right again, which must not count."""
    rng = np.random.default_rng(seed)
    counts = [int(c) for c in counts]
    R = sum(counts)
    x = (rng.random((R, V), dtype=np.float32) ** 12 * 0.05).astype(np.float16)
    x[rng.random((R, V)) < 0.6] = 0
    for r in range(R):
        kind = r % 7
        if kind == 2:                                    # a tie on the maximum: the first index wins
            cols = np.sort(rng.choice(V, size=3, replace=False))
            x[r, cols] = np.float16(0.25)
        elif kind == 4:
            x[r] = 0                                     # an all-zero row: token 0
        elif kind == 5:                                  # the maximum in the last column (a tail column
            x[r, V - 1] = np.float16(0.5)                # of the 16-byte path when V % 8 != 0)
    tok = _fast_tok(x)
    row_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    draft = np.full(R, -1, dtype=np.int32)
    kinds = []
    for i, c in enumerate(counts):
        r0 = int(row_start[i])
        kind = ("zero", "mid", "all")[i % 3]
        a = {"zero": 0, "mid": (c - 1) // 2, "all": c - 1}[kind]
        draft[r0:r0 + c - 1] = tok[r0:r0 + c - 1]                 # right everywhere ...
        if a < c - 1:
            draft[r0 + a] = (int(tok[r0 + a]) + 1) % V            # ... but at row a
        kinds.append(kind)
    return Case(name, x, row_start, draft, ld, offset, kinds)


_CASES: Optional[List[Case]] = None


def kernel_cases() -> List[Case]:
    global _CASES
    if _CASES is None:
        r17 = list(range(1, 18))
        _CASES = [
            _case("V97_300_suffixes", 97, [1 + (7 * i) % 17 for i in range(300)], 1),
            _case("V97_stride_104", 97, r17, 2, ld=104),
            _case("V97_stride_101", 97, r17, 3, ld=101),
            _case("V2056_vec", 2056, r17, 4),
            _case("V2056_stride_2064", 2056, r17, 5, ld=2064),
            _case("V2056_stride_2059", 2056, [3, 1, 17, 2], 6, ld=2059),
            _case("V2056_offset_1", 2056, [2, 17, 1, 5], 7, offset=1),
            _case("V32000_vec", 32000, [17, 1, 2, 9, 4], 8),
            _case("V32000_offset_1_stride", 32000, [1, 5, 17], 9, ld=32008, offset=1),
            _case("one_suffix_one_row", 97, [1], 10),
        ]
    return _CASES


# ------------------------------------------------------------------ engine harness
@dataclass
class Run:
    scores: list                  # per prompt [n_s, NUM_GEN, V] fp16, or TOPK [n_s, NUM_GEN, K]
    updated: list
    tokens: list                  # per prompt [n_s, NUM_GEN] int64
    stats: dict                   # lookup_calls, lookup_drafted, lookup_accepted, lookup_dropped_roundtrip
    calls: list                   # per runner call: dict(drafted, d2h, rows, kept, graph, accept, n_draft)
    record: dict
    cache: dict = field(default_factory=dict)    # the runner's K/V cache at the end: host mode, staged bytes


def engine_setup(tiny_model, seed: int = 21):
    """(config, tokenizer, prompts, host weights): 2 prompts x 3 suffixes of different lengths.
    Every suffix ends with a space, so ``s + decode(tokens)`` re-tokenizes to the suffix's ids
    followed by the tokens (the word-level tokenizer splits on whitespace)."""
    from flexible_llm_sharding_amd.runtime.weights import HostStore
    from flexible_llm_sharding_amd.utils.synthetic import synthetic_prompts
    from flexible_llm_sharding_amd.utils.tokenizer import load_tokenizer
    path, cfg = tiny_model
    tok = load_tokenizer(path)
    import random

    from flexible_llm_sharding_amd.utils.tokenizer import synthetic_word
    raw = synthetic_prompts(2, 40, 3, 12, cfg.vocab_size, seed=seed, vary=True)
    rng = random.Random(seed)
    prompts = []
    for pi, (pre, _) in enumerate(raw):
        sfx = [" ".join(synthetic_word(rng.randrange(3, cfg.vocab_size)) for _ in range(n + pi)) + " "
               for n in (2, 7, 13)]
        prompts.append((pre, tuple(sfx)))
    return cfg, tok, prompts, HostStore.from_model_path(cfg, path)


def generate(setup, device, lookup: int = 0, drafter=None, top_k: int = 0, num_gen: int = NUM_GEN, ngram: int = 3,
             prompts=None, **kw) -> Run:
    """One greedy generation through api.generation_loop on ``device`` (``lookup``: D)."""
    import argparse

    from flexible_llm_sharding_amd.api import generation_loop, greedy_tokens
    from flexible_llm_sharding_amd.engine import ShardedRunner
    from flexible_llm_sharding_amd.parallel.comm import Comm
    cfg, tok, default_prompts, src = setup
    prompts = default_prompts if prompts is None else prompts

    class Recording(ShardedRunner):
        def run_tokenized(self, tps, drafts=None):
            out = super().run_tokenized(tps, drafts=drafts)
            self.seen.append({"drafted": drafts is not None, "d2h": self.score_d2h_bytes,
                              "rows": self.lookup_rows, "kept": self.lookup_kept,
                              "graph": self.stats.get("graph_replays", 0),
                              # (drafted calls: the accepted count and the draft length of every suffix)
                              "accept": [int(a) for p in self.last_accept for a in p] if drafts is not None else None,
                              "n_draft": [len(d) for p in drafts for d in p] if drafts is not None else None})
            return out

    args = argparse.Namespace(num_gen_token=num_gen, data_parallel=False, num_batch=1, lookup_decoding=lookup,
                              lookup_ngram=ngram)
    base = dict(layer_num_per_shard=1, prefix_kv_cache=True, suffix_kv_cache=True)
    if str(device) != "cpu":
        base["resident"] = True
    base.update(kw)
    r = Recording(cfg, src, device, tok, score_top_k=top_k, **base)
    r.seen = []
    rec: dict = {}
    stats: dict = {}
    try:
        scores, updated = generation_loop(args, r, Comm(), tok, prompts, token_record=rec, drafter=drafter,
                                          lookup_stats=stats)
        seen = r.seen
        pc = r.prefix_cache
        cache = {"host": bool(pc.host), "suffix_reuse": bool(pc.suffix_reuse),
                 "staged_h2d": pc.stage.bytes_h2d if pc.stage is not None else 0,
                 "staged_d2h": pc.stage.bytes_d2h if pc.stage is not None else 0,
                 "direct": pc.stage.bytes_direct if pc.stage is not None else 0,
                 "on_device": any(t.is_cuda for e in pc.entries.values() for t in e.layers.values())} if pc else {}
    finally:
        r.close()
    if top_k:
        tokens = [np.asarray(t) for t in rec["token_ids"]]
    else:
        tokens = [np.asarray(greedy_tokens(s)) for s in scores]
    return Run(scores, updated, tokens, stats, seen, rec, cache)


def has_special(run: Run) -> bool:
    """A generated <unk> / <s> / </s> (ids 0..2): such a token does not survive ``decode`` and
    re-tokenization as one ordinary word, so the prompts are not fit for a draft round trip."""
    return any((t < 3).any() for t in run.tokens)


def continuation_table(setup, plain, prompts=None, gen: int = NUM_GEN) -> dict:
    """ids of (prefix + suffix + the plain run's first g tokens) -> the plain run's tokens from g
    on, for every suffix and g: what a perfect drafter proposes."""
    from flexible_llm_sharding_amd.utils.tokenizer import tokenize_prompts
    cfg, tok, default_prompts, _ = setup
    prompts = default_prompts if prompts is None else prompts
    table = {}
    for g in range(gen):
        ext = [(pre, tuple(s + (tok.decode(plain.tokens[pi][si][:g]) if g else "") for si, s in enumerate(sfx)))
               for pi, (pre, sfx) in enumerate(prompts)]
        for pi, tp in enumerate(tokenize_prompts(tok, ext)):
            for si, ids in enumerate(tp.suffixes):
                table[tuple(tp.prefix) + tuple(ids)] = [int(t) for t in plain.tokens[pi][si][g:]]
    return table


def oracle_drafter(table: dict):
    def draft(tokens, n_max, d):
        return np.asarray(table.get(tuple(int(t) for t in tokens), [])[:d], dtype=np.int64)
    return draft


def wrong_at(table: dict, j: int, vocab: int):
    """The oracle's draft with position j replaced by another ordinary word (ids 3 .. vocab - 1)."""
    def draft(tokens, n_max, d):
        out = list(table.get(tuple(int(t) for t in tokens), [])[:d])
        if j < len(out):
            out[j] = 3 + (out[j] - 3 + 1) % (vocab - 3)
        return np.asarray(out, dtype=np.int64)
    return draft


def all_wrong(table: dict, vocab: int):
    def draft(tokens, n_max, d):
        out = [3 + (t - 3 + 1) % (vocab - 3) for t in table.get(tuple(int(t) for t in tokens), [])[:d]]
        return np.asarray(out, dtype=np.int64)
    return draft


def only_first_suffix(table: dict, setup, prompts=None):
    """The oracle's drafts for suffix 0 of every prompt, none for the others: suffix 0 finishes
    early and rides along while the others still run."""
    from flexible_llm_sharding_amd.utils.tokenizer import tokenize_prompts
    cfg, tok, default_prompts, _ = setup
    prompts = default_prompts if prompts is None else prompts
    heads = []
    for tp in tokenize_prompts(tok, prompts):
        heads.append(tuple(tp.prefix) + tuple(tp.suffixes[0]))

    def draft(tokens, n_max, d):
        key = tuple(int(t) for t in tokens)
        if any(key[:len(h)] == h for h in heads):
            return np.asarray(table.get(key, [])[:d], dtype=np.int64)
        return np.zeros(0, dtype=np.int64)
    return draft


def repeat_prompts(setup, plain: Run):
    """Prompts whose prefix ends with each suffix's last word followed by the plain run's
    continuation of that suffix: the real drafter finds the suffix's tail in the prefix and
    proposes those tokens.  (The longer prefix changes the model's own continuation, so whether
    they are accepted is up to the model: the outputs must equal the plain run either way.)"""
    cfg, tok, prompts, _ = setup
    out = []
    for pi, (pre, sfx) in enumerate(prompts):
        extra = [s.split()[-1] + " " + tok.decode(plain.tokens[pi][si]) for si, s in enumerate(sfx)]
        out.append((pre + " " + " ".join(extra), sfx))
    return out
