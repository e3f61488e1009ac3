"""Prompt-lookup speculative generation (``--lookup_decoding D``): the host side.

No draft model: the next tokens of a suffix are guessed from its own text.  :func:`lookup_draft`
finds the latest earlier occurrence of the text's last n-gram and proposes the tokens that followed
it; one call of the model then scores the suffix's last token and every draft token
(``ShardedRunner.run_tokenized(..., drafts=...)``), and :func:`verify_rows` — the host definition of
``ops.verify_rows`` / the ``fls_verify_rows`` kernel (``csrc/kernels/lookup.hip``) — keeps the draft
tokens the greedy decoding would have produced itself.  Only the kept rows are copied to the host and
split back into suffixes (``runtime/outputs.py``, ``Outputs._start_drafted``).

With the prefix K/V cache every call is row-exact (``engine.py`` "exact K/V reuse"): a row's scores
do not depend on the rows that share its call, so the scores of an accepted draft position are bit
for bit those of the one-token-per-call loop, and a run with the flag writes the same files in fewer
calls.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np

MAX_DRAFT = 16      # --lookup_decoding: 0 (off) or 1..MAX_DRAFT draft tokens per suffix per call
MAX_NGRAM = 8       # --lookup_ngram: 1..MAX_NGRAM, the longest n-gram tried
DEFAULT_NGRAM = 3


def check_lookup_values(d, n=DEFAULT_NGRAM) -> Tuple[int, int]:
    """(D, N) as ints, or a ``ValueError`` naming the flag."""
    if isinstance(d, bool) or not isinstance(d, (int, np.integer)) or not 0 <= int(d) <= MAX_DRAFT:
        raise ValueError(f"--lookup_decoding must be 0 (off) or an integer in 1..{MAX_DRAFT}, got {d!r}")
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= int(n) <= MAX_NGRAM:
        raise ValueError(f"--lookup_ngram must be an integer in 1..{MAX_NGRAM}, got {n!r}")
    return int(d), int(n)


def lookup_draft(tokens: Sequence[int], n_max: int, d: int) -> np.ndarray:
    """Up to ``d`` draft tokens for the text ``tokens`` (prefix + suffix + generated so far).

    For n = ``n_max`` .. 1: take the last n tokens, find their LATEST earlier occurrence that is
    followed by at least one token, and return up to ``d`` of the tokens after it; the first n
    that matches decides.  An empty array when none does.  Pure and deterministic."""
    t = np.asarray(tokens, dtype=np.int64).reshape(-1)
    L = int(t.shape[0])
    empty = np.zeros(0, dtype=np.int64)
    if d <= 0 or L < 2:
        return empty
    for n in range(min(int(n_max), L - 1), 0, -1):
        # an occurrence starts at i <= L - n - 1: it ends before the text does, so a token follows
        # it (it may overlap the final n-gram itself)
        hit = t[L - n:]
        ok = np.ones(L - n, dtype=bool)
        for k in range(n):
            ok &= t[k:L - n + k] == hit[k]
        idx = np.flatnonzero(ok)
        if idx.size:
            s = int(idx[-1]) + n
            return t[s:s + int(d)].copy()
    return empty


def verify_rows(probs: np.ndarray, row_start: np.ndarray, draft: np.ndarray):
    """The host definition of ``ops.verify_rows``.

    ``probs``: [R, V] fp16 probabilities; ``row_start``: [n_sfx + 1] first row of every suffix
    (suffix i owns rows row_start[i] .. row_start[i + 1] - 1: its last token, then one row per
    draft token); ``draft``: [R] int32, the draft token scored NEXT to each row (row j of a suffix
    predicts draft j), -1 on each suffix's last row.

    -> (tok [R] int32, accept [n_sfx] int32, keep [n_kept] int32): each row's greedy id (largest
    fp16 bit pattern, first index on ties: ``argmax_rows``), per suffix the number of leading rows
    whose greedy id equals their draft token, and the kept rows — rows 0 .. accept of every suffix
    — in suffix order."""
    p = np.ascontiguousarray(probs)
    if p.dtype != np.float16:
        p = p.astype(np.float16)
    tok = np.argmax(p.view(np.uint16), axis=1).astype(np.int32) if p.shape[0] else np.zeros(0, np.int32)
    rs = np.asarray(row_start, dtype=np.int64)
    dr = np.asarray(draft, dtype=np.int32)
    n = rs.shape[0] - 1
    accept = np.zeros(n, dtype=np.int32)
    keep = []
    for i in range(n):
        a, r0, r1 = 0, int(rs[i]), int(rs[i + 1])
        while r0 + a < r1 - 1 and tok[r0 + a] == dr[r0 + a]:
            a += 1
        accept[i] = a
        keep.extend(range(r0, r0 + a + 1) if r1 > r0 else ())
    return tok, accept, np.asarray(keep, dtype=np.int32)
