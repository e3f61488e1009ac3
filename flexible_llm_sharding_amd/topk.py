"""Compact next-token scores (``--score_top_k K``): the K best entries of each row, integer-exact.

Instead of the whole ``[n_s, 1, V]`` fp16 distribution, a run returns per scored row the K most
probable ``(token id, fp16 probability)`` pairs in rank order, and the id and probability of the
token the engine chose for the row (greedy or sampled).  The probabilities on the device, the chosen
tokens and the updated prompts are those of the same run without the flag.  Device kernel
(``csrc/kernels/topk.hip``), this host implementation and the test oracle return the same entries
for every input.  ``runtime/outputs.py`` packs the entries for the host (``Outputs._compact``) and
splits them back into prompts.

1. A row is V fp16 bit patterns ``b_i``.
2. The key of entry i is ``k_i = b_i`` if ``b_i <= 0x3C00`` (0 to 1.0), else 0: negative, NaN and
   > 1 patterns rank with the zeros, as in the sampler (the softmax kernel never writes them).
3. Entries are ranked by ``(key descending, index ascending)``.
4. The result is the first K ranked entries: ``ids[K]`` (int32) and ``vals[K]`` (uint16, the key
   itself, which read as fp16 is the probability).
5. ``1 <= K <= min(V, 1024)``; every other value is refused.
6. V is limited by int32 indexing only (the sampler's ``V < 2^18`` is the sampler's own).

Consequences: ``ids[0]`` is the greedy token (``fls_argmax_rows``, ``api.greedy_tokens``) of every
row without invalid patterns; an all-zero row gives ids ``0 .. K-1``; a row with fewer than K
non-zero keys is filled with its lowest-index zero-key entries.  The probability of the chosen
token is ``key(b[row, token])``, the same clamp.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

ONE_BITS = 0x3C00                  # fp16 1.0
MAX_K = 1024
# one returned entry; a prompt's output is a [n_s, steps, K] array of these
TOPK_DTYPE = np.dtype([("id", "<i4"), ("p", "<f2")])
_CHUNK_ELEMS = 1 << 22             # rows are processed in chunks of about this many int64 composites


def check_k(K, vocab: Optional[int] = None, flag: str = "--score_top_k") -> int:
    """``K`` as an int in ``1 .. min(vocab, 1024)``; a ``ValueError`` names ``flag``."""
    if isinstance(K, bool) or int(K) != K:
        raise ValueError(f"{flag} must be an integer, got {K!r}")
    K = int(K)
    if not 1 <= K <= MAX_K:
        raise ValueError(f"{flag} must be in 1..{MAX_K}, got {K}")
    if vocab is not None and K > vocab:
        raise ValueError(f"{flag} {K} exceeds the vocabulary size {vocab}")
    return K


def _bits(scores_fp16: np.ndarray) -> np.ndarray:
    scores = np.asarray(scores_fp16)
    if scores.dtype != np.float16 or scores.ndim != 2:
        raise TypeError("scores must be a [rows, V] float16 array")
    return np.ascontiguousarray(scores).view(np.uint16)


def keys(bits: np.ndarray) -> np.ndarray:
    """The uint16 keys of an array of fp16 bit patterns: the pattern itself up to 0x3C00, else 0."""
    bits = np.asarray(bits, dtype=np.uint16)
    return np.where(bits <= ONE_BITS, bits, np.uint16(0))


def topk_rows(scores_fp16: np.ndarray, K: int) -> Tuple[np.ndarray, np.ndarray]:
    """The host implementation: ``(ids int32 [rows, K], vals uint16 [rows, K])`` of ``scores_fp16``
    ([rows, V] float16).  Each entry becomes one int64 ``key << 32 | (2^32 - 1 - index)``, whose
    plain order is the ranking; ``np.partition`` brings a row's K largest to its end (O(V) per
    row), and only those are sorted."""
    bits = _bits(scores_fp16)
    rows, V = bits.shape
    K = check_k(K, V, "K")
    ids = np.empty((rows, K), dtype=np.int32)
    vals = np.empty((rows, K), dtype=np.uint16)
    low = np.int64(0xFFFFFFFF) - np.arange(V, dtype=np.int64)
    step = max(1, _CHUNK_ELEMS // V)
    for r0 in range(0, rows, step):
        comp = (keys(bits[r0:r0 + step]).astype(np.int64) << 32) | low
        if K < V:
            comp = np.partition(comp, V - K, axis=1)[:, V - K:]
        best = np.sort(comp, axis=1)[:, ::-1]
        ids[r0:r0 + step] = (np.int64(0xFFFFFFFF) - (best & np.int64(0xFFFFFFFF))).astype(np.int32)
        vals[r0:r0 + step] = (best >> 32).astype(np.uint16)
    return ids, vals


def picked_keys(scores_fp16: np.ndarray, picked: np.ndarray) -> np.ndarray:
    """uint16 [rows]: the key of entry ``picked[r]`` of row r; 0 for an id outside [0, V)."""
    bits = _bits(scores_fp16)
    rows, V = bits.shape
    picked = np.asarray(picked).reshape(-1).astype(np.int64)
    if picked.shape[0] != rows:
        raise ValueError(f"{rows} rows but {picked.shape[0]} picked ids")
    ok = (picked >= 0) & (picked < V)
    out = np.zeros(rows, dtype=np.uint16)
    out[ok] = keys(bits[np.flatnonzero(ok), picked[ok]])
    return out


def pack(ids: np.ndarray, vals: np.ndarray) -> np.ndarray:
    """``TOPK_DTYPE`` array of the shape of ``ids`` (``vals``: uint16 keys or float16)."""
    vals = np.asarray(vals)
    out = np.empty(np.shape(ids), dtype=TOPK_DTYPE)
    out["id"] = ids
    out["p"] = vals.view(np.float16) if vals.dtype == np.uint16 else vals.astype(np.float16)
    return out
