"""Sampled generation: temperature, top-k and top-p, integer-exact.

The sampler works on the fp16 probabilities the engine returns (``scores[s, t, :]``), which no
sampling flag changes.  Device kernel (``csrc/kernels/sampling.hip``), this host sampler and the
test oracle return the same token for every input, so a run can be replayed from its output file
and the seed.

1. Weights.  A probability is an fp16 bit pattern ``b`` in ``0x0000..0x3C00`` (0 to 1.0); its
   weight is ``W[b] = floor(2^30 * p_b^(1/T) + 0.5)`` (:func:`weight_table`), exactly ``p_b * 2^30``
   at ``T = 1``; any other bit pattern (negative, NaN, > 1) weighs 0.  Temperature is therefore
   ``p^(1/T)`` renormalised: ``softmax(logits / T)`` over the tokens whose fp16 probability is
   non-zero.
2. Order.  Tokens are ranked by ``(b descending, index ascending)`` — by the bits, not the weight
   (distinct bit patterns can share a weight at ``T != 1``); tokens of weight 0 are dropped.
3. Truncation, in HF's order.  ``top_k > 0`` keeps the first ``top_k`` ranked tokens, of weight sum
   ``S_k``; with ``P = clip(round(top_p * 65536), 1, 65536)`` and ``tau = max(1, ceil(S_k * P /
   65536))``, top-p keeps the shortest ranked prefix whose weight sum is ``>= tau``; ``S`` is the
   kept sum.
4. Draw.  ``draw(seed, p, s, t) = splitmix64(splitmix64(splitmix64(seed) ^ p) ^ ((s << 32) | t))``
   with ``p`` the prompt's index in the prompt file, ``s`` the suffix index and ``t`` the generation
   step: a token is a function of ``(scores row, seed, p, s, t)`` and nothing else.
5. Choice.  ``u = (draw * S) >> 64``; the token is the first ranked one whose inclusive cumulative
   weight exceeds ``u``.  ``S = 0`` (an all-zero row, or at ``T < 1`` one whose few subnormals all
   round to weight 0) gives token 0.  ``top_k = 1`` is the greedy token, first index on ties, for
   every row with a non-zero weight; so is ``P = 1`` whenever the largest weight is at least
   ``2^-16`` of ``S_k`` (``tau = ceil(S_k / 65536)`` is then within the first token).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

ONE_BITS = 0x3C00                  # fp16 1.0
TABLE_SIZE = ONE_BITS + 1
MAX_VOCAB = 1 << 18                # S_k * P < 2^64 needs V < 2^18
_M64 = (1 << 64) - 1


def weight_table(temperature: float) -> np.ndarray:
    """[0x3C01] uint32: the weight of every fp16 bit pattern 0 .. 0x3C00 at ``temperature``."""
    T = float(temperature)
    if not (T > 0.0 and np.isfinite(T)):
        raise ValueError(f"temperature must be a finite number > 0, got {temperature!r}")
    p = np.arange(TABLE_SIZE, dtype=np.uint16).view(np.float16).astype(np.float64)
    w = np.zeros(TABLE_SIZE, dtype=np.float64)
    w[1:] = np.floor(np.exp2(np.log2(p[1:]) / T + 30.0) + 0.5)
    table = w.astype(np.uint32)
    assert table[0] == 0 and int(table.max()) <= 1 << 30
    assert (np.diff(table.astype(np.int64)) >= 0).all(), "weight table is not non-decreasing"
    return table


def top_p_units(top_p: float) -> int:
    """``P = clip(round(top_p * 65536), 1, 65536)``."""
    return int(min(65536, max(1, int(np.floor(float(top_p) * 65536.0 + 0.5)))))


def splitmix64(z: int) -> int:
    """The generator step of ``csrc/kernels/elementwise.hip``."""
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def draws(seed: int, prompt_ids: Sequence[int], n_suffix: Sequence[int], step: int) -> np.ndarray:
    """uint64 draws of one generation step, one per (prompt, suffix) in prompt -> suffix order.
    ``prompt_ids``: each prompt's index in the prompt file; ``n_suffix``: its suffix count."""
    h = splitmix64(int(seed) & _M64)
    out = np.empty(int(sum(n_suffix)), dtype=np.uint64)
    r = 0
    for p, ns in zip(prompt_ids, n_suffix):
        hp = splitmix64(h ^ (int(p) & _M64))
        for s in range(ns):
            out[r] = splitmix64(hp ^ (((s << 32) | int(step)) & _M64))
            r += 1
    return out


def sample_tokens(scores_fp16: np.ndarray, table: np.ndarray, top_k: int, P: int, draws: np.ndarray) -> np.ndarray:
    """The host sampler: [rows] int64 tokens of ``scores_fp16`` ([rows, V] float16), one draw each.
    Each row is reduced to its tokens of non-zero weight (a small part of a real row) before the
    stable sort by bit pattern."""
    scores = np.asarray(scores_fp16)
    if scores.dtype != np.float16 or scores.ndim != 2:
        raise TypeError("scores must be a [rows, V] float16 array")
    rows, V = scores.shape
    if V >= MAX_VOCAB:
        raise ValueError(f"sampling supports vocabularies below {MAX_VOCAB}, got {V}")
    if len(draws) != rows:
        raise ValueError(f"{rows} rows but {len(draws)} draws")
    if len(table) != TABLE_SIZE or top_k < 0 or not 1 <= P <= 65536:
        raise ValueError("table of 0x3C01 weights, top_k >= 0 and P in [1, 65536] expected")
    ext = np.zeros(TABLE_SIZE + 1, dtype=np.uint64)      # one more bin: every out-of-range pattern
    ext[:TABLE_SIZE] = table
    bits = np.ascontiguousarray(scores).view(np.uint16)
    weights = ext[np.minimum(bits, TABLE_SIZE)]
    out = np.zeros(rows, dtype=np.int64)
    for r in range(rows):
        idx = np.flatnonzero(weights[r])
        if idx.size == 0:
            continue
        idx = idx[np.argsort(-bits[r, idx].astype(np.int32), kind="stable")]
        if top_k > 0:
            idx = idx[:top_k]
        cum = np.cumsum(weights[r, idx], dtype=np.uint64)
        s_k = int(cum[-1])
        tau = max(1, (s_k * P + 65535) >> 16)
        keep = int(np.searchsorted(cum, np.uint64(tau), side="left")) + 1
        u = (int(draws[r]) * int(cum[keep - 1])) >> 64
        out[r] = idx[int(np.searchsorted(cum[:keep], np.uint64(u), side="right"))]
    return out


@dataclass(frozen=True)
class SamplingParams:
    temperature: float = 1.0
    top_k: int = 0
    top_p: float = 1.0
    seed: int = 0

    def __post_init__(self):
        check_sampling_values(self.temperature, self.top_k, self.top_p)

    @property
    def P(self) -> int:
        return top_p_units(self.top_p)

    def table(self) -> np.ndarray:
        return weight_table(self.temperature)

    def as_dict(self) -> dict:
        return {"do_sample": True, "temperature": float(self.temperature), "top_k": int(self.top_k),
                "top_p": float(self.top_p), "seed": int(self.seed)}

    @staticmethod
    def from_args(args) -> Optional["SamplingParams"]:
        """The run's sampling parameters, or None for greedy generation (no ``--do_sample``)."""
        if not getattr(args, "do_sample", False):
            return None
        return SamplingParams(float(getattr(args, "temperature", 1.0)), int(getattr(args, "top_k", 0)),
                              float(getattr(args, "top_p", 1.0)), int(getattr(args, "seed", 0)))


def check_sampling_values(temperature, top_k, top_p) -> None:
    """Out-of-range values are refused, naming the flag."""
    if not (np.isfinite(temperature) and temperature > 0.0):
        raise ValueError(f"--temperature must be > 0, got {temperature}")
    if int(top_k) != top_k or top_k < 0:
        raise ValueError(f"--top_k must be an integer >= 0, got {top_k}")
    if not (0.0 < top_p <= 1.0):
        raise ValueError(f"--top_p must be in (0, 1], got {top_p}")
