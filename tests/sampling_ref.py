"""Oracle and cases for sampled generation (temperature, top-k, top-p).

The oracle is written from the definition alone (``flexible_llm_sharding_amd/sampling.py``'s
docstring) and shares no code with the package: per row a ``np.lexsort`` on ``(index, -bits)``,
a ``cumsum`` and ``searchsorted``, with Python ints for the 128-bit product.  ``mutant`` switches on
one deliberate mistake, for the test that the cases discriminate:

* ``"tie_order"``  equal bit patterns ranked by index descending
* ``"tau_gt"``     top-p keeps the shortest prefix whose sum is ``> tau`` instead of ``>= tau``
* ``"by_weight"``  ranked by (weight descending, index ascending) instead of by the bits
"""
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

ONE = 0x3C00
M64 = (1 << 64) - 1


def ref_weights(bits: np.ndarray, T: float) -> np.ndarray:
    """uint64 weights of an array of fp16 bit patterns: floor(2^30 p^(1/T) + 0.5), 0 outside (0, 1]."""
    bits = np.asarray(bits, dtype=np.uint16)
    ok = (bits >= 1) & (bits <= ONE)
    p = bits.view(np.float16).astype(np.float64)
    w = np.zeros(bits.shape, dtype=np.float64)
    w[ok] = np.floor(np.exp2(np.log2(p[ok]) / T + 30.0) + 0.5)
    return w.astype(np.uint64)


def ref_P(top_p: float) -> int:
    return min(65536, max(1, int(round(top_p * 65536))))


def _mix(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def ref_draw(seed: int, p: int, s: int, t: int) -> int:
    return _mix(_mix(_mix(seed & M64) ^ p) ^ ((s << 32) | t))


def ref_token(row: np.ndarray, T: float, top_k: int, P: int, draw: int, mutant: Optional[str] = None) -> int:
    """The token of one fp16 row."""
    bits = np.ascontiguousarray(row, dtype=np.float16).view(np.uint16).astype(np.int64)
    w = ref_weights(bits.astype(np.uint16), T)
    idx = np.arange(len(bits))
    key = np.where((bits >= 1) & (bits <= ONE), bits, 0)
    if mutant == "by_weight":
        order = np.lexsort((idx, -w.astype(np.int64)))
    elif mutant == "tie_order":
        order = np.lexsort((-idx, -key))
    else:
        order = np.lexsort((idx, -key))
    order = order[w[order] > 0]
    if top_k > 0:
        order = order[:top_k]
    if len(order) == 0:
        return 0
    cum = np.cumsum(w[order], dtype=np.uint64)
    s_k = int(cum[-1])
    tau = max(1, -(-s_k * P // 65536))
    n = int(np.searchsorted(cum, np.uint64(tau), side="right" if mutant == "tau_gt" else "left")) + 1
    n = min(n, len(order))
    u = (int(draw) * int(cum[n - 1])) >> 64
    return int(order[int(np.searchsorted(cum[:n], np.uint64(u), side="right"))])


def ref_tokens(scores: np.ndarray, T: float, top_k: int, P: int, draws, mutant: Optional[str] = None) -> np.ndarray:
    return np.asarray([ref_token(scores[r], T, top_k, P, int(draws[r]), mutant) for r in range(len(scores))],
                      dtype=np.int64)


# ------------------------------------------------------------------ cases
@dataclass
class Case:
    name: str
    family: str
    scores: np.ndarray            # [rows, V] float16
    T: float
    top_k: int
    P: int
    draws: np.ndarray             # [rows] uint64
    ld: int = 0                   # row stride on the device (0: V)
    offset: int = 0               # elements the device base is moved by (1: no 16-byte alignment)
    _want: dict = field(default_factory=dict)

    @property
    def V(self) -> int:
        return self.scores.shape[1]

    def want(self, mutant: Optional[str] = None) -> np.ndarray:
        if mutant not in self._want:
            self._want[mutant] = ref_tokens(self.scores, self.T, self.top_k, self.P, self.draws, mutant)
        return self._want[mutant]


SETTINGS = [(1.0, 0, 65536), (0.7, 50, ref_P(0.95)), (1.5, 0, ref_P(0.9)), (1.0, 5, 65536), (0.7, 0, 32768),
            (1.5, 3, ref_P(0.5))]
TIE_COLS = (0, 7, 8, 2040, -1)


def _softmax_rows(rng, rows, V, scale):
    x = rng.standard_normal((rows, V)) * scale
    e = np.exp(x - x.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True)).astype(np.float16)


def _draws(rng, rows):
    d = rng.integers(0, 1 << 64, size=rows, dtype=np.uint64, endpoint=False)
    d[0] = 0
    d[-1] = M64
    return d


def _u64(values) -> np.ndarray:
    return np.asarray([int(v) & M64 for v in values], dtype=np.uint64)


def flat_draw(j: int, n: int) -> int:
    """ceil(j 2^64 / n): the smallest draw that lands on the j-th of n equal weights."""
    return -(-(j << 64) // n)


def edge_columns(V: int) -> List[int]:
    """Columns next to every boundary the kernel has: lanes (8 columns), sweeps of a wave
    (512 / 64 columns), the waves' quarters of the row in both load widths, the row's ends."""
    e = {0, 1, V - 2, V - 1}
    for q in (8, 64, 256, 512, 2048):
        e.update((q - 1, q, q + 1))
    for units, width in ((V // 8, 8), (V, 1)):
        per = -(-units // 4)
        for w in (1, 2, 3):
            c = w * per * width
            e.update((c - 1, c, c + 1, c + 63 * width, c + 64 * width))
    return sorted(c for c in e if 0 <= c < V)


def equal_weight_bits(T: float):
    """Two adjacent fp16 bit patterns (the largest such pair) with the same non-zero weight at T."""
    w = ref_weights(np.arange(ONE + 1, dtype=np.uint16), T)
    same = np.flatnonzero((w[1:] == w[:-1]) & (w[1:] > 0))
    assert same.size, T
    b = int(same[-1])
    return b, b + 1


_CASES: List[Case] = []


def kernel_cases() -> List[Case]:
    """Built once and shared (the expected tokens are cached on each case); never modified."""
    if _CASES:
        return _CASES
    rng = np.random.default_rng(20240611)
    out: List[Case] = []
    # random rows: every vocabulary size x every setting; peaked and nearly flat rows, draws 0 and 2^64 - 1
    for V, rows in ((97, 12), (2056, 12), (32000, 6), (151936, 4)):
        sc = np.concatenate([_softmax_rows(rng, rows // 2, V, 4.0), _softmax_rows(rng, rows - rows // 2, V, 1.0)])
        for T, k, P in SETTINGS:
            out.append(Case(f"random_V{V}_T{T}_k{k}_P{P}", "random", sc, T, k, P, _draws(rng, rows)))
    sc = _softmax_rows(rng, 8, 2056, 3.0)
    out.append(Case("stride_vec", "layout", sc, 1.0, 0, 65536, _draws(rng, 8), ld=2056 + 24))
    out.append(Case("stride_scalar", "layout", sc, 0.7, 40, ref_P(0.9), _draws(rng, 8), ld=2056 + 3))
    out.append(Case("stride_V97", "layout", _softmax_rows(rng, 8, 97, 2.0), 1.0, 0, 65536, _draws(rng, 8), ld=128))
    out.append(Case("offset_one", "layout", sc, 1.0, 0, ref_P(0.95), _draws(rng, 8), offset=1))
    out.append(Case("rows300", "layout", _softmax_rows(rng, 300, 2056, 3.0), 0.7, 50, ref_P(0.95), _draws(rng, 300)))
    # ties at the maximum: subsets of TIE_COLS share the largest value, top_k 1..3, a draw per kept token
    V = 2056
    cols = [c % V for c in TIE_COLS]
    for k in (1, 2, 3):
        rows_, dr = [], []
        for sub in (cols, cols[2:], cols[3:], cols[1:3], [cols[4], cols[0]]):
            for j in list(range(k)) + [None]:
                r = (_softmax_rows(rng, 1, V, 1.0)[0].astype(np.float64) * 0.25).astype(np.float16)
                r[sub] = np.float16(0.125)
                rows_.append(r)
                dr.append(M64 if j is None else flat_draw(j, k))
        out.append(Case(f"ties_k{k}", "ties", np.stack(rows_), 1.0, k, 65536, _u64(dr)))
    # flat rows: draw j 2^64 / V lands on column j -- the ordered count across lanes, sweeps and waves
    for V, T, kw in ((97, 1.0, {}), (2056, 1.0, {}), (2056, 1.5, {"offset": 1}), (32000, 1.0, {}), (151936, 0.7, {})):
        js = list(range(V)) if V <= 2056 and not kw else edge_columns(V)
        sc = np.full((len(js), V), np.float16(1.0 / V), dtype=np.float16)
        out.append(Case(f"flat_V{V}_T{T}" + ("_offset" if kw else ""), "flat", sc, T, 0, 65536,
                        _u64(flat_draw(j, V) for j in js), **kw))
    # subnormals, zeros, a single non-zero entry, an all-zero row
    V = 2056
    sc = np.zeros((10, V), dtype=np.uint16)
    sc[0, :] = rng.integers(0, 0x400, V)                  # zeros and subnormals only
    sc[1, rng.integers(0, V, 40)] = rng.integers(1, 0x400, 40)
    for r, c in zip(range(2, 7), (0, 7, 1029, 2048, V - 1)):
        sc[r, c] = 0x0001 if r % 2 else 0x3C00            # one entry: the smallest subnormal, or 1.0
    sc[8, :] = 0x0001                                     # (rows 7 and 9 stay all-zero)
    out.append(Case("sparse", "sparse", sc.view(np.float16), 1.0, 0, 65536, _draws(rng, 10)))
    out.append(Case("sparse_T0.7_p", "sparse", sc.view(np.float16), 0.7, 3, ref_P(0.5), _draws(rng, 10)))
    # bit patterns outside [0, 1]: -0, NaN, 1.5, -inf, -1 -- never chosen, wherever they stand
    sc = _softmax_rows(rng, 8, V, 2.0).view(np.uint16).copy()
    bad = (0x8000, 0x7E00, 0x3E00, 0xFC00, 0xBC00)
    for r in range(8):
        at = rng.choice(V, 64, replace=False)
        sc[r, at] = [bad[i % 5] for i in range(64)]
        sc[r, 0] = bad[r % 5]
        sc[r, V - 1] = bad[(r + 1) % 5]
    sc[6, :] = 0x7E00
    sc[6, 100] = 0x2000
    sc[7, :] = [bad[i % 5] for i in range(V)]             # nothing valid: token 0
    out.append(Case("invalid", "invalid", sc.view(np.float16), 1.0, 0, 65536, _draws(rng, 8)))
    out.append(Case("invalid_k2", "invalid", sc.view(np.float16), 1.5, 2, ref_P(0.9), _draws(rng, 8)))
    # tau on a cumulative boundary.  T = 1, weights 1/2, 1/4, 1/8, 1/8 of S_k = 2^30 (normal values)
    # or of S_k = 2^16 (subnormals, where tau = P): P = 49152 puts tau on the boundary after two
    # tokens, 49151 below it (2^14 or one weight unit), 49153 above; the largest draw takes the last kept token
    for tag, bits4 in (("normal", (0x3800, 0x3400, 0x3000, 0x3000)), ("unit", (0x0200, 0x0100, 0x0080, 0x0080))):
        sc = np.zeros((4, V), dtype=np.uint16)
        for r in range(4):
            sc[r, [1500 + r, 9, 2047, 8]] = bits4
        for P in (49151, 49152, 49153):
            out.append(Case(f"tau_{tag}_P{P}", "tau", sc.view(np.float16), 1.0, 0, P,
                            _u64([M64, M64 - 1, 0, flat_draw(1, 2)])))
    # T = 0.7: two distinct bit patterns of equal weight; the larger bits stand at the larger index
    lo, hi = equal_weight_bits(0.7)
    sc = np.zeros((6, V), dtype=np.uint16)
    for r, (a, b) in enumerate(((0, 7), (7, 8), (8, 2040), (100, V - 1), (511, 512), (3, 1030))):
        sc[r, a], sc[r, b] = lo, hi
        if r >= 3:
            sc[r, 1200:1300] = max(1, lo - 3)             # a tail below both
    for k, P in ((1, 65536), (0, 65536), (0, 1), (2, ref_P(0.5))):
        out.append(Case(f"equal_weight_k{k}_P{P}", "equal_weight", sc.view(np.float16), 0.7, k, P,
                        _u64([0, M64, flat_draw(1, 2) - 1, flat_draw(1, 2), 0, M64])))
    _CASES.extend(out)
    return _CASES
