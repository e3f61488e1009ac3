"""Cases, float64 oracle and float32 emulation for the segment-pooling kernel ``fls_pool_rows``
(``ops.pool_rows``; flexible_llm_sharding_amd/embed.py holds the definition and the summation
order).  Shared by tests/test_embed_cpu.py and tests/test_embed_gpu.py; needs no GPU.

The oracle is float64 on the identical fp16 inputs.  ``emulated_f32`` performs the kernel's
documented float32 operations in its documented order on the host.  The bound of a group of
cases is ``tau = 8 x max |emulated_f32 - ref64|`` over every output of the group (the scheme of
tests/loglik_ref.py ``group_tau``): the factor covers a fused multiply-add rounding once where the
emulation rounds twice, and the hardware's square root and division.  Cases are grouped by the
scale of their outputs — values of order 1 or of order 65504, normalised or not — because float32
spacing follows the magnitude.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np

TAU_FACTOR = 8.0
SEPARATION = 4.0
THREADS = 256           # l2_normalize_kernel: threads per block
WAVE = 64
NORM_EPS = 1e-12
RAGGED = [1, 2, 63, 64, 65, 300]
F16_MAX = 65504.0


# ------------------------------------------------------------------ oracle and emulation
def ref64(x: np.ndarray, segs: Sequence[np.ndarray], D: int, normalize: bool) -> np.ndarray:
    """float64 [n_seg, D]: embed.py's definition on the fp16 rows ``x``; ``segs[i]`` holds the rows
    of segment i in order (an empty one gives zeros)."""
    out = np.zeros((len(segs), D), dtype=np.float64)
    for i, rows in enumerate(segs):
        if len(rows):
            out[i] = x[np.asarray(rows), :D].astype(np.float64).sum(0) / len(rows)
    if normalize:
        out = out / np.maximum(np.sqrt((out * out).sum(1, keepdims=True)), NORM_EPS)
    return out


def _sumsq_f32(e: np.ndarray) -> np.float32:
    """The kernel's sum of squares of one fp32 row: thread t of 256 accumulates columns t, t + 256,
    ... (one multiply-add each, emulated in float64 and rounded), the 64 lanes of a wave combine
    by the xor butterfly (offsets 32 .. 1), the 4 wave sums are added in wave order from 0."""
    D = e.shape[0]
    pad = np.zeros(-(-D // THREADS) * THREADS, dtype=np.float32)
    pad[:D] = e
    ss = np.zeros(THREADS, dtype=np.float32)
    for chunk in pad.reshape(-1, THREADS):
        ss = (chunk.astype(np.float64) * chunk.astype(np.float64) + ss.astype(np.float64)).astype(np.float32)
    lanes = np.arange(THREADS)
    for o in (32, 16, 8, 4, 2, 1):
        ss = (ss + ss[lanes ^ o]).astype(np.float32)          # (x ^ o stays inside its wave for o < 64)
    tot = np.float32(0.0)
    for w in range(THREADS // WAVE):
        tot = np.float32(tot + ss[w * WAVE])
    return tot


def emulated_f32(x: np.ndarray, segs: Sequence[np.ndarray], D: int, normalize: bool) -> np.ndarray:
    """float32 [n_seg, D]: the kernel's operations in its order — a column's rows added one by one
    starting from the first row itself, one division by float32(n); then the norm as ``_sumsq_f32``,
    sqrt, max with 1e-12 and one division per column."""
    out = np.zeros((len(segs), D), dtype=np.float32)
    for i, rows in enumerate(segs):
        if not len(rows):
            continue
        acc = x[rows[0], :D].astype(np.float32)
        for r in rows[1:]:
            acc = (acc + x[r, :D].astype(np.float32)).astype(np.float32)
        out[i] = acc / np.float32(len(rows))
    if normalize:
        for i in range(len(segs)):
            nrm = np.maximum(np.sqrt(_sumsq_f32(out[i]), dtype=np.float32), np.float32(NORM_EPS))
            out[i] = out[i] / nrm
    return out


# ------------------------------------------------------------------ cases
@dataclass
class PoolCase:
    name: str
    x: np.ndarray                 # fp16 [rows, H], contiguous rows in segment order
    lens: List[int]               # rows per segment (0: an empty segment)
    D: int
    normalize: bool
    group: str
    ld: int = 0                   # row stride on the device (0: H)
    offset: int = 0               # fp16 elements the device base is shifted from a 256-byte boundary
    gather: bool = False          # the device holds the rows permuted; row_idx restores the order
    zero: List[int] = field(default_factory=list)      # all-zero segments (dropping a zero row moves nothing)
    _cache: dict = field(default_factory=dict, repr=False)

    @property
    def H(self) -> int:
        return self.x.shape[1]

    @property
    def seg_start(self) -> np.ndarray:
        return np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int32)

    def segs(self) -> List[np.ndarray]:
        ss = self.seg_start
        return [np.arange(ss[i], ss[i + 1]) for i in range(len(self.lens))]

    def ref(self) -> np.ndarray:
        if "ref" not in self._cache:
            self._cache["ref"] = ref64(self.x, self.segs(), self.D, self.normalize)
        return self._cache["ref"]

    def emu_err(self) -> float:
        if "emu" not in self._cache:
            emu = emulated_f32(self.x, self.segs(), self.D, self.normalize)
            self._cache["emu"] = float(np.abs(emu.astype(np.float64) - self.ref()).max())
        return self._cache["emu"]

    def drop_last_effect(self) -> Dict[int, float]:
        """segment -> max |oracle without its last row - oracle| (segments with a row)."""
        base, segs = self.ref(), self.segs()
        out = {}
        for i, rows in enumerate(segs):
            if len(rows):
                alt = ref64(self.x, [rows[:-1]], self.D, self.normalize)[0]
                out[i] = float(np.abs(alt - base[i]).max())
        return out

    def take_next_effect(self) -> Dict[int, float]:
        """segment -> max |oracle with the next segment's first row appended - oracle| (segments
        followed, possibly after empty ones, by a segment with a row)."""
        base, segs = self.ref(), self.segs()
        out = {}
        for i, rows in enumerate(segs[:-1]):
            nxt = next((s for s in segs[i + 1:] if len(s)), None)
            if nxt is not None:
                alt = ref64(self.x, [np.concatenate([rows, nxt[:1]])], self.D, self.normalize)[0]
                out[i] = float(np.abs(alt - base[i]).max())
        return out


def _group(scale: str, normalize: bool) -> str:
    return f"{scale}_{'norm' if normalize else 'raw'}"


def _unit_rows(rows: int, H: int, seed: int) -> np.ndarray:
    """N(0.25, 1) values: a mean that does not vanish, so a normalised mean has a direction."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((rows, H)) + 0.25).astype(np.float16)


def _steer_column0(x: np.ndarray, lens: Sequence[int]) -> None:
    """Column 0, which is all a D = 1 embedding holds (normalised: its sign alone): every segment
    of >= 2 rows starts with +3 and sums to -1, a one-row segment holds -1.  Dropping a segment's
    last row or taking the next segment's first row (+3) into it then flips the sign of its sum.
    (A one-row segment must not follow another segment: the cases put it first.)"""
    r = 0
    for n in lens:
        if n == 1:
            x[r, 0] = -1.0
        elif n >= 2:
            x[r, 0] = 3.0
            x[r + 1:r + n - 1, 0] = 0.125
            x[r + n - 1, 0] = -1.0 - 3.0 - 0.125 * (n - 2)
        r += n


def ragged_case(H: int, normalize: bool, seed: int, **kw) -> PoolCase:
    x = _unit_rows(sum(RAGGED), H, seed)
    tag = "".join(f"_{k}{v}" for k, v in kw.items())
    return PoolCase(f"ragged_H{H}_{'norm' if normalize else 'raw'}{tag}", x, list(RAGGED), H, normalize,
                    _group("unit", normalize), **kw)


def dim_case(H: int, D: int, normalize: bool, seed: int) -> PoolCase:
    lens = [1, 2, 65]
    x = _unit_rows(sum(lens), H, seed)
    _steer_column0(x, lens)
    return PoolCase(f"dim_H{H}_D{D}_{'norm' if normalize else 'raw'}", x, lens, D, normalize, _group("unit", normalize))


def edges_case(normalize: bool, H: int = 520, seed: int = 40) -> PoolCase:
    """An all-zero segment, a real one, an empty one between it and the next real one, a real one.
    The all-zero segment comes first: appending a zero row to a normalised mean moves nothing, so no
    segment may take its first row; dropping one of its own zero rows moves nothing either
    (``zero``), but taking the next segment's first row does."""
    lens = [4, 3, 0, 2, 5]
    x = _unit_rows(sum(lens), H, seed)
    x[:4] = 0.0
    return PoolCase(f"edges_{'norm' if normalize else 'raw'}", x, lens, H, normalize, _group("unit", normalize), zero=[0])


def big_case(normalize: bool, H: int = 520, seed: int = 41) -> PoolCase:
    """Rows whose every element is +65504 or -65504 (the fp16 extremes), segments of 1, 3, 63 and 65
    rows: the sums stay exact in float32 (multiples of 32 below 2^24 x 32), the divisions by 3, 63
    and 65 round."""
    lens = [1, 3, 63, 65]
    rng = np.random.default_rng(seed)
    x = np.where(rng.random((sum(lens), H)) < 0.5, -F16_MAX, F16_MAX).astype(np.float16)
    return PoolCase(f"big_{'norm' if normalize else 'raw'}", x, lens, H, normalize, _group("big", normalize))


_CASES: Optional[List[PoolCase]] = None


def kernel_cases() -> List[PoolCase]:
    """Built once and shared; nobody modifies a case's arrays."""
    global _CASES
    if _CASES is None:
        cs: List[PoolCase] = []
        for nz in (False, True):
            for i, H in enumerate((64, 520, 4096, 8192)):
                cs.append(ragged_case(H, nz, seed=10 + i))
            for H in (520, 4096):
                for D in (1, 7, 8, H - 8):
                    cs.append(dim_case(H, D, nz, seed=20 + D % 13))
            cs.append(ragged_case(520, nz, seed=30, ld=528))                 # ld > H, 16-byte loads
            cs.append(ragged_case(520, nz, seed=31, ld=523))                 # an odd stride: scalar loads
            cs.append(ragged_case(520, nz, seed=32, offset=1))               # a base 2 bytes off
            cs.append(ragged_case(4096, nz, seed=33, offset=4))              # a base 8 bytes off
            cs.append(ragged_case(520, nz, seed=34, gather=True))
            cs.append(ragged_case(4096, nz, seed=35, gather=True, ld=4104))
            cs.append(edges_case(nz))
            cs.append(big_case(nz))
        _CASES = cs
    return _CASES


def group_tau(cases: Sequence[PoolCase]) -> Dict[str, float]:
    """group -> tau = TAU_FACTOR x the largest emulation error over every output of the group."""
    tau: Dict[str, float] = {}
    for c in cases:
        tau[c.group] = max(tau.get(c.group, 0.0), TAU_FACTOR * c.emu_err())
    return tau
