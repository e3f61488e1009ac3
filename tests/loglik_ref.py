"""References and case builders for the continuation log-likelihood tests (no tests here).

Kernel level (``fls_logprob_rows``): one fp16 logits matrix, three readings of it

* :func:`ref64` - ``l[t] - logsumexp(l)`` and the greedy flag in float64;
* :func:`emulated_f32` - the same in float32 with the kernel's summation: 256 lanes, each an
  online max and sum over its 8-column chunks (or single columns on the scalar path), the lanes
  combined by ``block_max`` / ``block_sum`` (xor butterfly per 64-lane wave, then the 4 waves in
  order), ``(l_t - m) - logf(s)`` at the end;
* the kernel itself (tests/test_loglik_gpu.py).

The bound of a group of cases is ``tau = 8 * max |emulated_f32 - ref64|`` over every row of the
group, from the CPU alone (the method of tests/attention_rows.py): the factor covers the hardware
exp, fused multiply-adds and logf.  Cases are grouped by the scale of their logits, because the
error of the result is set by the float32 spacing at ``|lp|``: the cases with logits of order 1-10
share one tau, the rows near +-60000 (``|lp|`` ~ 1.2e5, spacing 2^-7) have their own.  A case is
usable when dropping any row's spike column from its logsumexp moves ``lp`` by at least 4 tau
(:func:`spike_effect`).

Engine level: prompts whose oracle target probabilities are bounded below (:func:`likely_prompts`),
so a probability tolerance carries to logs as ``atol_p / p_min``, and the target-shift
discrimination (:func:`shifted_sums`).
"""
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

TAU_FACTOR = 8.0
SEPARATION = 4.0
LANES = 256


# ------------------------------------------------------------------ kernel references
def scaled(logits: np.ndarray, inv_scale: float) -> np.ndarray:
    """The float32 values the kernel normalises: the fp16 logits, or fp16(logit * inv_scale)."""
    l = logits.astype(np.float32)
    if np.float32(inv_scale) != np.float32(1.0):
        l = (l * np.float32(inv_scale)).astype(np.float16).astype(np.float32)
    return l


def ref64(logits: np.ndarray, targets: np.ndarray, inv_scale: float = 1.0, drop: Optional[np.ndarray] = None):
    """-> (lp [rows] float64, greedy flag [rows]).  ``drop`` [rows]: a column left out of each
    row's logsumexp (the defect :func:`spike_effect` measures)."""
    l = scaled(logits, inv_scale).astype(np.float64)
    rows = np.arange(l.shape[0])
    lt = l[rows, targets]
    m = l.max(axis=1)
    e = np.exp(l - m[:, None])
    if drop is not None:
        e[rows, drop] = 0.0
    return lt - m - np.log(e.sum(axis=1)), (lt == m).astype(np.float64)


def emulated_f32(logits: np.ndarray, targets: np.ndarray, inv_scale: float = 1.0, vec: Optional[bool] = None):
    """float32 emulation of logprob_rows_kernel's arithmetic -> lp [rows] float32."""
    l = scaled(logits, inv_scale)
    R, V = l.shape
    if vec is None:
        vec = V % 8 == 0
    w = 8 if vec else 1                       # columns a lane takes per step
    per = LANES * w
    steps = -(-V // per)
    pad = np.full((R, steps * per), -np.inf, dtype=np.float32)
    pad[:, :V] = l
    x = pad.reshape(R, steps, LANES, w)       # step k, lane i: columns (k * 256 + i) * w ...
    valid = (np.arange(steps * per).reshape(steps, LANES, w)[:, :, 0] < V)
    m = np.full((R, LANES), -np.inf, dtype=np.float32)
    s = np.zeros((R, LANES), dtype=np.float32)
    with np.errstate(invalid="ignore"):
        for k in range(steps):
            v = x[:, k]
            nm = np.maximum(m, v.max(axis=2))
            s2 = s * np.exp(m - nm)
            s2 = np.where(np.isnan(s2), np.float32(0), s2).astype(np.float32)     # (m = nm = -inf: unused)
            for j in range(w):
                s2 = (s2 + np.exp(v[:, :, j] - nm)).astype(np.float32)
            ok = valid[k][None, :]
            s = np.where(ok, s2, s).astype(np.float32)
            m = np.where(ok, nm, m).astype(np.float32)
        gm = m.max(axis=1)
        c = np.where(np.isneginf(m), np.float32(0), s * np.exp(m - gm[:, None])).astype(np.float32)
    c = c.reshape(R, LANES // 64, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):            # warp_sum: v += shfl_xor(v, o)
        c = (c + c[:, :, lane ^ o]).astype(np.float32)
    gs = np.zeros(R, dtype=np.float32)
    for wv in range(LANES // 64):             # block_sum: the waves' totals in order
        gs = (gs + c[:, wv, 0]).astype(np.float32)
    lt = l[np.arange(R), targets]
    return ((lt - gm).astype(np.float32) - np.log(gs).astype(np.float32)).astype(np.float32)


def edge_columns(V: int) -> List[int]:
    """0, 7, 8, 2047, 2048, V - V % 8 - 1, V - V % 8, V - 1, clipped to [0, V)."""
    cols = [0, 7, 8, 2047, 2048, V - V % 8 - 1, V - V % 8, V - 1]
    return sorted({c for c in cols if 0 <= c < V})


def edge_kinds(V: int, col: int) -> List[int]:
    """Which of the eight edge formulas give ``col`` for this V."""
    cols = [0, 7, 8, 2047, 2048, V - V % 8 - 1, V - V % 8, V - 1]
    return [k for k, c in enumerate(cols) if c == col]


@dataclass
class KernelCase:
    name: str
    logits: np.ndarray            # [rows, V] fp16
    targets: np.ndarray           # [rows] int32
    spikes: np.ndarray            # [rows] the spike column of each row
    inv_scale: float = 1.0
    ld: int = 0                   # row stride the GPU test gives the matrix (0: V)
    group: str = "unit"           # cases sharing a tau

    @property
    def V(self) -> int:
        return self.logits.shape[1]

    @property
    def vec(self) -> bool:
        return self.V % 8 == 0 and (self.ld or self.V) % 8 == 0

    def ref(self):
        return ref64(self.logits, self.targets, self.inv_scale)

    def emu(self) -> np.ndarray:
        return emulated_f32(self.logits, self.targets, self.inv_scale, vec=self.vec)

    def emu_err(self) -> float:
        return float(np.abs(self.emu().astype(np.float64) - self.ref()[0]).max())

    def spike_effect(self) -> np.ndarray:
        """|lp with the spike column left out of the logsumexp - lp| per row."""
        return np.abs(ref64(self.logits, self.targets, self.inv_scale, drop=self.spikes)[0] - self.ref()[0])


def spiked_case(name: str, rows: int, V: int, seed: int, offset: int = 0, inv_scale: float = 1.0, ld: int = 0,
                spike: float = 8.0) -> KernelCase:
    """N(0, 1) logits; row r has ``spike`` on edge column (r + offset) mod n and its target on a
    different edge column, the pairing rotating so that with rows >= n every edge column is the
    spike of some row and the target of some row.  inv_scale != 1: the logits are divided by it
    first, so the kernel's scaled values have that shape."""
    rng = np.random.default_rng(seed)
    edges = edge_columns(V)
    n = len(edges)
    x = rng.standard_normal((rows, V)).astype(np.float32)
    r = np.arange(rows)
    si = (r + offset) % n
    ti = (si + 1 + (r // n) % (n - 1)) % n
    sp = np.asarray(edges)[si]
    x[r, sp] = spike
    x = x / np.float32(inv_scale)
    return KernelCase(name, x.astype(np.float16), np.asarray(edges)[ti].astype(np.int32), sp, inv_scale, ld)


def flat_case(V: int = 1000, value: float = 0.5) -> KernelCase:
    """One flat row: lp = -ln V, and the target ties with the maximum.  Its 'spike' (height 0) is
    edge column 0: leaving any column out moves lp by ln(V / (V - 1))."""
    x = np.full((1, V), value, dtype=np.float16)
    return KernelCase(f"flat_{V}", x, np.asarray([V - 1], dtype=np.int32), np.asarray([0]))


def tie_case(V: int = 2056, seed: int = 5) -> KernelCase:
    """Greedy flag under ties: rows whose target shares the maximum with the spike column (flag 1),
    sits one fp16 step below it (flag 0), or is the spike itself (flag 1)."""
    c = spiked_case("tie", 6, V, seed)
    top = np.float16(8.0)
    below = np.nextafter(top, np.float16(0))
    for r in range(6):
        t = c.targets[r]
        if r % 3 == 0:
            c.logits[r, t] = top
        elif r % 3 == 1:
            c.logits[r, t] = below
        else:
            c.targets[r] = c.spikes[r]
    c.name = f"tie_{V}"
    return c


def large_case(V: int = 4096, rows: int = 8, seed: int = 6) -> KernelCase:
    """Logits near +-60000 (fp16's largest is 65504, its spacing there 32, so no +8 spike exists):
    all columns near -60000 but the spike column and 1-3 more at +60000, the target a low column.
    lp = -(120000 + 32 j) - ln(k + 1): exp(m - nm) and the sum see differences of 1.2e5 without
    overflow, and leaving the spike out moves lp by ln((k + 1) / k) >= ln(4 / 3)."""
    rng = np.random.default_rng(seed)
    x = (-60000 + 32 * rng.integers(-3, 4, (rows, V))).astype(np.float32)
    edges = edge_columns(V)
    n = len(edges)
    r = np.arange(rows)
    sp = np.asarray(edges)[r % n]
    tg = np.asarray(edges)[(r + 1) % n]
    for i in range(rows):
        x[i, [100, 1000, 3000][:1 + i % 3]] = 60000
    x[r, sp] = 60000
    return KernelCase(f"large_{V}", x.astype(np.float16), tg.astype(np.int32), sp, group="large")


def kernel_cases() -> List[KernelCase]:
    """The shapes of the kernel test: (rows, V) = (1, 8), (3, 1000), (300, 2056), (5, 32000),
    (4, 32003) and (9, 2051) on the scalar path, (2, 151936); strided views on both paths, a scaled
    case, the flat row, ties, the rows near +-60000.  The offsets make the few rows of the small
    cases land on edge columns the other cases leave out."""
    return [
        spiked_case("1x8", 1, 8, 1),
        spiked_case("3x1000", 3, 1000, 2, offset=1),
        spiked_case("300x2056", 300, 2056, 3),
        spiked_case("5x32000", 5, 32000, 4, offset=2),
        spiked_case("4x32003", 4, 32003, 5, offset=5),
        spiked_case("9x2051", 9, 2051, 6),
        spiked_case("2x151936", 2, 151936, 7, offset=4),
        spiked_case("ld2064", 7, 2056, 8, ld=2064),
        spiked_case("ld2057", 7, 2056, 9, ld=2057),
        spiked_case("scaled", 7, 2056, 10, inv_scale=1.0 / 3.0),
        flat_case(),
        tie_case(),
        large_case(),
    ]


def group_tau(cases: List[KernelCase]) -> dict:
    """group -> tau = TAU_FACTOR x the largest emulation error over every row of the group."""
    tau = {}
    for c in cases:
        tau[c.group] = max(tau.get(c.group, 0.0), TAU_FACTOR * c.emu_err())
    return tau


# ------------------------------------------------------------------ engine cases
def likely_prompts(cfg, sd, tok, mode: str, shapes, seed: int = 0, p_floor: float = 0.02):
    """Prompts [(prefix words, suffix words ...)] for ``shapes`` = [(Lp, [L, ...]), ...] whose every
    suffix token is one the oracle itself finds likely given what precedes it: token t is drawn in
    turn from ranks 0, 1, 2, 3 of the oracle's next-token distribution (rank 0 when the ranked one
    falls below ``p_floor``), ids 0-2 (unk / bos / eos) left out.  The target probabilities then
    spread over more than a decade while staying above a floor, whatever the engine computes."""
    from flexible_llm_sharding_amd.models.reference import reference_logliks
    from flexible_llm_sharding_amd.utils.tokenizer import synthetic_word
    rng = np.random.default_rng(seed)

    def words(ids):
        return " ".join(synthetic_word(int(i)) for i in ids)

    prompts, k = [], 0
    for Lp, lens in shapes:
        prefix = words(rng.integers(3, cfg.vocab_size, Lp - 1))          # + BOS = Lp tokens
        sufs = []
        for L in lens:
            u: List[int] = []
            for _ in range(L):
                d = reference_logliks(cfg, sd, tok, [(prefix, (words(u + [3]),))], mode, dists=True)[0][0][-1]
                d = d.copy()
                d[:3] = -np.inf
                order = np.argsort(-d)
                pick = order[k % 4]
                u.append(int(pick if d[pick] >= np.log(p_floor) else order[0]))
                k += 1
            sufs.append(words(u))
        prompts.append((prefix, tuple(sufs)))
    return prompts


def shifted_sums(dists, targets) -> List[np.ndarray]:
    """Per prompt the suffix sums when every target is taken one position late: the prompt's
    targets, in suffix -> token order, rolled by one (a suffix of one token gets its neighbour's),
    read from the oracle's own [L, V] rows ``dists``."""
    out = []
    for dp, tp in zip(dists, targets):
        flat = np.roll(np.concatenate([np.asarray(u) for u in tp]), -1)
        sums, r = [], 0
        for d, u in zip(dp, tp):
            n = len(u)
            sums.append(float(d[np.arange(n), flat[r:r + n]].sum()))
            r += n
        out.append(np.asarray(sums))
    return out
