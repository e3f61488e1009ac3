"""Shared helpers of the LoRA tests: an exact-arithmetic oracle of the merge definition
(``fractions.Fraction``, independent of ``lora.fma32``'s float64 trick), kernel test data with the
edge cases planted, and the checkpoint / adapter / twin fixtures of the engine tests."""
import json
import os
from fractions import Fraction

import numpy as np
import torch

LIT_A = np.float32(2.0 ** -11 * (1 + 2.0 ** -14))      # the literal case: w = 1, b' = 1 + 2^-14 -> 0x3C01
LIT_B = np.float32(1 + 2.0 ** -14)

ROWS = (1, 31, 32, 33, 130)
COLS = (8, 24, 32, 40, 264, 1032)
COLS_NARROW = (1, 7, 20)
RANKS = (1, 2, 3, 4, 5, 16, 17, 64, 255, 256)
BASE_OFFSETS = (0, 2, 6)


# ------------------------------------------------------------------ exact arithmetic
def round_fraction(x: Fraction, p: int, emin: int, emax: int):
    """``x`` rounded to nearest-even in a binary format of ``p`` significand bits, minimum normal
    exponent ``emin`` (subnormals kept), overflow past ``emax`` to infinity -> (Fraction | +-inf)."""
    if x == 0:
        return Fraction(0)
    sign = -1 if x < 0 else 1
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    e = max(e, emin)
    q = Fraction(2) ** (e - p + 1)                       # spacing at this exponent
    n = a / q
    f = n.numerator // n.denominator
    rem = n - f
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and f % 2 == 1):
        f += 1
    r = f * q
    if r >= Fraction(2) ** (emax + 1):
        return sign * float("inf")
    return sign * r


def exact_merge_element(w: float, a, b) -> float:
    """One element of the definition in exact rational arithmetic: fp32 fma chain over ``a`` / ``b``
    (fp32 values, already padded), then fp16 rounding.  Returns a Python float (+-inf on overflow);
    the sign of a zero follows IEEE 754: a non-zero exact value that rounds to zero keeps its sign,
    an exact cancellation gives +0, and (-0) + (-0) is the only exact-zero sum that is -0."""
    import math
    acc, negzero = Fraction(float(w)), float(w) == 0 and math.copysign(1.0, float(w)) < 0
    for x, y in zip(a, b):
        if isinstance(acc, float):                       # infinite already (finite operands: stays)
            continue
        x, y = float(x), float(y)
        p = Fraction(x) * Fraction(y)
        s = p + acc
        if s != 0:
            acc = round_fraction(s, 24, -126, 127)
            negzero = not isinstance(acc, float) and acc == 0 and s < 0
        else:
            pneg = (math.copysign(1.0, x) < 0) != (math.copysign(1.0, y) < 0)
            negzero = p == 0 and acc == 0 and pneg and negzero
            acc = Fraction(0)
    if isinstance(acc, float):
        return acc
    r = round_fraction(acc, 11, -14, 15)
    if isinstance(r, float):
        return r
    if r == 0:
        return -0.0 if (acc < 0 or (acc == 0 and negzero)) else 0.0
    return float(r)


def bits16(x) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(x, dtype=np.float16)).view(np.uint16)


# ------------------------------------------------------------------ kernel test data
def full_mantissa(rng: np.random.Generator, shape, emin: int, emax: int) -> np.ndarray:
    """fp32 values with random signs, all 23 mantissa bits random, exponents in [emin, emax]."""
    mant = rng.integers(0, 1 << 23, size=shape, dtype=np.int64)
    exp = rng.integers(emin + 127, emax + 128, size=shape, dtype=np.int64)
    sign = rng.integers(0, 2, size=shape, dtype=np.int64)
    return ((sign << 31) | (exp << 23) | mant).astype(np.uint32).view(np.float32)


def kernel_case(rows: int, cols: int, r: int, seed: int):
    """(w fp16 [rows, cols], A fp32 [R, cols], Bs fp32 [rows, R], facts) with R = r padded to a
    multiple of 4 (+0).  Random full-mantissa operands in which every (o, i, k) matters, random fp16
    weights with -0 and subnormals sprinkled in, and — rows / columns permitting — planted rows:

    * the literal case (``w = 1``, ``b' = 1 + 2^-14`` at k = 0 only, ``a = 2^-11 (1 + 2^-14)`` ->
      ``0x3C01``) in the first, an interior and the last row and column (so in the first, an
      interior and the last tile);
    * row 1: ``b' = 2^24`` at k = 0 only: results overflow to +-inf;
    * row 2, column 1: ``b' = -w``, ``a = 1``: exact cancellation to +0;
    * row 3: subnormal weights and ``b'`` scaled by 2^-24: fp16 subnormal results;
    * fp32 subnormal operands on ``w = +0`` (they are kept, not flushed): row 4 has negative
      subnormal ``b'`` at k = 0 only, so where ``a[0, i] > 0`` the chain ends at a negative fp32
      subnormal, ``-0`` in fp16 (a flushed ``b'`` gives ``+0``); row 5 has ``b' = -1`` at k = 0 only
      and column 2 a positive subnormal ``a[0, 2]``: ``-0`` again (a flushed ``a`` gives ``+0``).

    ``facts`` lists (row, col, expected fp16 bits) of the planted literals and the cancellation."""
    rng = np.random.default_rng(seed)
    R = (r + 3) // 4 * 4
    A = np.zeros((R, cols), np.float32)
    Bs = np.zeros((rows, R), np.float32)
    A[:r] = full_mantissa(rng, (r, cols), -6, 0)
    Bs[:, :r] = full_mantissa(rng, (rows, r), -8, -2)
    wbits = rng.integers(0, 0x7000, size=(rows, cols), dtype=np.int64) | (rng.integers(0, 2, size=(rows, cols)) << 15)
    w = wbits.astype(np.uint16).view(np.float16).copy()
    spr = rng.random((rows, cols))
    w[spr < 0.03] = np.float16(-0.0)
    w[(spr >= 0.03) & (spr < 0.05)] = np.float16(0.0)
    sub = (spr >= 0.05) & (spr < 0.08)
    w[sub] = rng.integers(1, 0x400, size=int(sub.sum())).astype(np.uint16).view(np.float16)
    facts = []
    lit_rows = sorted({0, rows // 2, rows - 1})
    lit_cols = sorted({0, cols // 2, cols - 1})
    special = rows >= 31 and cols >= 7
    if special:
        Bs[1, :] = 0
        Bs[1, 0] = np.float32(2.0 ** 24)
        A[0, 1] = np.float32(1.0)
        Bs[2, 1:] = 0
        Bs[2, 0] = -np.float32(w[2, 1]) if np.isfinite(w[2, 1]) else np.float32(0)
        facts.append((2, 1, 0x0000))
        w[3, :] = rng.integers(1, 0x400, size=cols).astype(np.uint16).view(np.float16)
        Bs[3, :] *= np.float32(2.0 ** -24)
        sub = lambda n: rng.integers(1, 1 << 23, size=n).astype(np.uint32)            # noqa: E731
        w[4:6, :] = np.float16(0.0)
        Bs[4:6, :] = 0
        Bs[4, 0] = (sub(1) | np.uint32(1 << 31)).view(np.float32)[0]
        Bs[5, 0] = np.float32(-1.0)
        A[0, 2] = sub(1).view(np.float32)[0]
        facts.append((5, 2, 0x8000))
    for i in lit_cols:
        A[0, i] = LIT_A
    for o in lit_rows:
        Bs[o, :] = 0
        Bs[o, 0] = LIT_B
        for i in lit_cols:
            w[o, i] = np.float16(1.0)
            facts.append((o, i, 0x3C01))
    if special:                                   # (after the literal columns: their a[0, i] is set)
        facts += [(4, i, 0x8000) for i in range(cols) if A[0, i] > 0 and i != 2]
    return w, A, Bs, facts


def kernel_cases():
    """Every (rows, cols) pair of the kernel test, each with two ranks, so that every rank meets
    several shapes: [(rows, cols, r)]."""
    out, p = [], 0
    for cols in COLS + COLS_NARROW:
        for rows in ROWS:
            out.append((rows, cols, RANKS[p % len(RANKS)]))
            out.append((rows, cols, RANKS[(3 * p + 5) % len(RANKS)]))
            p += 1
    return out


# ------------------------------------------------------------------ adapters on disk
def write_adapter(path, tensors: dict, **conf) -> str:
    """An adapter directory from literal tensors ({module: (A, B)}) and config fields."""
    from flexible_llm_sharding_amd.utils.safetensors_io import save_file
    os.makedirs(path, exist_ok=True)
    sd = {}
    for module, (A, B) in tensors.items():
        if A is not None:
            sd[f"base_model.model.{module}.lora_A.weight"] = A
        if B is not None:
            sd[f"base_model.model.{module}.lora_B.weight"] = B
    c = {"peft_type": "LORA", "lora_alpha": 8, "bias": "none"}
    c.update(conf)
    with open(os.path.join(path, "adapter_config.json"), "w") as f:
        json.dump(c, f)
    save_file(sd, os.path.join(path, "adapter_model.safetensors"))
    return str(path)


# ------------------------------------------------------------------ engine fixtures
R_TEST = 4


def make_base(root, name: str, quantize=None, seed: int = 3, **kw):
    """(cfg, checkpoint dir) of preset ``name``: fp16, ``quantize="bf16"`` (a bf16 checkpoint), or
    quantised (``fp8`` / ``int4``)."""
    from flexible_llm_sharding_amd.config import preset
    from flexible_llm_sharding_amd.utils.synthetic import write_synthetic_checkpoint
    cfg = preset(name)
    d = os.path.join(str(root), f"{name}_{quantize or 'fp16'}")
    if not os.path.isdir(d):
        how = {"dtype": torch.bfloat16} if quantize == "bf16" else {"quantize": quantize} if quantize else {}
        write_synthetic_checkpoint(cfg, d, seed=seed, std=0.05, **how, **kw)
    return cfg, d


def make_adapter(root, cfg, name: str, r: int = R_TEST, seed: int = 1, **kw):
    """(adapter dir, loaded adapter) of a random adapter on every target ``cfg`` has."""
    from flexible_llm_sharding_amd import lora
    d = os.path.join(str(root), f"{name}_adapter_r{r}_{seed}")
    if not os.path.isdir(d):
        lora.write_synthetic_adapter(cfg, d, r=r, seed=seed, **kw)
    return d, lora.LoraAdapter.load(cfg, d)


def make_twin(root, name: str, base: str, adapter, quantize=None) -> str:
    """The merged fp16 twin of ``base`` (a quantised base: of its fp16 twin)."""
    from flexible_llm_sharding_amd import fp8, int4, lora
    src = base
    if quantize in ("fp8", "int4"):
        src = base + "_twin16"
        if not os.path.isdir(src):
            (fp8 if quantize == "fp8" else int4).write_twin(base, src)
    d = base + "_merged"
    if not os.path.isdir(d):
        lora.write_twin(src, adapter, d)
    return d


def prompts_for(cfg, n: int = 3, seed: int = 5):
    from flexible_llm_sharding_amd.utils.synthetic import synthetic_prompts
    return synthetic_prompts(n, 24, 3, 6, cfg.vocab_size, seed=seed, vary=True)


def same_arrays(a, b) -> bool:
    """Two runs' outputs (arrays, or nested lists of arrays) equal in every bit."""
    if isinstance(a, (list, tuple)) or isinstance(b, (list, tuple)):
        return isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)) and len(a) == len(b) \
            and all(same_arrays(x, y) for x, y in zip(a, b))
    x, y = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
