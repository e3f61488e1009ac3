"""MXFP4 (OCP microscaling v1.0: e2m1 elements, e8m0 block scales) checkpoints: the host definition.

A 2-D projection weight ``X.weight`` of model shape ``[out, in]`` is stored as

    X.weight         U8  [out, in / 2]    byte j of a row holds element 2j in its LOW nibble and
                                          element 2j + 1 in its high nibble
    X.weight_scale   U8  [out, in / 32]   one e8m0 exponent byte ``e`` per block of 32 consecutive
                                          elements of a row

``in % 32 == 0``, so blocks never straddle rows.  For the nibble ``u`` of an element and the byte
``e`` of its block

    code = (0, 0.5, 1, 1.5, 2, 3, 4, 6)[u & 7], negated when u & 8          (e2m1; u = 8 is -0)
    w16  = fp16_rne( code * 2^(e - 127) )                                    e in 0 .. 254
    w16  = 0x7E00 (NaN) for every element of the block                        e = 255

the product formed exactly and rounded ONCE to fp16, round to nearest even: magnitudes above 65504
become +-inf, subnormal results round as usual, tiny products become +-0 with the sign kept.  It is
computed here in fp64, which holds every product exactly, and rounded by numpy's fp64 -> fp16
conversion.  This is the layout AMD Quark's MXFP4 export is understood to write.
``X.weight_scale_inv``, ``X.weight_zero_point`` and ``X.input_scale`` next to a U8 weight are refused.

The *fp16 twin* of an MXFP4 checkpoint is the same directory with ``X.weight`` written as ``w16`` and
the scale tensors removed (:func:`write_twin`): a run on the MXFP4 checkpoint gives, bit for bit, the
outputs of the same run on its twin.

Landing layout (:func:`region_layout`): as INT4's, segment by segment stacked down from the top of
the tensor's own ``2N``-byte region (:mod:`.quant` has the layout and the argument) with groups of 32
and one-byte scales, one segment per launch of ``fls_dequant_mxfp4`` (``csrc/kernels/dequant.hip``).
Every segment boundary is a block boundary, and there are no tables.
"""
from __future__ import annotations

import functools
from typing import Dict, Sequence, Tuple

import numpy as np
import torch

from . import quant
from .fp8 import is_quantized_name
from .quant import PER_THREAD, TAIL, Segment          # noqa: F401  (the landing layout's, re-exported)

BLOCK = 32                          # elements per e8m0 scale
SCALE_ES = 1
SCALE = ".weight_scale"
CODE = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)      # e2m1 magnitudes
NAN_BITS = 0x7E00
REFUSED = {"_scale_inv": "an inverse / block scale", "_zero_point": "a zero point (asymmetric quantisation)"}
REFUSED_NAMES = {".input_scale": "an activation scale (weights only are MXFP4 here; activations stay fp16)"}


# ------------------------------------------------------------------------------- the value
def unpack(packed: torch.Tensor) -> torch.Tensor:
    """Nibbles ``u`` (uint8, 0..15) of shape ``[out, in]`` from the bytes ``[out, in / 2]``."""
    if packed.dtype != torch.uint8 or packed.dim() != 2:
        raise TypeError(f"MXFP4 bytes are 2-D uint8, got {packed.dtype} {tuple(packed.shape)}")
    by = packed.detach().to("cpu")
    return torch.stack((by & 15, by >> 4), -1).reshape(by.shape[0], by.shape[1] * 2)


def pack(u: torch.Tensor) -> torch.Tensor:
    """Bytes ``[out, in / 2]`` of the nibbles ``u`` (0..15) of shape ``[out, in]``."""
    if u.dim() != 2 or u.shape[1] % 2:
        raise ValueError(f"MXFP4 weights are 2-D with an even row length, got shape {tuple(u.shape)}")
    v = u.detach().to("cpu").to(torch.uint8).reshape(u.shape[0], -1, 2)
    return (v[..., 0] | (v[..., 1] << 4)).contiguous()


def dequantize(packed: torch.Tensor, scale: torch.Tensor, shape: Sequence[int]) -> torch.Tensor:
    """``w16`` of shape ``shape`` = ``[out, in]`` from the bytes and the e8m0 block scales."""
    out, inn = (int(x) for x in shape)
    if inn % BLOCK or tuple(packed.shape) != (out, inn // 2):
        raise ValueError(f"MXFP4 bytes of a [{out}, {inn}] weight (in % 32 == 0) have shape [{out}, {inn // 2}], got "
                         f"{tuple(packed.shape)}")
    if scale.dtype != torch.uint8 or tuple(scale.shape) != (out, inn // BLOCK):
        raise TypeError(f"MXFP4 scales of a [{out}, {inn}] weight are U8 [{out}, {inn // BLOCK}], got {scale.dtype} "
                        f"{tuple(scale.shape)}")
    u = unpack(packed).numpy().reshape(out, inn // BLOCK, BLOCK)
    e = scale.detach().to("cpu").numpy().astype(np.int64).reshape(out, inn // BLOCK, 1)
    code = np.array(CODE + tuple(-c for c in CODE), dtype=np.float64)[u]
    with np.errstate(over="ignore"):
        w = (code * np.ldexp(1.0, e - 127)).astype(np.float16)        # exact in fp64, then one rounding
    w = np.where(e == 255, np.uint16(NAN_BITS), w.view(np.uint16)).astype(np.uint16)
    return torch.from_numpy(w.reshape(out, inn).view(np.float16))


def quantize(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(bytes U8 [out, in / 2], scales U8 [out, in / 32])`` by the OCP rule.  Per block
    ``e = clamp(floor(log2(amax)) - 2 + 127, 0, 254)`` (127 for an all-zero block); each element is
    ``w / 2^(e - 127)`` rounded to the nearest e2m1 value, ties to the even code, saturating at +-6."""
    if w.dim() != 2 or w.shape[1] % BLOCK:
        raise ValueError(f"MXFP4 weights are 2-D with in % 32 == 0, got shape {tuple(w.shape)}")
    out, inn = w.shape
    f = w.detach().to("cpu").to(torch.float64).reshape(out, inn // BLOCK, BLOCK)
    amax = f.abs().amax(-1, keepdim=True)
    k = torch.frexp(amax)[1].to(torch.int64) - 1                        # floor(log2(amax)) where amax > 0
    e = torch.where(amax > 0, (k - 2 + 127).clamp(0, 254), torch.full_like(k, 127))
    x = torch.ldexp(f, 127 - e).abs()
    # the index of the nearest magnitude: one comparison per midpoint of neighbouring codes, a tie
    # going to the neighbour with the even index (> keeps the lower one, >= takes the upper one)
    u = torch.zeros(f.shape, dtype=torch.uint8)
    for i in range(7):
        mid = (CODE[i] + CODE[i + 1]) / 2
        u += (x > mid) if i % 2 == 0 else (x >= mid)
    u |= torch.signbit(f).to(torch.uint8) << 3
    return pack(u.reshape(out, inn)), e.to(torch.uint8).reshape(out, inn // BLOCK)


# --------------------------------------------------------------------------- names
def is_companion_name(name: str) -> bool:
    """A tensor that belongs to an MXFP4 weight: its block scales."""
    return name.endswith(SCALE)


def weight_of_companion(name: str) -> str:
    """``X.weight`` for ``X.weight_scale``."""
    if not name.endswith(SCALE):
        raise ValueError(name)
    return name[:-len(SCALE)] + ".weight"


def is_mxfp4_source(weight_name: str, infos) -> bool:
    """``weight_name`` is a U8 tensor with an ``X.weight_scale`` next to it (U8, or :func:`check_entry`
    refuses it by name)."""
    return weight_name in infos and infos[weight_name].dtype == torch.uint8 and weight_name + "_scale" in infos


def check_entry(weight_name: str, infos, shape: Sequence[int], where: str = "") -> Tuple[str, str]:
    """Validate the tensors of MXFP4 weight ``weight_name`` whose placement has ``shape``.  ``infos``
    maps names to objects with ``dtype`` and ``shape`` (tensors, or safetensors header entries).
    Returns ``(packed name, scale name)``; TypeError naming the tensor otherwise."""
    sk = weight_name + "_scale"
    what = f"{where}{weight_name} (MXFP4)"
    stem = weight_name[:-len(".weight")] if weight_name.endswith(".weight") else weight_name
    for k, why in [(weight_name + suf, why) for suf, why in REFUSED.items()] + \
                  [(stem + suf, why) for suf, why in REFUSED_NAMES.items()]:
        if k in infos:
            raise TypeError(f"{what} has {why}, {k}; only e2m1 bytes with e8m0 block scales are supported")
    if len(tuple(shape)) != 2:
        raise TypeError(f"{what}: only 2-D projection weights may be MXFP4, this one has shape {tuple(shape)}")
    out, inn = (int(x) for x in shape)
    if inn % BLOCK:
        raise TypeError(f"{what}: the row length {inn} is no multiple of the MX block size 32")
    p = infos[weight_name]
    if p.dtype != torch.uint8 or tuple(p.shape) != (out, inn // 2):
        raise TypeError(f"{what}: packed as {p.dtype} {tuple(p.shape)}, a [{out}, {inn}] weight packs to U8 "
                        f"[{out}, {inn // 2}] (two weights per byte)")
    if sk not in infos:
        raise TypeError(f"{what} has no scale tensor {sk}")
    s = infos[sk]
    if s.dtype != torch.uint8:
        raise TypeError(f"{what}: {sk} has dtype {s.dtype}; MXFP4 scales are U8 (e8m0 exponent bytes)")
    if tuple(s.shape) != (out, inn // BLOCK):
        raise TypeError(f"{what}: {sk} has shape {tuple(s.shape)}, a [{out}, {inn}] weight has [{out}, {inn // BLOCK}] "
                        "scales (one per 32 elements of a row)")
    return weight_name, sk


def dequantize_entry(sd: Dict[str, torch.Tensor], weight_name: str, shape: Sequence[int], where: str = "") -> torch.Tensor:
    """``w16`` of MXFP4 weight ``weight_name`` of a state dict, validated against ``shape``."""
    pk, sk = check_entry(weight_name, sd, shape, where)
    return dequantize(sd[pk], sd[sk], shape)


# --------------------------------------------------------------------------- converter
def quantize_state_dict(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """``--quantize mxfp4`` of one file's tensors: every 2-D projection weight
    (``fp8.is_quantized_name``) of a float dtype becomes the bytes and their block scales; everything
    else, the tensors of a checkpoint that is MXFP4 already included, passes through."""
    out = {}
    for k, v in sd.items():
        if is_quantized_name(k) and v.dim() == 2 and v.dtype in (torch.float16, torch.bfloat16, torch.float32):
            out[k], out[k + "_scale"] = quantize(v)
        else:
            out[k] = v
    return out


def dequantize_state_dict(sd: Dict[str, torch.Tensor], where: str = "") -> Dict[str, torch.Tensor]:
    """The twin of one file's tensors: ``X.weight`` = ``w16``, the scale tensors dropped."""
    out = {}
    for k, v in sd.items():
        if is_companion_name(k) and is_mxfp4_source(weight_of_companion(k), sd):
            continue
        if is_mxfp4_source(k, sd):
            if v.dim() != 2:
                raise TypeError(f"{where}{k} (MXFP4): packed as {v.dtype} {tuple(v.shape)}, not U8 [out, in / 2]")
            out[k] = dequantize_entry(sd, k, (v.shape[0], v.shape[1] * 2), where)
        else:
            out[k] = v
    return out


def write_twin(src_dir: str, dst_dir: str) -> None:
    """Write the fp16 twin of the checkpoint directory ``src_dir`` to ``dst_dir``."""
    quant.write_twin(src_dir, dst_dir, dequantize_state_dict)


# --------------------------------------------------------------------------- landing layout
def _check(n: int, g: int, scale_es: int) -> None:
    if g != BLOCK or scale_es != SCALE_ES:
        raise ValueError(f"MXFP4 has blocks of 32 with one-byte scales, not {g} / {scale_es}")
    if n < 0 or n % BLOCK:
        raise ValueError(f"MXFP4: the {n} weights are no whole blocks of 32")


@functools.lru_cache(maxsize=256)
def region_layout(n: int, g: int = BLOCK, scale_es: int = SCALE_ES) -> Tuple[Segment, ...]:
    """The segments of a tensor of ``n`` weights in launch order (``quant.segments``), the arguments
    checked.  The host code of ``fls_dequant_mxfp4`` mirrors this function."""
    _check(n, g, scale_es)
    return quant.segments(n, g, scale_es)


# ``schedule(n, 32, 1)``, ``landing_span(n, 32, 1)``, ``land(region, packed_bytes, scale_bytes, n, 32, 1)``
# and ``unland(region, n, 32, 1)`` of quant.py, for this format's layout
schedule = functools.partial(quant.schedule, region_layout)
landing_span = functools.partial(quant.landing_span, region_layout)
land = functools.partial(quant.land, region_layout)
unland = functools.partial(quant.unland, region_layout)
