"""GPTQ and AWQ 4-bit checkpoints (asymmetric, group-scaled, input-major): the host definition.

A 2-D projection weight ``X.weight`` of model shape ``[out, in]``, ``N = out * in``, in groups of
``g`` consecutive inputs (``g`` a multiple of 32 that divides ``in``; ``g == in`` is per channel,
``group_size: -1``), is stored in one of two layouts, told apart by the shape of ``X.qweight``:

**GPTQ** (the tensors AutoGPTQ is understood to write)

    X.qweight  I32 [in / 8, out]      nibble i (bits [4i, 4i + 4)) of word [r, o] is u[o, 8r + i]
    X.qzeros   I32 [in / g, out / 8]  nibble i of word [j, c] is zs[j, 8c + i];  z = (zs + 1) & 15
    X.scales   F16 [in / g, out]
    X.g_idx    I32 [in]               optional; must equal k // g (no activation order)

**AWQ** (AutoAWQ's GEMM version)

    X.qweight  I32 [in, out / 8]      nibble i of word [k, c] is u[8c + P[i], k],  P = (0, 2, 4, 6, 1, 3, 5, 7)
    X.qzeros   I32 [in / g, out / 8]  the same nibble order;  z = zs
    X.scales   F16 [in / g, out]

The value, for both:

    w16[o, k] = fp16_rne( fp32(u[o, k] - z[k // g, o]) * fp32(s[k // g, o]) )

The difference lies in -15..15 and the scale has 11 significant bits, so the fp32 product is exact
and the value is rounded once (overflow to +-inf, NaN from a NaN scale, ``0 * negative`` is -0).
Neither library was at hand when this was written: the layouts are pinned by literal known answers
in the tests, compatibility with files of those libraries is intended and unverified.

The *fp16 twin* is the same directory with ``X.weight`` written as ``w16`` and the companions
removed (:func:`write_twin`): a run on the checkpoint gives, bit for bit, the run on its twin.

Landing (:func:`input_layout`): the three file tensors land as they are at the *bottom* of the
tensor's own ``2N``-byte region, ``qweight`` at 0, then ``scales``, then ``qzeros``.  One launch of
``fls_repack_w4`` (``csrc/kernels/repack.hip``) transposes them into INT4's segmented landing layout
at the *top* of the region (:func:`region_layout`: ``quant.segments`` with 4-byte group entries,
``fp16 s | u16 z``), and ``fls_dequant_w4z`` (``csrc/kernels/dequant.hip``) expands those segments in
place.  The input ends below the first segment for every ``g >= 32`` (about ``0.52 N`` against
``2N - 0.63 N``); :func:`input_layout` checks it.
"""
from __future__ import annotations

import functools
import json
import os
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import torch

from . import quant
from .fp8 import is_quantized_name
from .quant import PER_THREAD, TAIL, Segment          # noqa: F401  (the landing layout's, re-exported)

LAYOUTS = ("gptq", "awq")
LAYOUT_CODES = {"gptq": 0, "awq": 1}                 # fls_repack_w4's layout
AWQ_ORDER = (0, 2, 4, 6, 1, 3, 5, 7)                 # P: nibble i holds column 8c + P[i]
ENTRY_ES = 4                                         # bytes of a repacked group entry (fp16 s, u16 z)
QWEIGHT, QZEROS, SCALES, G_IDX = ".qweight", ".qzeros", ".scales", ".g_idx"
_SUFFIXES = (QWEIGHT, QZEROS, SCALES, G_IDX)
_SHIFTS = torch.arange(8, dtype=torch.int32) * 4


# ------------------------------------------------------------------------------- the value
def _nibbles(words: torch.Tensor) -> torch.Tensor:
    """``[..., 8]`` uint8 nibbles of int32 words, nibble i last-index i."""
    if words.dtype != torch.int32 or words.dim() != 2:
        raise TypeError(f"4-bit words are 2-D int32, got {words.dtype} {tuple(words.shape)}")
    w = words.detach().to("cpu").contiguous()
    return ((w.unsqueeze(-1) >> _SHIFTS) & 15).to(torch.uint8)


def _words(nib: torch.Tensor) -> torch.Tensor:
    """int32 words of ``[..., 8]`` nibbles (the inverse of :func:`_nibbles`)."""
    w = (nib.to(torch.int64) << (_SHIFTS.to(torch.int64))).sum(-1)
    return (w - ((w >> 31) << 32)).to(torch.int32)            # (bit 31 set: the negative int32)


def _order(layout: str) -> torch.Tensor:
    if layout not in LAYOUTS:
        raise ValueError(f"layout {layout!r}: gptq or awq")
    return torch.tensor(AWQ_ORDER if layout == "awq" else range(8))


def unpack_columns(words: torch.Tensor, layout: str) -> torch.Tensor:
    """uint8 ``[rows, 8 * cols]`` from words ``[rows, cols]`` packed along the columns (both layouts'
    ``qzeros``, AWQ's ``qweight``): column ``8c + order[i]`` is nibble ``i`` of word ``c``."""
    nib = _nibbles(words)
    out = torch.empty_like(nib)
    out[..., _order(layout)] = nib
    return out.reshape(words.shape[0], words.shape[1] * 8)


def pack_columns(v: torch.Tensor, layout: str) -> torch.Tensor:
    rows, cols = v.shape
    return _words(v.reshape(rows, cols // 8, 8)[..., _order(layout)])


def unpack(qweight: torch.Tensor, layout: str) -> torch.Tensor:
    """``u`` (uint8, 0..15) of model shape ``[out, in]`` from the ``qweight`` words of ``layout``."""
    if layout == "awq":
        return unpack_columns(qweight, layout).t().contiguous()
    _order(layout)
    nib = _nibbles(qweight)                                    # [in / 8, out, 8]
    return nib.permute(1, 0, 2).reshape(qweight.shape[1], qweight.shape[0] * 8).contiguous()


def pack(u: torch.Tensor, layout: str) -> torch.Tensor:
    """The ``qweight`` words of ``layout`` of the values ``u`` in 0..15 of shape ``[out, in]``."""
    if u.dim() != 2 or u.shape[0] % 8 or u.shape[1] % 8:
        raise ValueError(f"4-bit weights are 2-D with out % 8 == 0 and in % 8 == 0, got shape {tuple(u.shape)}")
    v = u.detach().to("cpu")
    if v.numel() and (int(v.min()) < 0 or int(v.max()) > 15):
        raise ValueError("4-bit values lie in 0..15")
    if layout == "awq":
        return pack_columns(v.t().contiguous(), layout)
    _order(layout)
    out, inn = v.shape
    return _words(v.reshape(out, inn // 8, 8).permute(1, 0, 2))


def zero_points(qzeros: torch.Tensor, layout: str) -> torch.Tensor:
    """``z`` (uint8, 0..15) of shape ``[in / g, out]``: GPTQ stores ``z - 1`` modulo 16."""
    zs = unpack_columns(qzeros, layout)
    return (zs + 1) & 15 if layout == "gptq" else zs


def pack_zero_points(z: torch.Tensor, layout: str) -> torch.Tensor:
    return pack_columns((z.to(torch.int16) - 1) & 15 if layout == "gptq" else z, layout)


def layout_of(qweight_shape: Sequence[int], scales_shape: Sequence[int]) -> Optional[str]:
    """``"gptq"`` for ``[in / 8, out]``, ``"awq"`` for ``[in, out / 8]``, given scales ``[in / g, out]``;
    None if the shapes fit neither."""
    qs, ss = tuple(qweight_shape), tuple(scales_shape)
    if len(qs) != 2 or len(ss) != 2:
        return None
    if qs[1] == ss[1]:
        return "gptq"
    if qs[1] * 8 == ss[1]:
        return "awq"
    return None


def dequantize(qweight: torch.Tensor, qzeros: torch.Tensor, scales: torch.Tensor,
               layout: Optional[str] = None) -> torch.Tensor:
    """``w16`` of model shape ``[out, in]`` from the three file tensors (the layout by shape if not
    given)."""
    layout = layout or layout_of(qweight.shape, scales.shape)
    if layout not in LAYOUTS:
        raise ValueError(f"qweight {tuple(qweight.shape)} with scales {tuple(scales.shape)} is neither GPTQ's "
                         "[in / 8, out] nor AWQ's [in, out / 8]")
    if scales.dtype != torch.float16:
        raise TypeError(f"GPTQ / AWQ scales are fp16, got {scales.dtype}")
    u = unpack(qweight, layout)
    out, inn = u.shape
    G = scales.shape[0]
    if tuple(scales.shape) != (G, out) or G == 0 or inn % G or tuple(qzeros.shape) != (G, out // 8):
        raise ValueError(f"a [{out}, {inn}] weight has scales [in / g, {out}] and qzeros [in / g, {out // 8}], got "
                         f"{tuple(scales.shape)} and {tuple(qzeros.shape)}")
    g = inn // G
    z = zero_points(qzeros, layout).t().to(torch.int16).reshape(out, G, 1)
    s = scales.detach().to("cpu").t().to(torch.float32).reshape(out, G, 1)
    d = (u.to(torch.int16).reshape(out, G, g) - z).to(torch.float32)
    return (d * s).to(torch.float16).reshape(out, inn)


def quantize(w: torch.Tensor, layout: str, group: int = 128):
    """``(qweight, qzeros, scales)`` of ``layout``, round to nearest.  Per group of ``g`` consecutive
    inputs of a row: ``lo = min(w, 0)``, ``hi = max(w, 0)``, ``s = fp16((hi - lo) / 15)`` (1 for an
    all-zero group; the next lower fp16 where ``15 s`` would round to inf), ``z = clamp(round(-lo /
    s), 0, 15)``, ``u = clamp(round(w / s) + z, 0, 15)``.  ``group <= 0``: per channel (``g = in``)."""
    _order(layout)
    if w.dim() != 2:
        raise ValueError(f"4-bit weights are 2-D, got shape {tuple(w.shape)}")
    out, inn = w.shape
    g = inn if group <= 0 else int(group)
    if out % 8 or inn % 32 or g % 32 or inn % g:
        raise ValueError(f"--int4_group {g}: a multiple of 32 that divides the row length {inn} (in % 32 == 0, "
                         f"out % 8 == 0; this weight is [{out}, {inn}])")
    f = w.detach().to("cpu").to(torch.float32).reshape(out, inn // g, g)
    lo, hi = f.amin(-1).clamp(max=0), f.amax(-1).clamp(min=0)
    s = ((hi - lo) / 15.0).to(torch.float16)
    s = torch.where(s == 0, torch.ones_like(s), s)
    s = torch.where(torch.isinf(s), torch.full_like(s, torch.finfo(torch.float16).max), s)
    over = torch.isinf((s.to(torch.float32) * 15.0).to(torch.float16))
    if bool(over.any()):
        s = torch.where(over, (s.view(torch.int16) - 1).view(torch.float16), s)   # (s > 0: the next lower value)
    s32 = s.to(torch.float32)
    z = torch.clamp(torch.round(-lo / s32), 0, 15)
    u = torch.clamp(torch.round(f / s32.unsqueeze(-1)) + z.unsqueeze(-1), 0, 15)
    return (pack(u.reshape(out, inn).to(torch.uint8), layout),
            pack_zero_points(z.t().contiguous().to(torch.uint8), layout), s.t().contiguous())


# --------------------------------------------------------------------------- names
def is_companion_name(name: str) -> bool:
    """A tensor that belongs to a GPTQ / AWQ weight: its words, zero points, scales or group index."""
    return name.endswith(_SUFFIXES)


def weight_of_companion(name: str) -> str:
    """``X.weight`` for ``X.qweight`` / ``X.qzeros`` / ``X.scales`` / ``X.g_idx``."""
    for suf in _SUFFIXES:
        if name.endswith(suf):
            return name[:-len(suf)] + ".weight"
    raise ValueError(name)


def stem(weight_name: str) -> str:
    return weight_name[:-len(".weight")] if weight_name.endswith(".weight") else weight_name


def qweight_name(weight_name: str) -> str:
    return stem(weight_name) + QWEIGHT


def source_format(weight_name: str, infos) -> Optional[str]:
    """``"gptq"`` / ``"awq"`` if ``infos`` holds ``X.qweight`` for ``weight_name``, by its shape (GPTQ
    where the shapes fit neither: :func:`check_entry` then refuses it by name); None otherwise."""
    qk, sk = qweight_name(weight_name), stem(weight_name) + SCALES
    if qk not in infos:
        return None
    return (layout_of(infos[qk].shape, infos[sk].shape) if sk in infos else None) or "gptq"


class Entry(NamedTuple):
    layout: str
    qweight: str
    qzeros: str
    scales: str
    g_idx: Optional[str]
    group: int


def check_entry(weight_name: str, infos, shape: Sequence[int], where: str = "") -> Entry:
    """Validate the tensors of GPTQ / AWQ weight ``weight_name`` whose placement has ``shape``.
    ``infos`` maps names to objects with ``dtype`` and ``shape`` (tensors, or safetensors header
    entries).  TypeError naming the tensor otherwise.  The *contents* of ``X.g_idx`` are the caller's
    to compare (:func:`check_g_idx`)."""
    st = stem(weight_name)
    qk, zk, sk, gk = st + QWEIGHT, st + QZEROS, st + SCALES, st + G_IDX
    what = f"{where}{weight_name} (GPTQ / AWQ)"
    if len(tuple(shape)) != 2:
        raise TypeError(f"{what}: only 2-D projection weights may be GPTQ / AWQ, this placement has shape "
                        f"{tuple(shape)}")
    out, inn = (int(x) for x in shape)
    for k in (zk, sk):
        if k not in infos:
            raise TypeError(f"{what} has no {k}")
    q, z, s = infos[qk], infos[zk], infos[sk]
    for k, t, dt in ((qk, q, torch.int32), (zk, z, torch.int32), (sk, s, torch.float16)):
        if t.dtype != dt:
            raise TypeError(f"{what}: {k} has dtype {t.dtype}; qweight and qzeros are I32 (eight nibbles per word, "
                            "4 bits), scales are F16")
    if out % 8 or inn % 32:
        raise TypeError(f"{what}: a [{out}, {inn}] weight needs out % 8 == 0 and in % 32 == 0")
    if tuple(q.shape) == (inn // 8, out):
        layout = "gptq"
    elif tuple(q.shape) == (inn, out // 8):
        layout = "awq"
    else:
        raise TypeError(f"{what}: {qk} has shape {tuple(q.shape)}, a [{out}, {inn}] weight packs to [{inn // 8}, {out}] "
                        f"(GPTQ) or [{inn}, {out // 8}] (AWQ GEMM) at 4 bits")
    ss = tuple(s.shape)
    if len(ss) != 2 or ss[1] != out or ss[0] < 1 or inn % ss[0] or (inn // ss[0]) % 32:
        raise TypeError(f"{what}: {sk} has shape {ss}; scales are [in / g, {out}] with a group size g that is a "
                        f"multiple of 32 dividing {inn}, or {inn} itself")
    if tuple(z.shape) != (ss[0], out // 8):
        raise TypeError(f"{what}: {zk} has shape {tuple(z.shape)}, not [{ss[0]}, {out // 8}]")
    if gk in infos:
        gi = infos[gk]
        if layout != "gptq" or gi.dtype != torch.int32 or tuple(gi.shape) != (inn,):
            raise TypeError(f"{what}: {gk} is {gi.dtype} {tuple(gi.shape)}; a GPTQ group index is I32 [{inn}]")
    return Entry(layout, qk, zk, sk, gk if gk in infos else None, inn // ss[0])


def check_g_idx(weight_name: str, values: torch.Tensor, group: int, where: str = "") -> None:
    """``X.g_idx`` must be ``k // g``: activation order (``desc_act``) permutes the inputs of a group
    and is refused."""
    want = torch.arange(values.numel(), dtype=torch.int64) // group
    if not torch.equal(values.to(torch.int64).reshape(-1), want):
        raise TypeError(f"{where}{weight_name} (GPTQ): {stem(weight_name) + G_IDX} is not k // {group}: activation "
                        "order (desc_act) is not supported")


def check_quantization_config(model_dir: str) -> None:
    """Refuse what ``config.json``'s ``quantization_config`` says cannot be read: other bit widths,
    GPTQ's v2 checkpoint format, AWQ versions other than GEMM, activation order.  A directory without
    one (a converted synthetic checkpoint) passes."""
    try:
        with open(os.path.join(model_dir, "config.json")) as f:
            qc = json.load(f).get("quantization_config") or {}
    except (OSError, ValueError):
        return
    what = f"{model_dir}: quantization_config"
    if "bits" in qc and int(qc["bits"]) != 4:
        raise TypeError(f"{what}.bits is {qc['bits']}; only 4-bit GPTQ / AWQ checkpoints are supported")
    if str(qc.get("checkpoint_format", "gptq")).lower() != "gptq":
        raise TypeError(f"{what}.checkpoint_format is {qc['checkpoint_format']!r}; only the original GPTQ format "
                        "(zero points stored minus one) is supported")
    if str(qc.get("quant_method", "")).lower() == "awq" and str(qc.get("version", "gemm")).lower() != "gemm":
        raise TypeError(f"{what}.version is {qc['version']!r}; only AWQ's GEMM layout is supported")
    if qc.get("desc_act"):
        raise TypeError(f"{what}.desc_act is set: activation order is not supported")


def dequantize_entry(sd: Dict[str, torch.Tensor], weight_name: str, shape: Sequence[int], where: str = "") -> torch.Tensor:
    """``w16`` of GPTQ / AWQ weight ``weight_name`` of a state dict, validated against ``shape``."""
    e = check_entry(weight_name, sd, shape, where)
    if e.g_idx is not None:
        check_g_idx(weight_name, sd[e.g_idx], e.group, where)
    return dequantize(sd[e.qweight], sd[e.qzeros], sd[e.scales], e.layout)


# --------------------------------------------------------------------------- converter
def quantize_state_dict(sd: Dict[str, torch.Tensor], layout: str, group: int = 128) -> Dict[str, torch.Tensor]:
    """``--quantize gptq|awq`` of one file's tensors: every 2-D projection weight
    (``fp8.is_quantized_name``) of a float dtype becomes its companions (GPTQ: with the ``g_idx``
    AutoGPTQ always writes); everything else, the companions of a checkpoint that is in either format
    already included, passes through."""
    out = {}
    for k, v in sd.items():
        if is_quantized_name(k) and v.dim() == 2 and v.dtype in (torch.float16, torch.bfloat16, torch.float32):
            st = stem(k)
            out[st + QWEIGHT], out[st + QZEROS], out[st + SCALES] = quantize(v, layout, group)
            if layout == "gptq":
                g = v.shape[1] if group <= 0 else int(group)
                out[st + G_IDX] = (torch.arange(v.shape[1]) // g).to(torch.int32)
        else:
            out[k] = v
    return out


def dequantize_state_dict(sd: Dict[str, torch.Tensor], where: str = "") -> Dict[str, torch.Tensor]:
    """The twin of one file's tensors: ``X.weight`` = ``w16`` in the place of ``X.qweight``, the other
    companions dropped."""
    out = {}
    for k, v in sd.items():
        if k.endswith(QWEIGHT):
            w = weight_of_companion(k)
            sk = stem(w) + SCALES
            lay = layout_of(v.shape, sd[sk].shape) if sk in sd else None
            if lay is None:
                raise TypeError(f"{where}{w} (GPTQ / AWQ): {k} {tuple(v.shape)} has no scales that fit it")
            shape = (v.shape[1], v.shape[0] * 8) if lay == "gptq" else (v.shape[1] * 8, v.shape[0])
            out[w] = dequantize_entry(sd, w, shape, where)
        elif k.endswith(_SUFFIXES) and qweight_name(weight_of_companion(k)) in sd:
            continue
        else:
            out[k] = v
    return out


def write_twin(src_dir: str, dst_dir: str) -> None:
    """Write the fp16 twin of the checkpoint directory ``src_dir`` to ``dst_dir``."""
    quant.write_twin(src_dir, dst_dir, dequantize_state_dict)


# --------------------------------------------------------------------------- landing layout
def _check(out: int, inn: int, g: int) -> None:
    if out <= 0 or inn <= 0 or out % 8 or inn % 32 or g <= 0 or g % 32 or inn % g:
        raise ValueError(f"GPTQ / AWQ: a [{out}, {inn}] weight in groups of {g} needs out % 8 == 0, in % 32 == 0 and "
                         "a group that is a multiple of 32 dividing in")


@functools.lru_cache(maxsize=256)
def region_layout(n: int, g: int, scale_es: int = ENTRY_ES) -> Tuple[Segment, ...]:
    """The segments the repack writes and ``fls_dequant_w4z`` expands, in launch order
    (``quant.segments`` with 4-byte entries).  ``fls_dequant_w4z_segment`` mirrors this function."""
    if scale_es != ENTRY_ES or g <= 0 or g % 32 or n < 0 or n % g:
        raise ValueError(f"GPTQ / AWQ: group {g} must be a multiple of 32 that divides the {n} weights (entries of "
                         f"{ENTRY_ES} bytes, not {scale_es})")
    return quant.segments(n, g, ENTRY_ES)


schedule = functools.partial(quant.schedule, region_layout)


@functools.lru_cache(maxsize=256)
def input_layout(out: int, inn: int, g: int) -> Tuple[Tuple[int, int], ...]:
    """``((offset, bytes), ...)`` of ``qweight``, ``scales`` and ``qzeros`` at the bottom of the
    ``2 * out * inn``-byte region, each at a 16-byte aligned offset.  ValueError if the input would not
    end below the first segment of :func:`region_layout` (it does for every ``g >= 32``).
    ``fls_repack_w4_input`` mirrors this function."""
    _check(out, inn, g)
    n, G = out * inn, inn // g
    q = (0, n // 2)
    s = ((q[0] + q[1] + 15) & ~15, G * out * 2)
    z = ((s[0] + s[1] + 15) & ~15, G * (out // 8) * 4)
    if z[0] + z[1] > region_layout(n, g)[0].scale_off:
        raise ValueError(f"GPTQ / AWQ: the landed input of a [{out}, {inn}] weight in groups of {g} ends at byte "
                         f"{z[0] + z[1]}, above the first repacked segment")
    return q, s, z


def landing_span(out: int, inn: int, g: int) -> Tuple[int, int]:
    """``(offset, bytes)`` of the part of the region the landed file tensors occupy."""
    z = input_layout(out, inn, g)[2]
    return 0, z[0] + z[1]


def land(region: torch.Tensor, qweight: torch.Tensor, scales: torch.Tensor, qzeros: torch.Tensor, g: int) -> None:
    """Place the three file tensors into the uint8 ``region`` the way the loader does (tests,
    benchmarks)."""
    lay = layout_of(qweight.shape, scales.shape)
    out, inn = (qweight.shape[1], qweight.shape[0] * 8) if lay == "gptq" else (qweight.shape[1] * 8, qweight.shape[0])
    for t, (off, nb) in zip((qweight, scales, qzeros), input_layout(out, inn, g)):
        region[off:off + nb].copy_(t.detach().to("cpu").contiguous().view(torch.uint8).reshape(-1))


def unland(region: torch.Tensor, out: int, inn: int, g: int, layout: str):
    """The inverse of :func:`land` on a CPU uint8 ``region``: ``(qweight, scales, qzeros)``."""
    (qo, qn), (so, sn), (zo, zn) = input_layout(out, inn, g)
    qshape = (inn // 8, out) if layout == "gptq" else (inn, out // 8)
    return (region[qo:qo + qn].clone().view(torch.int32).reshape(qshape),
            region[so:so + sn].clone().view(torch.float16).reshape(inn // g, out),
            region[zo:zo + zn].clone().view(torch.int32).reshape(inn // g, out // 8))
