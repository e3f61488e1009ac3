"""What the weight-only checkpoint formats share: the format table, the 4-bit landing layout, the
twin writer, the ``--quantize`` dispatch and the checkpoint-name lookups of the loader.

The formats themselves (value definition, converter, checks) are :mod:`.fp8`, :mod:`.int4`,
:mod:`.nf4`, :mod:`.mxfp4` and :mod:`.gptq` (GPTQ and AWQ); the device kernels are
``csrc/kernels/dequant.hip`` and ``csrc/kernels/repack.hip``.

Landing layout of a 4-bit tensor (:func:`segments`).  A tensor of ``N`` weights owns its ``2N``-byte
region of the layer image and nothing else.  The kernel expands elements ``[a, b)`` per stream-ordered
launch, writing bytes ``[2a, 2b)``; a launch must not write a byte that is still unread.  Packed bytes
and scales both have to approach the top of the region as the element index approaches ``N``, which
two contiguous blocks cannot do, so the inputs land *segment by segment*, one segment per launch,
stacked downwards from the top of the region in reverse launch order:

    [ ... free ... | scales_0 | packed_0 | scales_1 | packed_1 | ... | scales_tail | packed_tail ]

``packed_j`` are the ``(b_j - a_j) / 2`` packed bytes of launch ``j``, ``scales_j`` the raw scale
bytes (as in the file) of the groups that *end* in ``[a_j, b_j)``, at a 16-byte aligned offset.  A
group that straddles a launch boundary is read by the earlier launch from the later segment, which
lies above it.  Launch ``j`` may run because ``2 b_j <= offset(scales_j)``: everything unread lies at
or above its own segment.  The segments are sized from the top: the tail holds at most ``TAIL``
weights, which one block reads into registers before a barrier and then writes; every segment below
takes as many weights as fit under the rule, about ``1 / (1/4 + es / 2g)`` times what lies above it,
so the chain is about ``log(N / TAIL) / log(3.2 .. 3.9)`` launches.
"""
from __future__ import annotations

import glob
import os
import shutil
from typing import Callable, Dict, List, NamedTuple, Optional, Tuple

import torch

from .utils.safetensors_io import load_file, save_file

PER_THREAD = 32                    # weights per kernel thread: one 16-byte load of nibbles
TAIL = PER_THREAD * 256            # weights the final single-block launch can hold


# --------------------------------------------------------------------------- landing layout
class Segment(NamedTuple):
    """One launch: elements ``[a, b)``; their packed bytes at region offset ``packed_off``; the
    ``n_groups`` scales of groups ``first_group ...`` (those that end in ``[a, b)``) at ``scale_off``."""
    a: int
    b: int
    packed_off: int
    scale_off: int
    first_group: int
    n_groups: int


Layout = Callable[[int, int, int], Tuple[Segment, ...]]     # a format's checked, cached region_layout


def segments(n: int, g: int, scale_es: int) -> Tuple[Segment, ...]:
    """The segments of a tensor of ``n`` weights in groups of ``g`` with ``scale_es``-byte scales, in
    launch order.  Built from the top of the ``2n``-byte region: the tail first, then each earlier
    launch as large as ``2 b <= scale_off`` allows.  The arguments are the caller's to check
    (``int4.region_layout``, ``nf4.region_layout``, ``mxfp4.region_layout``)."""
    segs: List[Segment] = []
    if n == 0:
        return ()
    top, b = 2 * n, n
    a = 0 if n <= TAIL else n - TAIL
    while True:
        k0, k1 = a // g, b // g
        p_off = top - (b - a) // 2
        s_off = (p_off - (k1 - k0) * scale_es) & ~15
        segs.append(Segment(a, b, p_off, s_off, k0, k1 - k0))
        if a == 0:
            break
        top, b = s_off, a
        # the next lower launch takes cnt weights: cnt / 2 packed bytes, at most cnt / g + 1 scales
        # and up to 15 bytes of alignment must fit between the write front 2b and `top`
        avail = top - 2 * b
        cnt = (avail - scale_es - 15) * 2 * g // (g + 2 * scale_es) // PER_THREAD * PER_THREAD
        if cnt <= 0:
            raise AssertionError("4-bit landing layout made no progress")
        a = max(0, b - cnt)
    return tuple(reversed(segs))


def schedule(layout: Layout, n: int, g: int, scale_es: int) -> List[Tuple[int, int]]:
    """The ``[a, b)`` element ranges of the kernel's launches, in order."""
    return [(s.a, s.b) for s in layout(n, g, scale_es)]


def landing_span(layout: Layout, n: int, g: int, scale_es: int) -> Tuple[int, int]:
    """``(offset, bytes)`` of the part of the region the landed inputs occupy: from the first
    segment's scales to the end of the region."""
    lay = layout(n, g, scale_es)
    return (lay[0].scale_off, 2 * n - lay[0].scale_off) if lay else (0, 0)


def land(layout: Layout, region: torch.Tensor, packed_bytes: torch.Tensor, scale_bytes: torch.Tensor, n: int,
         g: int, scale_es: int) -> None:
    """Place a tensor's packed bytes (``n / 2``) and raw scale bytes into the uint8 ``region`` the way
    the loader does (tests, benchmarks)."""
    for s in layout(n, g, scale_es):
        region[s.packed_off:s.packed_off + (s.b - s.a) // 2].copy_(packed_bytes[s.a // 2:s.b // 2])
        if s.n_groups:
            region[s.scale_off:s.scale_off + s.n_groups * scale_es].copy_(
                scale_bytes[s.first_group * scale_es:(s.first_group + s.n_groups) * scale_es])


def unland(layout: Layout, region: torch.Tensor, n: int, g: int, scale_es: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The inverse of :func:`land` on a CPU uint8 ``region``: ``(packed bytes, raw scale bytes)``."""
    packed = torch.empty(n // 2, dtype=torch.uint8)
    scales = torch.empty(n // g * scale_es, dtype=torch.uint8)
    for s in layout(n, g, scale_es):
        packed[s.a // 2:s.b // 2] = region[s.packed_off:s.packed_off + (s.b - s.a) // 2]
        scales[s.first_group * scale_es:(s.first_group + s.n_groups) * scale_es] = \
            region[s.scale_off:s.scale_off + s.n_groups * scale_es]
    return packed, scales


# --------------------------------------------------------------------------- twin writer
def write_twin(src_dir: str, dst_dir: str, dequantize_state_dict) -> None:
    """Write the fp16 twin of the checkpoint directory ``src_dir`` (per-layer files or an HF directory
    of safetensors files) to ``dst_dir``: every file's tensors through ``dequantize_state_dict(sd,
    where)``, everything else copied."""
    os.makedirs(dst_dir, exist_ok=True)
    for fn in sorted(glob.glob(os.path.join(src_dir, "*"))):
        base = os.path.basename(fn)
        if os.path.isdir(fn):
            continue
        if base.endswith(".safetensors"):
            save_file(dequantize_state_dict(load_file(fn), base + ": "), os.path.join(dst_dir, base))
        else:
            shutil.copy(fn, os.path.join(dst_dir, base))


# --------------------------------------------------------------------------- the format table
from . import fp8, gptq, int4, mxfp4, nf4   # noqa: E402  (the 4-bit modules import the landing layout above)


class Format(NamedTuple):
    name: str           # ``--quantize`` value, ``TensorRun.fmt``, the ``<name>_tensors`` counters
    label: str
    module: object
    verbose: str        # what ``--verbose`` says of a checkpoint that holds ``n`` such tensors


FORMATS = (
    Format("fp8", "FP8", fp8, "FP8 checkpoint: {n} e4m3 tensors are expanded to fp16 in HBM (weight-only FP8); "
                              "{ignored} input_scale tensors are ignored: activations stay fp16"),
    Format("int4", "INT4", int4, "INT4 checkpoint: {n} W4A16 tensors are expanded to fp16 in HBM (weight-only INT4)"),
    Format("nf4", "NF4", nf4, "NF4 checkpoint: {n} bitsandbytes 4-bit tensors are expanded to fp16 in HBM"),
)
BY_NAME = {f.name: f for f in FORMATS}
SEGMENTED = ("int4", "nf4")           # the 4-bit formats: they land segment by segment
# FORMATS, BY_NAME and SEGMENTED are frozen at the three formats above: tests/test_quant_cpu.py pins
# them entry for entry and lines them up with fixed tuples such as ``(is_fp8, is_int4, is_nf4)``.
# Nothing in the package reads them any more and new code MUST NOT: it would miss every format added
# since.  The tables below are the ones the loader, the converter and the metrics go through.
ALL_FORMATS = FORMATS + (
    Format("mxfp4", "MXFP4", mxfp4, "MXFP4 checkpoint: {n} e2m1 tensors with e8m0 block scales are expanded to fp16 in HBM"),
    Format("gptq", "GPTQ", gptq, "GPTQ checkpoint: {n} 4-bit tensors are repacked and expanded to fp16 in HBM"),
    Format("awq", "AWQ", gptq, "AWQ checkpoint: {n} 4-bit GEMM-layout tensors are repacked and expanded to fp16 in HBM"),
)
FORMAT_BY_NAME = {f.name: f for f in ALL_FORMATS}
LANDS_SEGMENTED = SEGMENTED + ("mxfp4",)
# GPTQ and AWQ: the file tensors land contiguous at the bottom of the region, one launch repacks them
# into the segmented layout at its top, then the chain expands them (gptq.py)
LANDS_REPACKED = ("gptq", "awq")
LANDS_IN_PIECES = LANDS_SEGMENTED + LANDS_REPACKED      # every format whose tensors land as several pieces


def quantize_format(quantize: str) -> Format:
    """The format ``--quantize`` names; ValueError otherwise."""
    if quantize not in FORMAT_BY_NAME:
        raise ValueError(f"--quantize {quantize!r}: fp8, int4 or nf4, or mxfp4, gptq or awq")
    return FORMAT_BY_NAME[quantize]


def quantize_state_dict(sd: Dict[str, torch.Tensor], quantize: str, fp8_scale: str = "channel",
                        int4_group: int = 128, int4_scale_dtype=torch.float16, nf4_block: int = 64,
                        nf4_double_quant: bool = True) -> Dict[str, torch.Tensor]:
    """``--quantize`` of one file's tensors: the named format's own ``quantize_state_dict`` with its
    own options."""
    args = {"fp8": (fp8_scale,), "int4": (int4_group, int4_scale_dtype), "nf4": (nf4_block, nf4_double_quant),
            "gptq": ("gptq", int4_group), "awq": ("awq", int4_group)}
    return quantize_format(quantize).module.quantize_state_dict(sd, *args.get(quantize, ()))


# --------------------------------------------------------------------------- checkpoint names
def is_companion(name: str, want) -> bool:
    """``name`` belongs to a weight among ``want`` in some format: an FP8 scale, the words, scales or
    shape of an INT4 weight, the absmax, code books or quant state of a bitsandbytes 4-bit weight, the
    block scales of an MXFP4 weight, the words, zero points, scales or group index of a GPTQ / AWQ
    weight."""
    return ((fp8.is_scale_name(name) and fp8.weight_of_scale(name) in want)
            or any(m.is_companion_name(name) and m.weight_of_companion(name) in want
                   for m in (int4, nf4, mxfp4, gptq)))


def source(weight_name: str, infos, where: str = "") -> Tuple[Optional[str], Optional[str]]:
    """``(format, key)`` of what feeds weight ``weight_name`` from the tensors ``infos`` (name ->
    object with a ``dtype``): the format is None for a tensor that is not quantised, the key is
    ``X.weight_packed`` for an INT4 weight, ``X.qweight`` for a GPTQ / AWQ weight, the weight's own
    name otherwise, None if it is absent."""
    pk, qk = int4.packed_name(weight_name), gptq.qweight_name(weight_name)
    if weight_name not in infos:
        if pk in infos:
            return "int4", pk
        return (gptq.source_format(weight_name, infos), qk) if qk in infos else (None, None)
    if pk in infos:
        raise TypeError(f"{where}{weight_name} is stored twice, as itself and as INT4 words ({pk}); a layer file "
                        "holds one of the two")
    if qk in infos:
        raise TypeError(f"{where}{weight_name} is stored twice, as itself and as GPTQ / AWQ words ({qk}); a layer "
                        "file holds one of the two")
    if nf4.is_nf4_source(weight_name, infos):
        return "nf4", weight_name
    if mxfp4.is_mxfp4_source(weight_name, infos):
        return "mxfp4", weight_name
    return ("fp8" if infos[weight_name].dtype == fp8.FP8_DTYPE else None), weight_name
