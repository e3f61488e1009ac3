"""Weight streaming from per-layer safetensors files (``--weight_cache stream``).

Reference (``/root/reference/utils.py:121-131``; DP ``utils.py:72-73``): every
time a layer is needed its file is read whole into a Python ``bytes`` object,
deserialised on the CPU, and each tensor is copied to the GPU (pageable,
synchronous) with a cast to fp16.  Host RAM needed: about one layer; the model
itself never has to fit in RAM (README: 70B with >= 8 GB of RAM).

Here the same small-RAM envelope costs no CPU work per pass:

* the packed HBM image of a layer is the checkpoint's own tensors concatenated
  (:mod:`..models.layout`), so a layer is a set of *file byte ranges* with a
  destination offset each (:class:`LayerPlan`);
* the native streamer (``fls_streamer_*`` in ``csrc/runtime/runtime.cpp``)
  reads those ranges with a persistent ``pread`` pool (optionally
  ``O_DIRECT``) into a small ring of pinned chunks (default 6 x 64 MiB) and
  DMAs every piece straight to its place in the HBM weight slot on the copy
  stream, so disk reads, PCIe DMA and compute of the previous shard overlap;
* bf16 tensors are converted to fp16 in place in HBM by a HIP kernel on the
  copy stream (``fls_cast_f16``); fp32 tensors (norm weights of mixed
  checkpoints) are converted on the host while they sit in the pinned chunk;
* FP8 (e4m3fn) tensors of a weight-only FP8 checkpoint (:mod:`..fp8`) are read and copied as
  they are, one byte per weight, into the upper half of the tensor's own region of the image,
  and expanded to fp16 in place there by ``fls_dequant_fp8`` on the copy stream, scaled by the
  tensor's scales (read once at plan time, resident on the device in one arena per source);
* INT4 tensors of a weight-only W4A16 checkpoint (:mod:`..int4`) are read and copied as they are,
  nibbles and raw group scales, segment by segment into the top of the tensor's own region of the
  image (``int4.region_layout``) and expanded to fp16 in place there by ``fls_dequant_int4`` on the
  copy stream; the scales travel with the weights and take no device memory of their own;
* bitsandbytes 4-bit (NF4 / FP4) tensors (:mod:`..nf4`) land the same way, packed bytes and raw
  absmax bytes segment by segment (``nf4.region_layout``), and are expanded by ``fls_dequant_nf4``;
  their small tables (code books, nested absmax, offset) are read at plan time and live in the
  source's device arena next to the FP8 scales.

Data-parallel ranks stream only their 1/G byte range of the packed image
(:meth:`LayerPlan.pieces`) and complete the layer with an RCCL all-gather
(:mod:`..parallel.data_parallel`): each layer file is read from disk once per
pass for all GPUs, like the reference's shared host cache.
"""
from __future__ import annotations

import ctypes
import os
import threading
import time
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from .. import _native, fp8, int4, knobs, nf4
from ..config import ModelConfig
from ..models.layout import check_layer_tensors, layer_kind, layer_layout, placements, source_key
from ..utils.layer_format import layer_file
from ..utils.safetensors_io import TensorInfo, read_header
from . import hostmem
from .weights import LayerSource

KIND_RAW, KIND_F32 = 0, 1
_SRC_ES = {torch.float16: 2, torch.bfloat16: 2, torch.float32: 4, fp8.FP8_DTYPE: 1}
_ABSMAX_DTYPE = {nf4.ABSMAX_F32: torch.float32, nf4.ABSMAX_U8: torch.uint8}


@dataclass(frozen=True)
class TensorRun:
    """One checkpoint tensor: file bytes [file_off, file_off + numel * src_es) -> image bytes
    [img_off, img_off + 2 * numel).

    An FP8 tensor (``src_es`` 1, weight-only FP8: :mod:`..fp8`) lands as raw bytes in the upper
    half ``[img_off + numel, img_off + 2 * numel)`` of its region and is expanded to fp16 in place
    there; ``scale`` is its flat fp32 scale (read at plan time), ``scale_kind`` one of
    ``fp8.KIND_*``, ``cols`` the tensor's row length.

    An INT4 tensor (``group`` > 0, weight-only W4A16: :mod:`..int4`) is ``numel / 2`` bytes of
    nibbles at ``file_off`` plus ``numel / group`` raw scales of ``scale_dtype`` at ``scale_off`` of
    the file; both land in the top of the region as ``int4.region_layout`` lays them out.

    A bitsandbytes 4-bit tensor (``quant`` set: :mod:`..nf4`) is ``numel / 2`` packed bytes at
    ``file_off`` plus ``numel / group`` raw absmax entries (``group`` is the block size; 1 or 4 bytes
    each) at ``scale_off`` of the file, landing as ``nf4.region_layout`` lays them out; ``quant``
    holds the checked quant state with the small tables (read at plan time)."""
    hf_name: str
    file_off: int
    img_off: int
    numel: int
    src_dtype: torch.dtype
    scale_kind: int = -1
    cols: int = 0
    scale: Optional[torch.Tensor] = field(default=None, compare=False, repr=False)
    group: int = 0
    scale_off: int = 0
    scale_dtype: Optional[torch.dtype] = None
    quant: Optional[nf4.QuantState] = field(default=None, compare=False, repr=False)

    @property
    def src_es(self) -> int:
        return _SRC_ES[self.src_dtype]

    @property
    def is_int4(self) -> bool:
        return self.group > 0 and self.quant is None

    @property
    def is_nf4(self) -> bool:
        return self.quant is not None

    @property
    def lands_segmented(self) -> bool:
        """A 4-bit tensor (INT4 or NF4): it lands segment by segment and loads whole."""
        return self.group > 0

    @property
    def scale_es(self) -> int:
        return self.quant.absmax_es if self.is_nf4 else _SRC_ES[self.scale_dtype]

    @property
    def file_nbytes(self) -> int:
        """Tensor bytes of the file that a pass reads and copies for this tensor."""
        if self.lands_segmented:
            return self.numel // 2 + self.numel // self.group * self.scale_es
        return self.numel * self.src_es

    def nf4_pieces(self) -> List[Tuple[int, int, int]]:
        """(file_off, bytes, region offset) of an NF4 tensor's landing pieces: per segment its packed
        bytes and, where it holds any, the raw absmax bytes of the blocks that end in it."""
        out = []
        for s in nf4.region_layout(self.numel, self.group, self.scale_es):
            if s.n_groups:
                out.append((self.scale_off + s.first_group * self.scale_es, s.n_groups * self.scale_es, s.scale_off))
            out.append((self.file_off + s.a // 2, (s.b - s.a) // 2, s.packed_off))
        return out

    def landing_pieces(self) -> List[Tuple[int, int, int]]:
        return self.nf4_pieces() if self.is_nf4 else self.int4_pieces()

    def landing_span(self) -> Tuple[int, int]:
        """``(offset, bytes)`` of the part of a 4-bit tensor's region that its landed inputs occupy."""
        return (nf4 if self.is_nf4 else int4).landing_span(self.numel, self.group, self.scale_es)

    def int4_pieces(self) -> List[Tuple[int, int, int]]:
        """(file_off, bytes, region offset) of an INT4 tensor's landing pieces: per segment its
        nibbles and, where it holds any, its scales."""
        out = []
        for s in int4.region_layout(self.numel, self.group, self.scale_es):
            if s.n_groups:
                out.append((self.scale_off + s.first_group * self.scale_es, s.n_groups * self.scale_es, s.scale_off))
            out.append((self.file_off + s.a // 2, (s.b - s.a) // 2, s.packed_off))
        return out

    @property
    def is_fp8(self) -> bool:
        return self.src_dtype == fp8.FP8_DTYPE

    @property
    def land_off(self) -> int:
        """Image offset where the tensor's file bytes land."""
        return self.img_off + (self.numel if self.is_fp8 else 0)


class LayerPlan:
    """Byte-level plan of one layer file -> packed fp16 image."""

    def __init__(self, cfg: ModelConfig, layer_name: str, path: str):
        self.name, self.path = layer_name, path
        infos = hostmem.read_header_native(path)
        if infos is None:
            infos, _ = read_header(path)
        infos = _relabel_layer(infos, layer_name)
        check_layer_tensors(cfg, layer_name, infos)
        runs = []
        for pl in placements(cfg, layer_name):
            key = source_key(cfg, layer_name, pl.hf_name, infos)
            if key != pl.hf_name and key == int4.packed_name(pl.hf_name):
                runs.append(self._int4_run(path, pl, infos))
                continue
            ti: TensorInfo = infos[key]
            if key == pl.hf_name and nf4.is_nf4_source(key, infos):
                runs.append(self._nf4_run(path, pl, infos))
                continue
            if ti.dtype == torch.int8:
                raise AssertionError("int8 not supported (need to add fp16_statistics)")   # utils.py:129
            if ti.dtype not in _SRC_ES:
                raise TypeError(f"{path}: {key} has dtype {ti.dtype}; fp16 / bf16 / fp32 and FP8 (e4m3fn, "
                                "with a scale tensor) supported")
            if tuple(ti.shape) != pl.shape:
                raise ValueError(f"{path}: {key} has shape {tuple(ti.shape)}, config expects {pl.shape}")
            if ti.nbytes != pl.numel * _SRC_ES[ti.dtype]:
                raise ValueError(f"{path}: {key} byte size {ti.nbytes} does not match its shape")
            if ti.dtype == fp8.FP8_DTYPE:
                runs.append(self._fp8_run(path, key, ti, pl, infos))
            else:
                runs.append(TensorRun(key, ti.begin, pl.offset, pl.numel, ti.dtype))
        self.runs = sorted(runs, key=lambda r: r.file_off)
        self.nbytes = layer_layout(cfg, layer_kind(layer_name)).nbytes
        # bytes of the file's tensors that a pass reads and copies (FP8 tensors: 1 per weight; INT4
        # tensors: half a byte per weight plus the scales)
        self.file_bytes = sum(r.file_nbytes for r in self.runs)
        self.fp8_tensors = sum(1 for r in self.runs if r.is_fp8)
        self.int4_tensors = sum(1 for r in self.runs if r.is_int4)
        self.nf4_tensors = sum(1 for r in self.runs if r.is_nf4)
        self.ignored_scales = sorted(k for k in infos if k.endswith(".input_scale"))

    @staticmethod
    def _fp8_run(path: str, key: str, ti: TensorInfo, pl, infos: Dict[str, TensorInfo]) -> TensorRun:
        """The run of FP8 tensor ``key``: its scale tensor is read now and kept as fp32 on the host."""
        where = f"{path}: "
        if len(pl.shape) != 2:
            raise TypeError(f"{where}{key} has dtype F8_E4M3; only 2-D projection weights may be FP8")
        sk = fp8.find_scale(key, infos, where)
        si = infos[sk]
        kind = fp8.check_scale(key, sk, tuple(si.shape), pl.shape, where)
        if si.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise TypeError(f"{where}{sk} has dtype {si.dtype}; FP8 scales are fp32 / fp16 / bf16")
        raw = torch.empty(si.nbytes, dtype=torch.uint8)
        hostmem.pread_into(path, si.begin, si.nbytes, raw)
        scale = raw.view(si.dtype).to(torch.float32).reshape(-1).contiguous()
        return TensorRun(key, ti.begin, pl.offset, pl.numel, ti.dtype, kind, pl.shape[1], scale)

    @staticmethod
    def _int4_run(path: str, pl, infos: Dict[str, TensorInfo]) -> TensorRun:
        """The run of the INT4 tensor that feeds placement ``pl``.  Only ``X.weight_shape`` (16 bytes)
        is read now; the scales are read with the weights, every pass."""
        where = f"{path}: "
        pk, sk, hk, g = int4.check_entry(pl.hf_name, infos, pl.shape, where)
        raw = torch.empty(16, dtype=torch.uint8)
        hostmem.pread_into(path, infos[hk].begin, 16, raw)
        int4.check_shape_values(pl.hf_name, raw.view(torch.int64).tolist(), pl.shape, where)
        ti, si = infos[pk], infos[sk]
        if ti.nbytes != pl.numel // 2 or si.nbytes != pl.numel // g * _SRC_ES[si.dtype]:
            raise ValueError(f"{path}: {pk} / {sk} byte sizes do not match their shapes")
        return TensorRun(pl.hf_name, ti.begin, pl.offset, pl.numel, ti.dtype, group=g, scale_off=si.begin,
                         scale_dtype=si.dtype)

    @staticmethod
    def _nf4_run(path: str, pl, infos: Dict[str, TensorInfo]) -> TensorRun:
        """The run of the bitsandbytes 4-bit tensor that feeds placement ``pl``.  The quant state and
        the small tables (code books, nested absmax) are read now; the absmax bytes are read with the
        weights, every pass."""
        where = f"{path}: "

        def read(name: str) -> torch.Tensor:
            ti = infos[name]
            raw = torch.empty(ti.nbytes, dtype=torch.uint8)
            hostmem.pread_into(path, ti.begin, ti.nbytes, raw)
            return raw.view(ti.dtype)

        qs = nf4.check_entry(pl.hf_name, infos, pl.shape, read, where)
        ti, ai = infos[pl.hf_name], infos[qs.absmax_name]
        if ti.nbytes != pl.numel // 2 or ai.nbytes != pl.numel // qs.block * qs.absmax_es:
            raise ValueError(f"{path}: {pl.hf_name} / {qs.absmax_name} byte sizes do not match their shapes")
        return TensorRun(pl.hf_name, ti.begin, pl.offset, pl.numel, ti.dtype, group=qs.block, scale_off=ai.begin,
                         scale_dtype=_ABSMAX_DTYPE[qs.absmax_kind], quant=qs)

    def pieces(self, lo: int = 0, hi: Optional[int] = None) -> List[Tuple[int, int, int, int]]:
        """(file_off, file_bytes, dst_off, kind) covering image bytes [lo, hi); dst_off relative to lo.
        lo / hi must be even (whole fp16 elements)."""
        hi = self.nbytes if hi is None else hi
        if lo % 2 or hi % 2:
            raise ValueError("image ranges must cover whole fp16 elements")
        out = []
        for r in self.runs:
            a, b = max(lo, r.img_off), min(hi, r.img_off + 2 * r.numel)
            if a >= b:
                continue
            if r.lands_segmented:
                if (a, b) != (r.img_off, r.img_off + 2 * r.numel):
                    fmt = "NF4" if r.is_nf4 else "INT4"
                    raise ValueError(f"{self.path}: image range [{lo}, {hi}) cuts through the {fmt} tensor "
                                     f"{r.hf_name} (an {fmt} tensor loads whole)")
                out += [(fo, nb, r.img_off + do - lo, KIND_RAW) for fo, nb, do in r.landing_pieces()]
                continue
            if r.is_fp8:
                if (a, b) != (r.img_off, r.img_off + 2 * r.numel):
                    raise ValueError(f"{self.path}: image range [{lo}, {hi}) cuts through the FP8 tensor "
                                     f"{r.hf_name} (an FP8 tensor loads whole)")
                out.append((r.file_off, r.numel, r.land_off - lo, KIND_RAW))
                continue
            e0, e1 = (a - r.img_off) // 2, (b - r.img_off) // 2
            out.append((r.file_off + e0 * r.src_es, (e1 - e0) * r.src_es, a - lo,
                        KIND_F32 if r.src_dtype == torch.float32 else KIND_RAW))
        if self.int4_tensors or self.nf4_tensors:
            out.sort(key=lambda p: p[0])      # (the streamer reads pieces in file order)
        return out

    def bf16_runs(self, lo: int = 0, hi: Optional[int] = None) -> List[Tuple[int, int]]:
        """(image offset, bytes) of bf16 tensors within [lo, hi) (offsets relative to lo): these
        are converted to fp16 in place after landing."""
        hi = self.nbytes if hi is None else hi
        out = []
        for r in self.runs:
            if r.src_dtype != torch.bfloat16:
                continue
            a, b = max(lo, r.img_off), min(hi, r.img_off + 2 * r.numel)
            if a < b:
                out.append((a - lo, b - a))
        return out

    def fp8_runs(self, lo: int = 0, hi: Optional[int] = None) -> List[Tuple[int, TensorRun]]:
        """(region offset relative to lo, run) of the FP8 tensors within [lo, hi): expanded to fp16 in
        place after landing."""
        hi = self.nbytes if hi is None else hi
        return [(r.img_off - lo, r) for r in self.runs
                if r.is_fp8 and r.img_off >= lo and r.img_off + 2 * r.numel <= hi]


    def int4_runs(self, lo: int = 0, hi: Optional[int] = None) -> List[Tuple[int, TensorRun]]:
        """(region offset relative to lo, run) of the INT4 tensors within [lo, hi)."""
        hi = self.nbytes if hi is None else hi
        return [(r.img_off - lo, r) for r in self.runs
                if r.is_int4 and r.img_off >= lo and r.img_off + 2 * r.numel <= hi]

    def nf4_runs(self, lo: int = 0, hi: Optional[int] = None) -> List[Tuple[int, TensorRun]]:
        """(region offset relative to lo, run) of the NF4 tensors within [lo, hi)."""
        hi = self.nbytes if hi is None else hi
        return [(r.img_off - lo, r) for r in self.runs
                if r.is_nf4 and r.img_off >= lo and r.img_off + 2 * r.numel <= hi]


def _relabel_layer(infos: Dict[str, TensorInfo], layer_name: str) -> Dict[str, TensorInfo]:
    """A decoder-layer file whose tensors all carry another layer index (a copied / hard-linked
    layer file, e.g. ``prepare_weights.py --synthetic --unique_layers K``) is read as this layer:
    tensors are identified by their name inside the layer."""
    if not layer_name.startswith("model.layers.") or any(k.startswith(layer_name + ".") for k in infos):
        return infos
    prefixes = {".".join(k.split(".")[:3]) for k in infos if k.startswith("model.layers.")}
    if len(prefixes) != 1:
        return infos
    (p,) = prefixes
    return {(layer_name + k[len(p):]) if k.startswith(p + ".") else k: v for k, v in infos.items()}


def _piece_array(pieces) -> ctypes.Array:
    arr = (_native.Piece * max(1, len(pieces)))()
    for i, (fo, nb, do, kind) in enumerate(pieces):
        arr[i].file_off, arr[i].nbytes, arr[i].dst_off, arr[i].kind = fo, nb, do, kind
    return arr


class FileLayerSource(LayerSource):
    """Per-layer safetensors files streamed to HBM on every pass (``--weight_cache stream``).

    ``chunk_mb`` x ``n_chunks`` is the whole pinned host footprint of the weight path.
    ``direct`` reads with ``O_DIRECT`` (bypassing the page cache; falls back to buffered
    reads where the file system refuses it).
    """

    def __init__(self, cfg: ModelConfig, model_path: str, names: Optional[Sequence[str]] = None,
                 dtype=torch.float16, chunk_mb: Optional[int] = None, n_chunks: Optional[int] = None,
                 io_threads: Optional[int] = None, direct: Optional[bool] = None):
        if dtype != torch.float16:
            raise ValueError("the packed weight image is fp16")
        self.cfg, self.model_path, self.dtype = cfg, model_path, dtype
        self.names = list(names) if names is not None else cfg.layer_names()
        missing = [n for n in self.names if not os.path.exists(layer_file(model_path, n))]
        if missing:
            raise FileNotFoundError(f"{model_path}: missing layer files {missing[:4]}...")
        self.chunk_bytes = (chunk_mb or knobs.get_int("FLS_STREAM_CHUNK_MB")) << 20
        self.n_chunks = n_chunks or knobs.get_int("FLS_STREAM_CHUNKS")
        self.io_threads = io_threads or knobs.get_int("FLS_IO_THREADS")
        self.direct = bool(knobs.get_int("FLS_O_DIRECT")) if direct is None else bool(direct)
        self._plans: Dict[str, LayerPlan] = {}
        self._lock = threading.Lock()
        self._streamer = None
        self._streamer_dev = None
        self._scale_arena: Optional[torch.Tensor] = None     # FP8 scales on the device (prepare_device)
        self._scales: Optional[Dict[Tuple[str, str], torch.Tensor]] = None
        self._scales_dev = None
        self._nf4_tables: Dict[Tuple[str, str], Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]] = {}
        self.read_seconds = 0.0
        self.read_bytes = 0

    # ---------------------------------------------------------------- plans
    def plan(self, name: str) -> LayerPlan:
        with self._lock:
            p = self._plans.get(name)
            if p is None:
                p = self._plans[name] = LayerPlan(self.cfg, name, layer_file(self.model_path, name))
            return p

    # ------------------------------------------------------------ host path
    def read_into(self, name: str, dst: torch.Tensor) -> None:
        """The whole packed image into a CPU byte buffer (host cache build, CPU runs)."""
        self.read_range_into(name, dst, 0, self.nbytes(name))

    def read_range_into(self, name: str, dst: torch.Tensor, lo: int, hi: int) -> None:
        """Image bytes [lo, hi) into ``dst[:hi - lo]`` (CPU); bf16 converted on the host."""
        t0 = time.perf_counter()
        pl = self.plan(name)
        pieces = pl.pieces(lo, hi)
        b = dst.view(torch.uint8)
        rt = _native.runtime_or_none()
        if rt is not None and pieces:
            arr = _piece_array(pieces)
            r = rt.fls_stream_read_host(pl.path.encode(), ctypes.addressof(arr), len(pieces), b.data_ptr(),
                                        self.io_threads)
            if r < 0:
                raise IOError(f"{pl.path}: read failed ({r})")
        else:
            self._read_pieces_py(pl.path, pieces, b)
        for off, nb in pl.bf16_runs(lo, hi):
            v = b[off:off + nb]
            v.view(torch.float16).copy_(v.view(torch.bfloat16).clone())
        for off, r in pl.fp8_runs(lo, hi):
            # FP8 bytes landed in the upper half of the tensor's region: the host definition
            from ..ops import get_ops
            get_ops(torch.device("cpu")).dequant_fp8(b[off:off + 2 * r.numel], r.numel, r.scale, r.scale_kind, r.cols)
        for off, r in pl.int4_runs(lo, hi):
            from ..ops import get_ops
            get_ops(torch.device("cpu")).dequant_int4(b[off:off + 2 * r.numel], r.numel, r.group, r.scale_dtype)
        for off, r in pl.nf4_runs(lo, hi):
            from ..ops import get_ops
            q = r.quant
            get_ops(torch.device("cpu")).dequant_nf4(b[off:off + 2 * r.numel], r.numel, q.block, q.absmax_kind, q.code,
                                                     q.code2, q.nested_absmax, q.nested_block, q.offset)
        self.read_bytes += sum(p[1] for p in pieces)
        self.read_seconds += time.perf_counter() - t0

    @staticmethod
    def _read_pieces_py(path: str, pieces, b: torch.Tensor) -> None:
        with open(path, "rb") as f:
            for fo, nb, do, kind in pieces:
                f.seek(fo)
                raw = f.read(nb)
                if len(raw) != nb:
                    raise IOError(f"{path}: short read")
                t = torch.frombuffer(bytearray(raw), dtype=torch.uint8)
                if kind == KIND_F32:
                    t = t.view(torch.float32).to(torch.float16).view(torch.uint8)
                b[do:do + t.numel()].copy_(t)

    # ------------------------------------------------------------- GPU path
    def _get_streamer(self, device: torch.device):
        if self._streamer is None:
            rt = _native.runtime()
            h = rt.fls_streamer_create(device.index or 0, self.chunk_bytes, self.n_chunks, self.io_threads,
                                       int(self.direct))
            if not h:
                raise RuntimeError("fls_streamer_create failed (pinned chunk ring)")
            self._streamer, self._streamer_dev = h, device
        elif self._streamer_dev != device:
            raise RuntimeError("one streaming source serves one device")
        return self._streamer

    def pinned_bytes(self) -> int:
        if self._streamer is None:
            return self.chunk_bytes * self.n_chunks
        return int(_native.runtime().fls_streamer_pinned_bytes(self._streamer))

    def stream_into(self, name: str, dst: torch.Tensor, stream, lo: int = 0, hi: Optional[int] = None,
                    cast: bool = True) -> int:
        """Enqueue image bytes [lo, hi) of ``name`` into the HBM byte tensor ``dst`` on ``stream``
        (a ``torch.cuda.Stream``).  Returns once every DMA is enqueued; the caller records its
        completion event.  ``cast`` also enqueues the in-place bf16 -> fp16 conversions (the
        data-parallel path casts after its all-gather instead).  Returns file bytes read."""
        pl = self.plan(name)
        hi = pl.nbytes if hi is None else hi
        pieces = pl.pieces(lo, hi)
        if not pieces:
            return 0
        h = self._get_streamer(dst.device)
        arr = _piece_array(pieces)
        t0 = time.perf_counter()
        r = _native.runtime().fls_streamer_load(h, pl.path.encode(), ctypes.addressof(arr), len(pieces),
                                                dst.data_ptr(), stream.cuda_stream)
        if r < 0:
            raise IOError(f"{pl.path}: streaming failed ({r})")
        self.read_seconds += time.perf_counter() - t0
        # tensor bytes, as on the host path (the streamer also reads through the small gaps between
        # two pieces of a file, such as an FP8 checkpoint's scale tensors: its own count is `r`)
        self.read_bytes += sum(p[1] for p in pieces)
        if cast:
            self.cast_on_gpu(name, dst, lo, hi)
        return int(r)

    def cast_on_gpu(self, name: str, dst: torch.Tensor, lo: int = 0, hi: Optional[int] = None) -> None:
        """In-place bf16 -> fp16 of the bf16 tensors in image bytes [lo, hi) of ``dst``, whose byte 0
        is image byte ``lo`` (current stream)."""
        pl = self.plan(name)
        runs, f8, i4, n4 = pl.bf16_runs(lo, hi), pl.fp8_runs(lo, hi), pl.int4_runs(lo, hi), pl.nf4_runs(lo, hi)
        if not runs and not f8 and not i4 and not n4:
            return
        from ..ops import get_ops
        ops = get_ops(dst.device)
        for off, r in i4:
            # INT4 tensors: expanded to fp16 in place in their own regions; the scales landed with them
            ops.dequant_int4(dst[off:off + 2 * r.numel], r.numel, r.group, r.scale_dtype)
        if n4:
            # NF4 tensors: expanded the same way; the absmax bytes landed with them, the small tables
            # are resident in the table arena
            self.prepare_device(dst.device)
            for off, r in n4:
                q = r.quant
                code, code2, nested = self._nf4_tables[(name, r.hf_name)]
                ops.dequant_nf4(dst[off:off + 2 * r.numel], r.numel, q.block, q.absmax_kind, code, code2, nested,
                                q.nested_block, q.offset)
        for off, nb in runs:
            v = dst[off:off + nb]
            ops.cast_f16(v, v, 1)
        if f8:
            # FP8 tensors: expanded to fp16 in place in their own regions (csrc/kernels/dequant.hip)
            scales = self.prepare_device(dst.device)
            for off, r in f8:
                ops.dequant_fp8(dst[off:off + 2 * r.numel], r.numel, scales[(name, r.hf_name)], r.scale_kind, r.cols)

    # ------------------------------------------------------------ FP8 scales
    def prepare_device(self, device) -> Dict[Tuple[str, str], torch.Tensor]:
        """The device-resident scale arena: the fp32 scales of every FP8 tensor of this source's
        layers, and the small tables of every NF4 tensor (code book, ``code2``, nested absmax;
        identical code books stored once), in ONE allocation, filled when the source first sees the
        device (the runner calls this before it plans its VRAM, so a cap sees the arena in the
        measured context).  Returns {(layer, tensor name): fp32 view} of the FP8 scales; the NF4
        tables are ``_nf4_tables[(layer, tensor name)] = (code, code2, nested_absmax)``."""
        device = torch.device(device)
        with self._lock:
            if self._scales is not None and self._scales_dev == device:
                return self._scales
        if self._scales is not None and self._scales_dev != device:
            raise RuntimeError("one streaming source serves one device")
        parts, index, off = [], {}, 0
        nf4_index, books = {}, {}

        def add(t: torch.Tensor) -> Tuple[int, int]:
            nonlocal off
            cnt, at = t.numel(), off
            parts.append(t)
            pad = -cnt % 4                         # every vector 16-byte aligned
            if pad:
                parts.append(torch.zeros(pad, dtype=torch.float32))
            off += cnt + pad
            return at, cnt

        def book(t: torch.Tensor) -> Tuple[int, int]:
            key = t.numpy().tobytes()              # (16 or 256 floats: identical code books once)
            if key not in books:
                books[key] = add(t)
            return books[key]

        for n in self.names:
            for r in self.plan(n).runs:
                if r.is_fp8:
                    index[(n, r.hf_name)] = add(r.scale)
                elif r.is_nf4:
                    q = r.quant
                    u8 = q.absmax_kind == nf4.ABSMAX_U8
                    nf4_index[(n, r.hf_name)] = (book(q.code), book(q.code2) if u8 else None,
                                                 add(q.nested_absmax) if u8 else None)
        views: Dict[Tuple[str, str], torch.Tensor] = {}
        arena = None
        if parts:
            host = torch.cat(parts)
            if device.type == "cuda":
                arena = hostmem.alloc_device(host.numel() * 4, device).view(torch.float32)
                arena.copy_(host)
                torch.cuda.current_stream(device).synchronize()
            else:
                arena = host
            views = {k: arena[o:o + c] for k, (o, c) in index.items()}
        tables = {k: tuple(None if oc is None else arena[oc[0]:oc[0] + oc[1]] for oc in v) for k, v in nf4_index.items()}
        with self._lock:
            self._scale_arena, self._scales, self._scales_dev = arena, views, device
            self._nf4_tables = tables
        return views

    def scale_arena_bytes(self) -> int:
        return 0 if self._scale_arena is None else self._scale_arena.numel() * 4

    def fp8_tensors(self) -> int:
        """FP8 tensors among this source's layers (0: a pure fp16 / bf16 / fp32 checkpoint)."""
        return sum(self.plan(n).fp8_tensors for n in self.names)

    def int4_tensors(self) -> int:
        """INT4 tensors among this source's layers."""
        return sum(self.plan(n).int4_tensors for n in self.names)

    def nf4_tensors(self) -> int:
        """bitsandbytes 4-bit tensors among this source's layers."""
        return sum(self.plan(n).nf4_tensors for n in self.names)

    def file_bytes(self, names: Optional[Sequence[str]] = None) -> int:
        """Tensor bytes of the layer files (what a pass reads and copies)."""
        return sum(self.plan(n).file_bytes for n in (self.names if names is None else names))

    def ignored_scales(self) -> List[str]:
        return [k for n in self.names for k in self.plan(n).ignored_scales]

    def stats(self) -> Dict[str, float]:
        out = {"read_s": self.read_seconds, "read_bytes": float(self.read_bytes)}
        if self._streamer is not None:
            rs, ws = ctypes.c_double(), ctypes.c_double()
            rb, hb = ctypes.c_uint64(), ctypes.c_uint64()
            fb = ctypes.c_int()
            _native.runtime().fls_streamer_stats(self._streamer, ctypes.byref(rs), ctypes.byref(ws),
                                                 ctypes.byref(rb), ctypes.byref(hb), ctypes.byref(fb))
            out.update({"pread_s": rs.value, "ring_wait_s": ws.value, "h2d_bytes": float(hb.value),
                        "direct_fallbacks": float(fb.value)})
        return out

    def close(self) -> None:
        if self._streamer is not None:
            _native.runtime().fls_streamer_destroy(self._streamer)
            self._streamer = None
        self._scale_arena = self._scales = self._scales_dev = None
        self._nf4_tables = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def host_ram_available() -> int:
    """MemAvailable from /proc/meminfo (bytes), 0 if unknown."""
    try:
        with open("/proc/meminfo") as f:
            for line in f:
                if line.startswith("MemAvailable:"):
                    return int(line.split()[1]) * 1024
    except OSError:
        pass
    return 0
