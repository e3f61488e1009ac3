"""Weight sources: where packed layer bytes come from before they reach HBM.

Reference behaviour (``/root/reference/utils.py:121-131``, DP cache
``utils.py:24-75``): every time a layer is needed its safetensors file is read
whole from disk, deserialized to CPU tensors and copied parameter by parameter
(pageable, synchronous) to the GPU; the whole thing repeats for every batch,
generation step and GPU.

Here a source yields the *packed* layer image (see :mod:`..models.layout`):

* :class:`~.stream.FileLayerSource` — per-layer safetensors files streamed
  every pass (file byte ranges -> pinned chunk ring -> HBM DMA, no CPU work);
  the reference's small-RAM mode (``--weight_cache stream``).
* :class:`HostStore` — every packed layer resident in pinned host memory
  (read once), so each shard H2D is one DMA at PCIe line rate
  (``--weight_cache host``).  Also built directly from synthetic random-init
  weights (generated on the GPU and copied down) for the 70B benchmark.
* :class:`CompactHostStore` — a quantised checkpoint's file bytes resident in
  pinned host memory as they are in the files (FP8: half the RAM and PCIe bytes
  of the fp16 image; INT4, NF4 and MXFP4: about a quarter), copied tensor by tensor to
  their landing positions and expanded to fp16 in the HBM slot as the file
  source does (:mod:`.stream` describes where each format lands).
* data-parallel scatter-load (:func:`piece_slices`): a rank keeps only its
  1/G byte-slice of every layer piece; the layer (or one piece of it) is
  re-assembled in HBM with an RCCL all-gather over xGMI
  (:mod:`..parallel.data_parallel`).
"""
from __future__ import annotations

import ctypes
import threading
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from .. import _native
from ..config import ModelConfig
from ..models.layout import LayerLayout, layer_kind, layer_layout
from . import hostmem


class LayerSource:
    cfg: ModelConfig
    dtype: torch.dtype = torch.float16

    def layout(self, name: str) -> LayerLayout:
        return layer_layout(self.cfg, layer_kind(name), torch.empty((), dtype=self.dtype).element_size())

    def nbytes(self, name: str) -> int:
        return self.layout(name).nbytes

    def host_buffer(self, name: str) -> Optional[torch.Tensor]:
        """Pinned uint8 buffer holding the packed layer, if resident on the host."""
        return None

    def read_into(self, name: str, dst: torch.Tensor) -> None:
        raise NotImplementedError


class HostStore(LayerSource):
    """All packed layers resident in (pinned) host memory.

    ``norms_folded``: every decoder layer's RMSNorm weights are already folded into the
    projections that consume the normalised rows (:meth:`fold_norms`, done once on the GPU), so
    the fused-norm engine streams them as they are — no per-load fold on the copy stream."""

    norms_folded = False
    # identity of the LoRA adapter merged into the buffers (lora.LoraAdapter.identity), or None;
    # lora_at_build: the store holds whole fp16 layers, so an adapter is merged once (merge_lora)
    lora_merged = None
    lora_at_build = True
    model_path = None           # the directory the layers were read from (from_source), if any
    synthetic_seed = None       # the seed of generated weights (synthetic), if any
    _pinning_full = False       # hipHostMalloc refused a layer: the rest of the store is pageable

    def __init__(self, cfg: ModelConfig, dtype=torch.float16, pinned: bool = True,
                 names: Optional[Sequence[str]] = None):
        self.cfg, self.dtype, self.pinned = cfg, dtype, pinned
        self.names = list(names) if names is not None else cfg.layer_names()
        self.buffers: Dict[str, torch.Tensor] = {}

    def merge_lora(self, adapter, device) -> "HostStore":
        """Merge a LoRA adapter (lora.LoraAdapter) into every decoder layer it targets, on
        ``device``: each layer goes H2D, is merged, and comes back (on the CPU: in place, by the host
        definition).  Once per store and before :meth:`fold_norms` — the folded weight is
        ``(W + sBA) diag(norm)``; passes then cost nothing extra."""
        from ..ops import get_ops
        if self.lora_merged is not None:
            if self.lora_merged != adapter.identity:
                raise ValueError("the host store already holds another LoRA adapter's merged weights")
            return self
        if self.norms_folded:
            raise ValueError("the host store's norms are folded already: merge the LoRA adapter before fold_norms")
        if self.dtype != torch.float16:
            raise TypeError(f"a LoRA adapter merges into fp16 weights, the store holds {self.dtype}")
        dev = torch.device(device)
        ops = get_ops(dev)
        dec = [n for n in self.names if n in self.buffers and adapter.targets(n)]
        if dec and dev.type == "cuda":
            stage = torch.empty(max(self.nbytes(n) for n in dec), dtype=torch.uint8, device=dev)
            ab = adapter.new_staging(dev)  # (this merge's own: passes need none, nothing is left to merge)
            for n in dec:
                buf = self.buffers[n]
                full = stage[:buf.numel()]
                full.copy_(buf)
                adapter.merge_views(ops, n, self.layout(n).views(full, self.dtype), ab)
                buf.copy_(full)
            torch.cuda.synchronize(dev)
            del stage, ab
        else:
            for n in dec:
                adapter.merge_views(ops, n, self.layout(n).views(self.buffers[n], self.dtype))
        self.lora_merged = adapter.identity
        return self

    def fold_norms(self, device) -> "HostStore":
        """Fold the RMSNorm weights into the projections (models.llama.fold_layer_norms) for
        every decoder layer, on ``device``: each layer goes H2D, is folded, and comes back.  Once
        per store, in place; a full 70B store takes a few seconds at PCIe rate."""
        from ..models.llama import fold_layer_norms
        from ..ops import get_ops
        if self.norms_folded:
            return self
        dev = torch.device(device)
        ops = get_ops(dev)
        dec = [n for n in self.names if layer_kind(n) == "decoder" and n in self.buffers]
        if dec:
            stage = torch.empty(max(self.nbytes(n) for n in dec), dtype=torch.uint8, device=dev)
            for n in dec:
                buf = self.buffers[n]
                full = stage[:buf.numel()]
                full.copy_(buf)
                fold_layer_norms(ops, self.layout(n).views(full, self.dtype))
                buf.copy_(full)
            del stage
        self.norms_folded = True
        return self

    @property
    def total_bytes(self) -> int:
        return sum(b.numel() for b in self.buffers.values())

    def host_buffer(self, name: str) -> Optional[torch.Tensor]:
        return self.buffers.get(name)

    def read_into(self, name: str, dst: torch.Tensor) -> None:
        src = self.buffers[name]
        dst[:src.numel()].copy_(src)

    # pinned memory handed back when the store meets the machine's pinning limit: the engine pins
    # more after the store is built (activation pools, staging buffers, score read-back)
    PINNED_HEADROOM = 4 << 30

    def alloc(self, name: str) -> torch.Tensor:
        refused = hostmem.pinned_refusals
        buf = hostmem.alloc_host(self.nbytes(name), pinned=self.pinned and not self._pinning_full)
        self.buffers[name] = buf
        if hostmem.pinned_refusals != refused:
            # the machine pins no more: this layer is pageable, and the store asks for no pinned
            # memory again (the H2D copies of pageable layers are staged by the runtime).  The
            # last pinned layers move to pageable memory too, so what the engine pins later
            # finds PINNED_HEADROOM bytes free
            self._pinning_full = True
            freed = 0
            for n in reversed(list(self.buffers)):
                if freed >= self.PINNED_HEADROOM:
                    break
                old = self.buffers[n]
                if hostmem.is_pinned_block(old):
                    self.buffers[n] = torch.empty_like(old).copy_(old)
                    freed += old.numel()
                    del old
        return buf

    @classmethod
    def from_source(cls, src: LayerSource, pinned: bool = True, threads: int = 4,
                    names: Optional[Sequence[str]] = None) -> "HostStore":
        st = cls(src.cfg, src.dtype, pinned, names)
        st.model_path = getattr(src, "model_path", None)     # (classify.head_for: score.safetensors lies there)
        for n in st.names:
            st.alloc(n)
        errs: List[BaseException] = []
        todo = list(st.names)
        lock = threading.Lock()

        def worker():
            while True:
                with lock:
                    if not todo or errs:
                        return
                    n = todo.pop(0)
                try:
                    src.read_into(n, st.buffers[n])
                except BaseException as e:  # noqa: BLE001
                    errs.append(e)
                    return

        ts = [threading.Thread(target=worker, daemon=True) for _ in range(max(1, threads))]
        [t.start() for t in ts]
        [t.join() for t in ts]
        if errs:
            raise errs[0]
        return st

    @classmethod
    def from_model_path(cls, cfg: ModelConfig, model_path: str, dtype=torch.float16,
                        pinned: bool = True, threads: int = 4) -> "HostStore":
        from .stream import FileLayerSource
        return cls.from_source(FileLayerSource(cfg, model_path, dtype=dtype), pinned, threads)

    @classmethod
    def synthetic(cls, cfg: ModelConfig, device: torch.device, seed: int = 0, std: float = 0.02,
                  pinned: bool = True, names: Optional[Sequence[str]] = None,
                  byte_range=None, progress=None, fold_norms: bool = False) -> "HostStore":
        """Random-init packed layers generated on ``device`` and copied to pinned host memory.

        ``byte_range=(r, G)`` keeps only slice r of G equal byte slices of every
        layer (data-parallel scatter-load).  Generation is deterministic in
        (seed, layer index, byte offset) so every rank's slices tile one model.
        ``fold_norms``: the RMSNorm weights are folded into the projections on the device before
        the copy (see :meth:`fold_norms`).
        """
        from ..models.llama import fold_layer_norms
        from ..ops import get_ops
        st = cls(cfg, torch.float16, pinned, names)
        st.synthetic_seed = seed                             # (classify.head_for: the seeded score layer)
        dev = torch.device(device)
        ops = get_ops(dev)
        maxb = max((st.nbytes(n) for n in st.names), default=0)   # an MP rank may own no layers
        stage = torch.empty(maxb, dtype=torch.uint8, device=dev)
        for li, n in enumerate(st.names):
            if progress is not None and li % 10 == 0:
                progress(li, len(st.names))
            lay = st.layout(n)
            full = stage[:lay.nbytes]
            ops.fill_layer_random(full, lay, seed=seed * 7919 + cfg.layer_names().index(n), std=std)
            if fold_norms and lay.kind == "decoder":
                fold_layer_norms(ops, lay.views(full, torch.float16))
            if byte_range is None:
                buf = st.alloc(n)
                buf.copy_(full, non_blocking=False)
            else:
                r, G = byte_range
                sl = piece_slices(lay, G)
                buf = hostmem.alloc_host(sum(p.chunk for p in sl), pinned=pinned)
                for p in sl:
                    a, b = p.rank_range(r)
                    if b > a:
                        buf[p.buf_off:p.buf_off + b - a].copy_(full[a:b])
                st.buffers[n] = buf
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        del stage
        st.norms_folded = bool(fold_norms)
        return st


class CompactHostStore(LayerSource):
    """The layer files' tensor bytes resident in pinned host memory as they are in the files —
    FP8 tensors as FP8, one byte per weight (``--weight_cache host`` for an FP8 checkpoint: half the
    pinned RAM and half the PCIe bytes of the fp16 image).

    It is a streaming source for the prefetchers (``host_buffer()`` is None): ``stream_into``
    copies every tensor of the range to its landing position in the HBM slot with one async H2D
    from pinned memory, and ``cast_on_gpu`` expands the quantised tensors (and casts bf16 ones) in
    place as the file source does.  Per layer the tensors sit in file order, each at a
    ``COMPACT_ALIGN``-byte aligned offset; fp32 tensors are kept as fp16.  ``norms_folded`` stays
    False: norms cannot be folded into quantised bytes without requantising, so they are folded as
    each layer lands.

    A 4-bit tensor (``TensorRun.lands_segmented``: INT4, NF4, MXFP4) is pinned as its landing image: the
    packed bytes and raw scales of its segments in the order and at the offsets they take in the
    tensor's region (the landing layout of :mod:`..quant`), so the whole tensor is still one H2D
    (``TensorRun.landing_span``).  A GPTQ / AWQ tensor likewise: its three file tensors at the offsets
    they take at the bottom of the region (``gptq.input_layout``)."""

    norms_folded = False
    COMPACT_ALIGN = 16

    def __init__(self, files, pinned: bool = True, threads: int = 4):
        from . import stream as st
        self.files, self.cfg, self.dtype = files, files.cfg, files.dtype
        self.names, self.pinned = list(files.names), pinned
        self.buffers: Dict[str, torch.Tensor] = {}
        self._offsets: Dict[str, Dict[str, int]] = {}
        self.h2d_bytes = 0
        rt = _native.runtime_or_none()
        for n in self.names:
            pl = files.plan(n)
            offs, off, pieces = {}, 0, []
            for r in pl.runs:
                offs[r.hf_name] = off
                if r.lands_segmented:
                    base, span = r.landing_span()
                    pieces += [(fo, nb, off + do - base, st.KIND_RAW) for fo, nb, do in r.landing_pieces()]
                    off += self._aligned(span)
                    continue
                f32 = r.src_dtype == torch.float32
                pieces.append((r.file_off, r.numel * r.src_es, off, st.KIND_F32 if f32 else st.KIND_RAW))
                off += self._aligned(r.numel * (2 if f32 else r.src_es))
            buf = hostmem.alloc_host(off, pinned=pinned)
            if rt is not None and pieces:
                arr = st._piece_array(pieces)
                rc = rt.fls_stream_read_host(pl.path.encode(), ctypes.addressof(arr), len(pieces), buf.data_ptr(),
                                             max(1, threads))
                if rc < 0:
                    raise IOError(f"{pl.path}: read failed ({rc})")
            else:
                files._read_pieces_py(pl.path, pieces, buf)
            self.buffers[n], self._offsets[n] = buf, offs

    @classmethod
    def _aligned(cls, n: int) -> int:
        return (n + cls.COMPACT_ALIGN - 1) // cls.COMPACT_ALIGN * cls.COMPACT_ALIGN

    @classmethod
    def from_model_path(cls, cfg: ModelConfig, model_path: str, pinned: bool = True,
                        names: Optional[Sequence[str]] = None) -> "CompactHostStore":
        from .stream import FileLayerSource
        return cls(FileLayerSource(cfg, model_path, names=names), pinned)

    @property
    def total_bytes(self) -> int:
        return sum(b.numel() for b in self.buffers.values())

    def pinned_bytes(self) -> int:
        return self.total_bytes

    def plan(self, name: str):
        return self.files.plan(name)

    def fold_norms(self, device):
        raise ValueError("--weight_cache host keeps an FP8, INT4, NF4 or MXFP4 checkpoint's bytes as they are in the files: norms "
                         "cannot be folded into quantised weights (they are folded as each layer lands)")

    def read_into(self, name: str, dst: torch.Tensor) -> None:
        self.files.read_into(name, dst)

    def prepare_device(self, device):
        return self.files.prepare_device(device)

    def stream_into(self, name: str, dst: torch.Tensor, stream, lo: int = 0, hi: Optional[int] = None,
                    cast: bool = True) -> int:
        """Enqueue image bytes [lo, hi) of ``name`` into the HBM byte tensor ``dst`` (whose byte 0 is
        image byte ``lo``) on ``stream``: one async H2D per tensor, then (``cast``) the in-place
        expansions.  Returns the host bytes copied."""
        pl = self.files.plan(name)
        hi = pl.nbytes if hi is None else hi
        pl.pieces(lo, hi)                   # (refuses a range through a quantised tensor)
        buf, offs, total = self.buffers[name], self._offsets[name], 0
        with torch.cuda.stream(stream):
            for r in pl.runs:
                a, b = max(lo, r.img_off), min(hi, r.img_off + 2 * r.numel)
                if a >= b:
                    continue
                if r.lands_segmented:
                    base, span = r.landing_span()
                    src, d0 = buf[offs[r.hf_name]:offs[r.hf_name] + span], r.img_off + base - lo
                elif r.is_fp8:
                    src, d0 = buf[offs[r.hf_name]:offs[r.hf_name] + r.numel], r.land_off - lo
                else:
                    s0 = offs[r.hf_name] + (a - r.img_off)
                    src, d0 = buf[s0:s0 + (b - a)], a - lo
                dst[d0:d0 + src.numel()].copy_(src, non_blocking=True)
                total += src.numel()
            if cast:
                self.cast_on_gpu(name, dst, lo, hi)
        self.h2d_bytes += total
        return total

    def cast_on_gpu(self, name: str, dst: torch.Tensor, lo: int = 0, hi: Optional[int] = None) -> None:
        self.files.cast_on_gpu(name, dst, lo, hi)

    def stats(self) -> Dict[str, float]:
        return {"h2d_bytes": float(self.h2d_bytes), "pinned_bytes": float(self.total_bytes)}

    def close(self) -> None:
        self.files.close()


def shard_chunk_bytes(nbytes: int, world: int, align: int = 4096) -> int:
    c = (nbytes + world - 1) // world
    return (c + align - 1) // align * align


def layer_pieces(lay: LayerLayout) -> List[Tuple[int, int]]:
    """Byte ranges of a packed layer image that load as one unit: a decoder layer's attention
    piece and MLP piece (``models.layout.mlp_offset``; the sub-layer piece pool streams them
    separately), one range for every other kind."""
    from ..models.layout import mlp_offset
    if lay.kind == "decoder":
        s = mlp_offset(lay)
        return [(0, s), (s, lay.nbytes)]
    return [(0, lay.nbytes)]


class PieceSlice(NamedTuple):
    """Data-parallel scatter-load of one piece ``[lo, hi)`` of a layer image over G ranks: rank r
    holds bytes ``[lo + r * chunk, min(hi, lo + (r + 1) * chunk))`` at ``buf_off`` of its host
    buffer, and the all-gather rebuilds the piece in a ``chunk * G``-byte HBM region."""
    lo: int
    hi: int
    chunk: int
    buf_off: int

    def rank_range(self, r: int) -> Tuple[int, int]:
        a = self.lo + r * self.chunk
        return a, max(a, min(self.hi, a + self.chunk))


def piece_slices(lay: LayerLayout, world: int) -> List[PieceSlice]:
    """Every rank's slices of ``lay``, piece by piece (:func:`layer_pieces`): each piece is split
    on its own, so a rank's slices serve the whole-layer all-gather and the per-piece one alike."""
    out, off = [], 0
    for lo, hi in layer_pieces(lay):
        c = shard_chunk_bytes(hi - lo, world)
        out.append(PieceSlice(lo, hi, c, off))
        off += c
    return out


def piece_views(lay: LayerLayout, regions: Sequence[Tuple[int, torch.Tensor]], dtype) -> Dict[str, torch.Tensor]:
    """Typed tensor views of a layer whose pieces sit in separate byte regions: ``regions`` =
    [(image offset of the piece, uint8 region holding it)] in image order."""
    es = torch.empty((), dtype=dtype).element_size()
    out = {}
    for ts in lay.slots:
        lo, reg = [(lo, reg) for lo, reg in regions if lo <= ts.offset][-1]
        o = ts.offset - lo
        out[ts.name] = reg[o:o + ts.numel * es].view(dtype).view(ts.shape)
    return out
