"""Data parallelism with scatter-loaded, all-gathered layer weights.

Reference DP (``/root/reference/utils.py:24-75, 122-124``): one host-RAM copy
of the current layer shared by every GPU thread; each GPU then copies the
whole layer over its own PCIe link (G x the host traffic) and the GPUs move
in lock-step under a Condition/Lock pair (ABBA order).

MI355X design: each rank owns only ITS 1/G byte-slice of every packed layer
and DMAs that slice into HBM over its own PCIe link; the full layer is
re-assembled in the HBM weight slot by ``all_gather_into_tensor`` — RCCL over
the fully connected xGMI fabric (7 links per GPU) — on the copy side of the
double buffer, so shard k+1's H2D + all-gather overlap shard k's compute.
The slice comes from either

* pinned host RAM (:class:`SlicedHostStore`, ``--weight_cache host``: 138/G GB
  per rank for 70B, each rank reading only its byte ranges of the layer files
  once at start-up), or
* the layer files on every pass (:class:`~..runtime.stream.FileLayerSource`,
  ``--weight_cache stream``): each rank streams only its 1/G byte range, so
  every file is read from disk once per pass for all GPUs — the reference's
  shared host cache without the host copy.

Per layer and GPU the PCIe (and disk) traffic drops G-fold; every rank issues
the same collectives in the same order (no P2P ordering hazards, no polling),
including ranks whose prompt slice is empty.  Prompts are split with
``np.array_split`` like ``main.py:69-70``; scores are gathered to rank 0.
"""
from __future__ import annotations

import time
from typing import Dict, List, Optional, Sequence

import torch

from ..models.layout import ALIGN_BYTES
from ..runtime import hostmem
from ..runtime.prefetch import PiecePoolPrefetcher, ShardPrefetcher
from ..runtime.weights import HostStore, LayerSource, PieceSlice, piece_slices, piece_views
from .comm import Comm


def _align(n: int) -> int:
    return (n + ALIGN_BYTES - 1) // ALIGN_BYTES * ALIGN_BYTES


class SlicedHostStore(HostStore):
    """Rank ``rank``'s 1/G byte slice of every piece of every packed layer (pinned), concatenated
    per layer (:func:`~..runtime.weights.piece_slices`): the slices serve the whole-layer
    all-gather (:class:`AllGatherPrefetcher`) and the sub-layer one (:class:`AllGatherPiecePool`)."""

    def __init__(self, cfg, rank: int, world: int, dtype=torch.float16, pinned=True, names=None):
        super().__init__(cfg, dtype, pinned, names)
        self.rank, self.world = rank, world

    def slices(self, name: str) -> List[PieceSlice]:
        return piece_slices(self.layout(name), self.world)

    def chunk_bytes(self, name: str) -> int:
        """Bytes of this rank's buffer for ``name`` (its slices of every piece)."""
        return sum(p.chunk for p in self.slices(name))

    def read_into(self, name: str, dst: torch.Tensor) -> None:   # pragma: no cover - not a full source
        raise RuntimeError("a sliced store holds only 1/G of each layer")

    @classmethod
    def from_source(cls, src: LayerSource, rank: int, world: int, pinned: bool = True,
                    names: Optional[Sequence[str]] = None) -> "SlicedHostStore":
        """Read only this rank's byte slices of every layer (``read_range_into``)."""
        st = cls(src.cfg, rank, world, src.dtype, pinned, names)
        for n in st.names:
            buf = hostmem.alloc_host(st.chunk_bytes(n), pinned=pinned)
            for p in st.slices(n):
                a, b = p.rank_range(rank)
                if b > a:
                    src.read_range_into(n, buf[p.buf_off:p.buf_off + p.chunk], a, b)
            st.buffers[n] = buf
        return st

    @classmethod
    def synthetic(cls, cfg, device, rank: int, world: int, seed: int = 0, std: float = 0.02,
                  pinned: bool = True, names=None, progress=None, fold_norms: bool = False) -> "SlicedHostStore":
        base = HostStore.synthetic(cfg, device, seed=seed, std=std, pinned=pinned, names=names,
                                   byte_range=(rank, world), progress=progress, fold_norms=fold_norms)
        st = cls(cfg, rank, world, torch.float16, pinned, names)
        st.buffers = base.buffers
        st.norms_folded = base.norms_folded
        return st

    lora_at_build = False           # a slice cannot be merged alone: the gathered layer is, as it lands

    def merge_lora(self, adapter, device):   # pragma: no cover - a slice cannot be merged alone
        raise RuntimeError("a sliced store holds 1/G of each layer: the adapter is merged as each layer is gathered")

    def fold_norms(self, device):   # pragma: no cover - a slice cannot be folded alone
        raise RuntimeError("a sliced store holds 1/G of each layer: fold before slicing (synthetic(fold_norms=True))")


class AllGatherPrefetcher(ShardPrefetcher):
    """Shard prefetcher whose H2D moves only this rank's slice; the layer is
    completed in HBM with one all-gather per layer over xGMI.

    ``store`` is a :class:`SlicedHostStore` (slices pinned in host RAM) or a
    streaming :class:`~..runtime.stream.FileLayerSource` (slices read from the
    layer files every pass by a loader thread, bf16 cast after the gather).

    Every all-gather is issued by the MAIN thread, inside :meth:`prefetch` — at the same program
    point on every rank (the engine's per-shard prefetch, also on ranks without prompts) — so the
    gathers on this communicator and the main thread's collectives on the default one (score
    gather, broadcasts, the bench's all-reduces) are enqueued in one order on every rank: two
    communicators whose RCCL streams share a hardware queue (GPU_MAX_HW_QUEUES = 4 < the streams
    of a rank) then cannot wait on each other in opposite orders on two ranks.  With a streaming
    source only the file reads (and their H2D of this rank's slice, on a stream of their own) run
    in the loader thread, started as soon as the slot they land in is released."""

    collective = True      # every rank must acquire every shard (engine: empty prompt slices too)

    def __init__(self, store: LayerSource, layer_names, shards, device, comm: Comm,
                 n_slots: int = 2, resident: bool = False):
        self.comm = comm.dup()               # own communicator: gathers come from the loader thread
        self.store = store
        self.streaming = not isinstance(store, SlicedHostStore)
        super().__init__(store, layer_names, shards, device, n_slots=n_slots, resident=resident)
        if not self.streaming:
            self._pool = None                 # slices are host-resident: no loader thread
        self.bytes_read = 0                   # file bytes this rank read (streaming)
        self.read_stream = torch.cuda.Stream(self.dev) if (self.cuda and self.streaming) else None
        self._reads: Dict[int, object] = {}   # shard -> Future of its slice reads (loader thread)

    def slices(self, name: str) -> List[PieceSlice]:
        return piece_slices(self.store.layout(name), self.comm.world)

    def shard_bytes(self, k: int) -> int:
        G = self.comm.world
        return sum(_align(p.chunk * G) for i in self.shards[k] for p in self.slices(self.names[i]))

    # ------------------------------------------------------------ streaming (reads / gathers split)
    def _read(self, k: int, epoch=None):
        """Loader thread: this rank's slices of shard k from the layer files into their places in
        the slot, on the read stream behind the slot's free event -> (slot, read event, pieces)."""
        s = self.slot_of(k, epoch)
        slot = self._slot(s)
        G, r = self.comm.world, self.comm.rank
        plan = []
        with torch.cuda.stream(self.read_stream):
            if self._free_ev[s] is not None:
                self.read_stream.wait_event(self._free_ev[s])
            off = 0
            for i in self.shards[k]:
                name = self.names[i]
                for p in self.slices(name):
                    region = slot[off:off + p.chunk * G]
                    mine = region[r * p.chunk:(r + 1) * p.chunk]
                    lo, hi = p.rank_range(r)
                    if hi > lo:
                        self.bytes_read += self.store.stream_into(name, mine, self.read_stream, lo, hi, cast=False)
                    plan.append((name, p, region, mine, hi - lo))
                    off += _align(p.chunk * G)
            ev = torch.cuda.Event()
            ev.record(self.read_stream)
        return s, ev, plan

    def _gather(self, rd):
        """Main thread: the all-gathers completing shard k's pieces (copy stream, after the reads),
        the bf16 casts and the load transform -> the ready entry."""
        s, rev, plan = rd
        views: Dict[str, Dict[str, torch.Tensor]] = {}
        regions: Dict[str, list] = {}
        with torch.cuda.stream(self.copy_stream):
            self.copy_stream.wait_event(rev)
            for name, p, region, mine, nb in plan:
                self.comm.all_gather_into(region, mine, async_op=True).wait()
                self.store.cast_on_gpu(name, region, p.lo, p.hi)
                regions.setdefault(name, []).append((p.lo, region))
                self.bytes_h2d += nb
            for name, regs in regions.items():
                views[name] = piece_views(self.store.layout(name), regs, self.dtype)
                self._loaded(name, views[name])
            ev = torch.cuda.Event()
            ev.record(self.copy_stream)
        return ev, views, s

    def _submit_read(self, k: int, epoch=None) -> None:
        if k not in self._reads and k not in self._ready:
            self._reads[k] = self._pool.submit(self._read, k, epoch)

    def prefetch(self, k: int, epoch=None) -> None:
        if not (self.streaming and self.cuda):
            return super().prefetch(k, epoch)
        if k < 0 or k >= len(self.shards):
            return
        with self.lock:
            if k in self._ready or (k in self._sticky and k in self._loaded_resident):
                return
        self._submit_read(k, epoch)
        rd = self._reads.pop(k).result()      # the host waits only for reads started a shard ago
        entry = self._gather(rd)
        with self.lock:
            self._ready[k] = entry

    def release(self, k: int) -> None:
        super().release(k)
        if self.streaming and self.cuda and not self.resident and self.in_rotation(k) and k not in self._sticky:
            # the slot is free (its event recorded): start reading the next shard that lands in it
            s = self.slot_of(k)
            for j in range(k + 1, len(self.shards)):
                if self.in_rotation(j) and j not in self._sticky:
                    if self.slot_of(j) == s:
                        self._submit_read(j)
                        break

    def discard_loaded(self) -> None:
        for f in list(self._reads.values()):
            try:
                f.result()
            except Exception:  # noqa: BLE001 - the load is being dropped anyway
                pass
        self._reads.clear()
        super().discard_loaded()

    def close(self):
        self.discard_loaded()
        super().close()

    def _load(self, k: int, epoch=None):
        t0 = time.perf_counter()
        s = self.slot_of(k, epoch)
        slot = self._slot(s)
        G, r = self.comm.world, self.comm.rank
        views: Dict[str, Dict[str, torch.Tensor]] = {}
        ctx = torch.cuda.stream(self.copy_stream) if self.cuda else _nullctx()
        ev = None
        with ctx:
            if self.cuda and self._free_ev[s] is not None:
                self.copy_stream.wait_event(self._free_ev[s])
            off = 0
            for i in self.shards[k]:
                name = self.names[i]
                regions = []
                for p in self.slices(name):
                    region = slot[off:off + p.chunk * G]
                    # in-place all-gather: this rank's slice lands straight in its own place in the
                    # slot (RCCL's sendbuff == recvbuff + rank * count form): no staging buffer in HBM
                    mine = region[r * p.chunk:(r + 1) * p.chunk]
                    lo, hi = p.rank_range(r)
                    if not self.streaming:
                        mine.copy_(self.store.buffers[name][p.buf_off:p.buf_off + p.chunk], non_blocking=self.cuda)
                    elif hi > lo and self.cuda:
                        self.bytes_read += self.store.stream_into(name, mine, self.copy_stream, lo, hi, cast=False)
                    elif hi > lo:
                        before = self.store.read_bytes
                        self.store.read_range_into(name, mine, lo, hi)
                        self.bytes_read += self.store.read_bytes - before
                    w = self.comm.all_gather_into(region, mine, async_op=self.cuda)
                    if self.cuda:
                        w.wait()              # the copy stream waits for the gather, not the host
                    if self.streaming and self.cuda:
                        self.store.cast_on_gpu(name, region, p.lo, p.hi)
                    regions.append((p.lo, region))
                    off += _align(p.chunk * G)
                    self.bytes_h2d += hi - lo
                views[name] = piece_views(self.store.layout(name), regions, self.dtype)
                self._loaded(name, views[name])      # (the gathered copy in the slot: on the CPU too)
            if self.cuda:
                ev = torch.cuda.Event()
                ev.record(self.copy_stream)
        self.load_seconds += time.perf_counter() - t0
        return ev, views, s


class AllGatherPiecePool(PiecePoolPrefetcher):
    """The sub-layer piece pool (``--max_vram_gb``, :class:`~..runtime.prefetch.PiecePoolPrefetcher`:
    one attention slot + two MLP slots, pieces loaded in pass order as slots free up) for data
    parallel: each piece is scatter-loaded — this rank H2Ds its 1/G slice into its place in the
    slot — and completed by an in-place all-gather on this prefetcher's own communicator, so every
    rank runs in the single-GPU memory envelope (VERDICT r3 #2a).  Pieces are issued in the same
    (global pass) order on every rank, so the gathers line up; each slot holds a gathered piece
    (``chunk x G`` bytes >= the piece)."""

    collective = True      # every rank acquires every shard (engine: empty prompt slices too)

    def __init__(self, store: SlicedHostStore, layer_names, shards, device, comm: Comm, dtype=torch.float16):
        self.comm = comm.dup()
        self.G, self.r = comm.world, comm.rank
        super().__init__(store, layer_names, shards, device, dtype)
        # slot sizes of the gathered pieces (>= the image bytes PiecePoolPrefetcher sized them for)
        self._slice = {}
        a_max = m_max = 0
        own = list(self._own_sizes)
        for kind, k, lo, hi in self.pieces:
            name = self.names[self.shards[k][0]]
            p = next(q for q in store.slices(name) if q.lo == lo)
            self._slice[(name, lo)] = p
            g = _align(p.chunk * self.G)
            if kind == "a":
                a_max = max(a_max, g)
            elif kind == "m":
                m_max = max(m_max, g)
            else:
                own[self._own[k]] = max(own[self._own[k]], g)
        self.a_bytes, self.m_bytes = a_max, m_max
        self.slot_bytes = m_max
        self._slot_sizes = [a_max, m_max, m_max] + own

    def _copy_piece(self, slot: torch.Tensor, name: str, lo: int, hi: int) -> int:
        p = self._slice[(name, lo)]
        mine = slot[self.r * p.chunk:(self.r + 1) * p.chunk]
        mine.copy_(self.src.buffers[name][p.buf_off:p.buf_off + p.chunk], non_blocking=True)
        w = self.comm.all_gather_into(slot[:p.chunk * self.G], mine, async_op=True)
        w.wait()                   # the copy stream waits for the gather, not the host
        a, b = p.rank_range(self.r)
        return b - a


class _nullctx:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def build_dp_sharded_runner(args, cfg, device, comm: Comm, tok, store: Optional[LayerSource] = None,
                            weight_cache: str = "host", prefix_kv_cache: Optional[bool] = None, lora=None):
    """Data-parallel runner with scatter-loaded weights: ``weight_cache`` ``host`` pins this
    rank's slices (read once), ``stream`` re-reads them from the layer files every pass."""
    from ..config import MAX_TOKEN_LEN
    from ..engine import ShardedRunner
    from ..runtime.stream import FileLayerSource
    from .planner import make_plan
    device = torch.device(device)
    from ..embed import EmbedParams, layer_names as mode_layer_names
    mode = getattr(args, "score_mode", "next_token")
    names = mode_layer_names(cfg, mode)              # (embed: no lm_head, which need not exist)
    embed_kw = {}
    if mode == "embed":
        ep = EmbedParams.from_args(args)
        embed_kw = dict(embed_pooling=ep.pooling, embed_dim=ep.dim, embed_normalize=ep.normalize)
    if store is None and getattr(args, "synthetic", None):
        from .. import knobs
        store = SlicedHostStore.synthetic(cfg, device, comm.rank, comm.world, pinned=device.type == "cuda",
                                          fold_norms=device.type == "cuda" and knobs.get_int("FLS_QKV_FOLD") == 1)
    elif store is None:
        src = FileLayerSource(cfg, args.model_path, names=names, direct=getattr(args, "o_direct", False))
        store = src if weight_cache == "stream" else SlicedHostStore.from_source(
            src, comm.rank, comm.world, pinned=device.type == "cuda")
    plan = make_plan(len(names), args.layer_num_per_shard, comm.world, comm.rank, True)
    shards = [s for s in plan.my_shards if len(s)]
    # the prefetcher's gather communicator (its comm.dup()): torch.distributed, or the native RCCL one
    comm.gather_native = getattr(args, "dp_gather_comm", "torch") == "native"
    if (getattr(args, "max_vram_gb", None) and args.layer_num_per_shard == 1 and device.type == "cuda"
            and not getattr(args, "resident", False) and isinstance(store, SlicedHostStore)):
        pf = AllGatherPiecePool(store, names, shards, device, comm)   # sub-layer pieces under a cap
    else:
        pf = AllGatherPrefetcher(store, names, shards, device, comm, resident=getattr(args, "resident", False))
    act = None
    if getattr(args, "dtype", None):
        act = torch.float16 if args.dtype == "float16" else torch.float32
    return ShardedRunner(cfg, store, device, tok, layer_num_per_shard=args.layer_num_per_shard,
                         storage_location=args.storage_location, disk_folder=args.disk_folder,
                         max_activation_in_cpu=args.max_activation_in_cpu,
                         prefix_attention=args.prefix_attention, token_budget=args.token_budget,
                         resident=getattr(args, "resident", False), comm=comm, data_parallel=True,
                         act_dtype=act, prefetcher=pf, verbose=getattr(args, "verbose", False),
                         resume_dir=getattr(args, "resume_dir", None),
                         checkpoint_every=getattr(args, "checkpoint_every", 0),
                         max_token_len=getattr(args, "max_token_len", None) or MAX_TOKEN_LEN,
                         hip_graphs=getattr(args, "hip_graphs", False),
                         prefix_kv_cache=(prefix_kv_cache if prefix_kv_cache is not None
                                          else getattr(args, "prefix_kv_cache", False) is True),
                         prefix_cache_entries=getattr(args, "prefix_cache_entries", 8),
                         suffix_kv_cache=_suffix_kv(args, comm), exact_reuse=getattr(args, "exact_reuse", True),
                         sliding_window_mode=getattr(args, "sliding_window_mode", "error"),
                         score_mode=getattr(args, "score_mode", "next_token"),
                         max_vram_gb=getattr(args, "max_vram_gb", None),
                         score_top_k=int(getattr(args, "score_top_k", 0) or 0), lora=lora, **embed_kw)


def _suffix_kv(args, comm: Comm) -> bool:
    from ..api import resolve_suffix_kv_cache
    return resolve_suffix_kv_cache(args, comm.world)
