"""LoRA adapters merged into the weights as they land: the host definition.

An adapter is a directory in PEFT's saved form: ``adapter_config.json`` and
``adapter_model.safetensors`` with, per adapted module (an HF module path such as
``model.layers.3.self_attn.q_proj``),

    base_model.model.<module>.lora_A.weight   [r, in]
    base_model.model.<module>.lora_B.weight   [out, r]

in fp16, bf16 or fp32.  The rank ``r`` of a module is read from its tensors.  Its scale is
``s = fp32(lora_scale * alpha / r)`` (``alpha / sqrt(r)`` with ``use_rslora``), computed in float64
and rounded once; ``alpha`` comes from ``alpha_pattern`` where a key matches the module by the
regular expression ``(.*\\.)?(key)$``, else it is ``lora_alpha``.

The merged weight.  With ``a = fp32(A)``, ``b' = fp32(s * fp32(B))`` (one fp32 multiply, done once on
the host) and ``R`` = ``r`` rounded up to a multiple of 4 with ``+0`` padding:

    acc_0      = fp32(w16[o, i])
    acc_{k+1}  = fmaf(b'[o, k], a[k, i], acc_k)        k = 0 .. R-1, in this order, one rounding each
    w16'[o, i] = fp16_rne(acc_R)

fp32 and fp16 subnormals are kept; the padding is part of the definition (it only decides the sign
of a zero result: ``-0`` with an all-zero adapter becomes ``+0``).  :func:`merge_reference` is this
function in numpy; the HIP kernel (``csrc/kernels/lora.hip``) computes it on the f32-input MFMA, in
place in the HBM weight slot.  A run with an adapter therefore equals, bit for bit, the same run on
the merged *twin* checkpoint (:func:`write_twin`).

Targets: ``q_proj``, ``k_proj``, ``v_proj``, ``o_proj``, ``gate_proj``, ``up_proj``, ``down_proj``
and Phi-3's fused ``qkv_proj`` / ``gate_up_proj``; each is a contiguous row range of one packed view
(``models/layout.py``).  On MoE models the attention projections only.
"""
from __future__ import annotations

import glob
import hashlib
import json
import math
import os
import re
import shutil
import struct
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .config import ModelConfig
from .models.layout import layer_kind, layer_layout, placements

CONFIG_NAME = "adapter_config.json"
WEIGHTS_NAME = "adapter_model.safetensors"
PREFIX = "base_model.model."
MAX_RANK = 256
TARGETS = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj", "qkv_proj", "gate_up_proj")
_DTYPES = (torch.float16, torch.bfloat16, torch.float32)


def padded_rank(r: int) -> int:
    return (r + 3) // 4 * 4


# --------------------------------------------------------------------------- the definition
def fma32(a: np.ndarray, b: np.ndarray, c: np.ndarray) -> np.ndarray:
    """fp32 ``fmaf(a, b, c)`` element-wise (float32 arrays): the product is exact in float64, the
    sum is rounded to odd in float64 (TwoSum gives the error's sign), and one rounding to fp32
    follows — 53 >= 24 + 2 bits, so the result is the correctly rounded fp32 fma."""
    a64, b64, c64 = a.astype(np.float64), b.astype(np.float64), c.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        p = a64 * b64
        t = p + c64
        bb = t - p
        e = (p - (t - bb)) + (c64 - bb)
        fix = np.isfinite(t) & (e != 0) & ((t.view(np.int64) & 1) == 0)
        if fix.any():
            t = np.where(fix, np.nextafter(t, np.where(e > 0, np.inf, -np.inf)), t)
        return t.astype(np.float32)


def merge_reference(w16, A, B, s) -> np.ndarray:
    """``w16'`` (numpy float16 ``[out, in]``) of the definition above for ``w16`` (fp16 ``[out, in]``),
    ``A`` (``[r, in]``), ``B`` (``[out, r]``; both fp16 / bf16 / fp32, torch or numpy) and the scale
    ``s``.  Pass ``s=None`` with a ``B`` that is already ``b'`` (fp32, scale folded in)."""
    w = _np16(w16)
    a = _np32(A)
    b = _np32(B)
    if s is not None:
        with np.errstate(over="ignore"):
            b = (b * np.float32(s)).astype(np.float32)
    if w.ndim != 2 or a.ndim != 2 or b.ndim != 2 or a.shape[1] != w.shape[1] or b.shape[0] != w.shape[0] \
            or a.shape[0] != b.shape[1]:
        raise ValueError(f"merge shapes: w {w.shape}, A {a.shape}, B {b.shape}")
    acc = w.astype(np.float32)
    r = a.shape[0]
    for k in range(padded_rank(r)):
        if k < r:
            acc = fma32(np.broadcast_to(b[:, k:k + 1], acc.shape), np.broadcast_to(a[k:k + 1, :], acc.shape), acc)
        else:
            acc = fma32(np.zeros_like(acc), np.zeros_like(acc), acc)
    with np.errstate(over="ignore"):
        return acc.astype(np.float16)


def _np16(w) -> np.ndarray:
    if isinstance(w, torch.Tensor):
        if w.dtype != torch.float16:
            raise TypeError(f"the merged weight is fp16, got {w.dtype}")
        return w.detach().cpu().contiguous().numpy()
    w = np.asarray(w)
    if w.dtype != np.float16:
        raise TypeError(f"the merged weight is fp16, got {w.dtype}")
    return w


def _np32(t) -> np.ndarray:
    if isinstance(t, torch.Tensor):
        if t.dtype not in _DTYPES:
            raise TypeError(f"adapter tensors are fp16 / bf16 / fp32, got {t.dtype}")
        return t.detach().cpu().to(torch.float32).contiguous().numpy()
    t = np.asarray(t)
    if t.dtype not in (np.float16, np.float32):
        raise TypeError(f"adapter tensors are fp16 / bf16 / fp32, got {t.dtype}")
    return t.astype(np.float32)


def check_merge_args(w: torch.Tensor, a: torch.Tensor, bs: torch.Tensor, r: int) -> None:
    """The argument contract of ``ops.lora_merge`` (both backends)."""
    if not 1 <= int(r) <= MAX_RANK:
        raise ValueError(f"lora_merge: r={r} is outside 1..{MAX_RANK}")
    R = padded_rank(int(r))
    if w.dtype != torch.float16 or w.dim() != 2 or not w.is_contiguous() or w.numel() == 0:
        raise TypeError(f"lora_merge: w is a contiguous fp16 [rows, cols] tensor, got {w.dtype} {tuple(w.shape)}")
    for t, shape, what in ((a, (R, w.shape[1]), "a"), (bs, (w.shape[0], R), "bs")):
        if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"lora_merge: {what} is a contiguous fp32 {list(shape)} tensor (padded to R = {R}), "
                             f"got {t.dtype} {tuple(t.shape)}")


def scale_of(alpha: float, r: int, lora_scale: float = 1.0, rslora: bool = False) -> np.float32:
    """``fp32(lora_scale * alpha / r)`` (``/ sqrt(r)`` with rsLoRA): float64, rounded once."""
    d = math.sqrt(float(r)) if rslora else float(r)
    return np.float32(np.float64(lora_scale) * np.float64(alpha) / np.float64(d))


# --------------------------------------------------------------------------- the adapter
@dataclass
class Target:
    """One adapted module of a decoder layer: rows ``[row_lo, row_lo + rows)`` of packed view
    ``view``; ``A`` fp32 ``[R, cols]`` and ``Bs`` = b' fp32 ``[rows, R]``, both views of the layer's
    pinned block at byte ``off`` (A first, then Bs)."""
    module: str
    view: str
    row_lo: int
    rows: int
    cols: int
    r: int
    scale: float
    off: int
    A: torch.Tensor
    Bs: torch.Tensor

    @property
    def R(self) -> int:
        return padded_rank(self.r)

    @property
    def nbytes(self) -> int:
        return 4 * self.R * (self.rows + self.cols)


def _pattern_value(pattern: dict, module: str, what: str):
    hit = [k for k in pattern if re.match(rf"(.*\.)?({k})$", module)]
    if len(hit) > 1:
        raise ValueError(f"{what}: keys {hit} all match {module}")
    return pattern[hit[0]] if hit else None


def _module_slot(cfg: ModelConfig, layer: str, module: str) -> Tuple[str, int, int, int]:
    """(view, first row, rows, cols) of ``module``'s weight in the packed image of ``layer``."""
    lay = layer_layout(cfg, "decoder")
    for pl in placements(cfg, layer):
        if pl.hf_name == module + ".weight":
            slot = [s for s in lay.slots if s.offset <= pl.offset][-1]
            rows, cols = pl.shape
            if len(slot.shape) != 2 or slot.shape[1] != cols:
                break
            return slot.name, (pl.offset - slot.offset) // (pl.elem_size * cols), rows, cols
    raise ValueError(f"{module}: the model has no such module")


def _check_module(cfg: ModelConfig, module: str) -> str:
    """The decoder layer of an adaptable ``module``; ValueError naming it otherwise."""
    if "embed_tokens" in module or module.endswith("lm_head") or ".lm_head" in module:
        raise ValueError(f"{module}: adapters on embed_tokens / lm_head are not supported")
    m = re.match(r"^(model\.layers\.(\d+))\.(.+)$", module)
    if m is None:
        raise ValueError(f"{module}: the model has no such module")
    layer, idx, rest = m.group(1), int(m.group(2)), m.group(3)
    if idx >= cfg.num_hidden_layers:
        raise ValueError(f"{module}: the model has no such module ({cfg.num_hidden_layers} layers)")
    if re.search(r"(^|\.)experts\.|shared_expert", rest):
        raise ValueError(f"{module}: adapters on MoE experts are not supported")
    if rest in ("block_sparse_moe.gate", "mlp.gate", "mlp.shared_expert_gate"):
        raise ValueError(f"{module}: adapters on an MoE router are not supported")
    leaf = rest.rsplit(".", 1)[-1]
    if leaf not in TARGETS:
        raise ValueError(f"{module}: not a LoRA target ({', '.join(TARGETS)})")
    if cfg.is_moe and not rest.startswith("self_attn."):
        raise ValueError(f"{module}: on an MoE model only the attention projections take an adapter")
    return layer


def check_config(conf: dict) -> None:
    """Refuse what the merge does not implement, naming the field."""
    if str(conf.get("peft_type", "LORA")).upper() != "LORA":
        raise ValueError(f"peft_type={conf.get('peft_type')!r}: only LORA adapters are supported")
    if conf.get("use_dora"):
        raise ValueError("use_dora: DoRA adapters are not supported")
    if conf.get("bias", "none") not in ("none", None):
        raise ValueError(f"bias={conf.get('bias')!r}: only bias='none' is supported")
    if conf.get("modules_to_save"):
        raise ValueError(f"modules_to_save={conf.get('modules_to_save')!r}: not supported (must be empty)")
    if conf.get("fan_in_fan_out"):
        raise ValueError("fan_in_fan_out: transposed base weights are not supported")
    for f in ("rank_pattern", "alpha_pattern"):
        if conf.get(f) is not None and not isinstance(conf.get(f), dict):
            raise TypeError(f"{f}: expected a mapping")
    if "lora_alpha" not in conf:
        raise ValueError("lora_alpha: missing from adapter_config.json")


class LoraAdapter:
    """A loaded adapter: per decoder layer the fp32 ``A`` and pre-scaled ``B'`` of every target,
    padded to ``R``, contiguous in one pinned host block (the image the staging buffer receives)."""

    def __init__(self, cfg: ModelConfig, layers: Dict[str, List[Target]], blocks: Dict[str, torch.Tensor],
                 identity: dict, lora_scale: float, path: str = ""):
        self.cfg, self.layers, self.blocks = cfg, layers, blocks
        self.identity, self.lora_scale, self.path = identity, float(lora_scale), path
        self.merge_launches = 0

    # ------------------------------------------------------------------ facts
    @property
    def n_tensors(self) -> int:
        return 2 * sum(len(t) for t in self.layers.values())

    @property
    def rank_max(self) -> int:
        return max((t.r for ts in self.layers.values() for t in ts), default=0)

    @property
    def nbytes(self) -> int:
        return sum(b.numel() for b in self.blocks.values())

    def layer_bytes(self, name: str) -> int:
        return self.blocks[name].numel() if name in self.blocks else 0

    def staging_bytes(self) -> int:
        return max((b.numel() for b in self.blocks.values()), default=0)

    def targets(self, name: str) -> List[Target]:
        return self.layers.get(name, [])

    def by_module(self) -> Dict[str, Target]:
        return {t.module: t for ts in self.layers.values() for t in ts}

    # ------------------------------------------------------------------ loading
    @classmethod
    def load(cls, cfg: ModelConfig, path: str, lora_scale: float = 1.0, pinned: Optional[bool] = None) -> "LoraAdapter":
        from .runtime import hostmem
        from .utils.safetensors_io import load_file, read_header
        if isinstance(path, (list, tuple)):
            raise ValueError("--lora: one adapter per run")
        cp, wp = os.path.join(path, CONFIG_NAME), os.path.join(path, WEIGHTS_NAME)
        if not os.path.isfile(cp):
            raise ValueError(f"{path}: no {CONFIG_NAME}")
        if not os.path.isfile(wp):
            raise ValueError(f"{path}: no {WEIGHTS_NAME}")
        with open(cp) as f:
            raw_conf = f.read()
        conf = json.loads(raw_conf)
        check_config(conf)
        if not math.isfinite(float(lora_scale)):
            raise ValueError(f"lora_scale={lora_scale!r}: not finite")
        infos, _ = read_header(wp)
        mods: Dict[str, Dict[str, str]] = {}
        for key in sorted(infos):
            if "lora_magnitude_vector" in key:
                raise ValueError(f"{key}: DoRA (lora_magnitude_vector) is not supported")
            if "lora_embedding_" in key:
                raise ValueError(f"{key}: embedding adapters (lora_embedding_*) are not supported")
            m = re.match(r"^(.*)\.lora_([AB])\.(.*)$", key)
            if m is None:
                raise ValueError(f"{key}: not a LoRA tensor (modules_to_save and other tensors are not supported)")
            if m.group(3) != "weight":
                raise ValueError(f"{key}: more than one adapter (a named adapter's tensors) is not supported")
            if not m.group(1).startswith(PREFIX):
                raise ValueError(f"{key}: expected the prefix {PREFIX!r}")
            if infos[key].dtype not in _DTYPES:
                raise TypeError(f"{key}: adapter tensors are fp16 / bf16 / fp32, got {infos[key].dtype}")
            mods.setdefault(m.group(1)[len(PREFIX):], {})[m.group(2)] = key
        if not mods:
            raise ValueError(f"{wp}: holds no LoRA tensors")
        sd = load_file(wp)
        rslora = bool(conf.get("use_rslora"))
        plan = []                          # (layer, module, view, row_lo, rows, cols, r, scale, A key, B key)
        for module in sorted(mods):
            ab = mods[module]
            for x, y in (("A", "B"), ("B", "A")):
                if x in ab and y not in ab:
                    raise ValueError(f"{ab[x]}: lora_{x} without its lora_{y}")
            layer = _check_module(cfg, module)
            view, row_lo, rows, cols = _module_slot(cfg, layer, module)
            A, B = sd[ab["A"]], sd[ab["B"]]
            if A.dim() != 2 or B.dim() != 2 or A.shape[1] != cols or B.shape[0] != rows or A.shape[0] != B.shape[1]:
                raise ValueError(f"{module}: lora_A {tuple(A.shape)} / lora_B {tuple(B.shape)} do not fit the "
                                 f"[{rows}, {cols}] projection")
            r = int(A.shape[0])
            if not 1 <= r <= MAX_RANK:
                raise ValueError(f"{module}: r={r} is outside 1..{MAX_RANK}")
            want = _pattern_value(conf.get("rank_pattern") or {}, module, "rank_pattern")
            want = conf.get("r") if want is None else want
            if want is not None and int(want) != r:
                raise ValueError(f"{module}: the tensors have r={r}, adapter_config.json (r / rank_pattern) says {want}")
            alpha = _pattern_value(conf.get("alpha_pattern") or {}, module, "alpha_pattern")
            alpha = conf["lora_alpha"] if alpha is None else alpha
            for k in (ab["A"], ab["B"]):
                if not bool(torch.isfinite(sd[k].to(torch.float32)).all()):
                    raise ValueError(f"{k}: holds a non-finite value")
            plan.append((layer, module, view, row_lo, rows, cols, r, scale_of(alpha, r, lora_scale, rslora), A, B))
        pin = torch.cuda.is_available() if pinned is None else pinned
        layers: Dict[str, List[Target]] = {}
        blocks: Dict[str, torch.Tensor] = {}
        for layer in sorted({p[0] for p in plan}, key=lambda n: int(n.rsplit(".", 1)[1])):
            mine = sorted((p for p in plan if p[0] == layer), key=lambda p: (p[2] not in ("wqkv", "wo"), p[2], p[3]))
            total = sum(4 * padded_rank(p[6]) * (p[4] + p[5]) for p in mine)
            block = hostmem.alloc_host(total, pinned=pin)
            block.zero_()
            off, ts = 0, []
            for _, module, view, row_lo, rows, cols, r, s, A, B in mine:
                R = padded_rank(r)
                a = block[off:off + 4 * R * cols].view(torch.float32).view(R, cols)
                bs = block[off + 4 * R * cols:off + 4 * R * (cols + rows)].view(torch.float32).view(rows, R)
                a[:r].copy_(A.to(torch.float32))
                with np.errstate(over="ignore"):
                    bsc = (_np32(B) * np.float32(s)).astype(np.float32)
                if not np.isfinite(bsc).all():
                    raise ValueError(f"{module}: lora_B times the scale {float(s)!r} overflows fp32")
                bs[:, :r].copy_(torch.from_numpy(bsc))
                ts.append(Target(module, view, row_lo, rows, cols, r, float(s), off, a, bs))
                off += 4 * R * (cols + rows)
            layers[layer], blocks[layer] = ts, block
        # what tells this adapter from another one (the resume fingerprint, a merged host store):
        # the config, the safetensors' size, a hash of its header and one of its bytes (two adapters
        # trained with one recipe share config, size and header), and lora_scale
        hdr, data = hashlib.sha256(), hashlib.blake2b(digest_size=16)
        with open(wp, "rb") as f:
            (n,) = struct.unpack("<Q", f.read(8))
            hdr.update(f.read(n))
            for chunk in iter(lambda: f.read(1 << 22), b""):
                data.update(chunk)
        identity = {"config": json.dumps(conf, sort_keys=True), "weights_bytes": os.path.getsize(wp),
                    "header_sha256": hdr.hexdigest(), "data_blake2b": data.hexdigest(),
                    "lora_scale": float(lora_scale)}
        return cls(cfg, layers, blocks, identity, lora_scale, path)

    # ------------------------------------------------------------------ the merge
    def new_staging(self, device, n: int = 1) -> Optional["Staging"]:
        """The device staging buffers of one owner (a runner, a host store's one-off merge): ``n``
        buffers of the largest layer's A + Bs, allocated now; None on the CPU."""
        dev = torch.device(device)
        if dev.type != "cuda" or not self.staging_bytes():
            return None
        return Staging(self.staging_bytes(), dev, n)

    def merge_views(self, ops, name: str, views: Dict[str, torch.Tensor], staging: Optional["Staging"] = None) -> int:
        """Merge the targets of layer ``name`` whose packed view is in ``views`` (a whole layer, or the
        piece that landed), in place, on the current stream.  On a GPU each target's A / Bs go H2D
        from the pinned block into the caller's ``staging`` buffer right before its launch (the
        stream orders the buffer's reuse).  Returns the launches."""
        done = 0
        for t in self.targets(name):
            if t.view not in views:
                continue
            w = views[t.view]
            if w.dim() != 2 or w.shape[1] != t.cols or w.dtype != torch.float16:
                raise ValueError(f"{t.module}: the packed view {t.view} is {tuple(w.shape)} {w.dtype}")
            rows = w[t.row_lo:t.row_lo + t.rows]
            if rows.is_cuda:
                if staging is None:
                    raise ValueError("merge_views on a GPU needs the caller's staging buffers (new_staging)")
                st = staging.buffer(rows.device)
                seg = st[t.off:t.off + t.nbytes]
                seg.copy_(self.blocks[name][t.off:t.off + t.nbytes], non_blocking=True)
                a = seg[:4 * t.R * t.cols].view(torch.float32).view(t.R, t.cols)
                bs = seg[4 * t.R * t.cols:].view(torch.float32).view(t.rows, t.R)
                ops.lora_merge(rows, a, bs, t.r)
            else:
                ops.lora_merge(rows, t.A, t.Bs, t.r)
            done += 1
        self.merge_launches += done
        return done


class Staging:
    """Device staging buffers for one owner's merges: allocated ahead, outside the caching
    allocator (the engine does it before any memory is measured for a VRAM plan); a stream that
    merges takes one and keeps it, so the stream orders its reuse.  The owner drops them
    (:meth:`release`) after synchronising."""

    def __init__(self, nbytes: int, device: torch.device, n: int = 1):
        from .runtime import hostmem
        self.nbytes, self.dev = nbytes, device
        self._spare = [hostmem.alloc_device(nbytes, device) for _ in range(n)]
        self._by_stream: Dict[int, torch.Tensor] = {}

    def buffer(self, device: torch.device) -> torch.Tensor:
        from .runtime import hostmem
        key = int(torch.cuda.current_stream(device).cuda_stream)
        if key not in self._by_stream:
            self._by_stream[key] = self._spare.pop() if self._spare else hostmem.alloc_device(self.nbytes, self.dev)
        return self._by_stream[key]

    def device_bytes(self) -> int:
        return sum(t.numel() for t in self._spare) + sum(t.numel() for t in self._by_stream.values())

    def release(self) -> None:
        self._spare.clear()
        self._by_stream.clear()


# --------------------------------------------------------------------------- twins and fixtures
def merge_state_dict(sd: Dict[str, torch.Tensor], mods: Dict[str, Target], merge=None) -> Dict[str, torch.Tensor]:
    """One file's tensors with every adapted ``<module>.weight`` replaced by its merged fp16."""
    out = {}
    for k, v in sd.items():
        t = mods.get(k[:-len(".weight")]) if k.endswith(".weight") else None
        if t is None:
            out[k] = v
            continue
        if v.dtype not in _DTYPES or tuple(v.shape) != (t.rows, t.cols):
            raise TypeError(f"{k}: {v.dtype} {tuple(v.shape)} cannot take the adapter (an fp16 / bf16 / fp32 "
                            f"[{t.rows}, {t.cols}] weight can: merge a quantised checkpoint's fp16 twin)")
        w16 = v.to(torch.float16).contiguous()
        if merge is not None:
            out[k] = merge(w16, t)
        else:
            out[k] = torch.from_numpy(merge_reference(w16, t.A[:t.r], t.Bs[:, :t.r], None))
    return out


def ops_merge(device):
    """``merge(w16, target)`` for :func:`write_twin` through ``get_ops(device)``: the HIP kernel on a
    GPU, the numpy definition on the CPU (slow for large models: seconds per 70B-sized tensor)."""
    from .ops import get_ops
    dev = torch.device(device)
    ops = get_ops(dev)

    def merge(w16: torch.Tensor, t: Target) -> torch.Tensor:
        w = w16.to(dev).contiguous()
        ops.lora_merge(w, t.A.to(dev), t.Bs.to(dev), t.r)
        return w.cpu()
    return merge


def write_twin(model_dir: str, adapter: LoraAdapter, out_dir: str, merge=None) -> None:
    """Write the merged fp16 twin of the checkpoint directory ``model_dir`` (per-layer files or an HF
    directory of safetensors files; fp16 / bf16 / fp32 weights — for a quantised base, the fp16 twin
    written by ``fp8.write_twin`` / ``int4.write_twin``) to ``out_dir``.  ``merge(w16, target)``
    replaces the numpy definition (``prepare_weights.py --merge_lora`` on a GPU)."""
    from .utils.safetensors_io import load_file, save_file
    os.makedirs(out_dir, exist_ok=True)
    mods, seen = adapter.by_module(), set()
    for fn in sorted(glob.glob(os.path.join(model_dir, "*"))):
        base = os.path.basename(fn)
        if os.path.isdir(fn):
            continue
        if base.endswith(".safetensors"):
            sd = load_file(fn)
            seen |= {k[:-len(".weight")] for k in sd if k.endswith(".weight")} & set(mods)
            save_file(merge_state_dict(sd, mods, merge), os.path.join(out_dir, base))
        else:
            shutil.copy(fn, os.path.join(out_dir, base))
    missing = sorted(set(mods) - seen)
    if missing:
        raise ValueError(f"{model_dir}: holds no weight of the adapted modules {missing[:4]}")


def target_modules(cfg: ModelConfig, targets: Sequence[str]) -> List[str]:
    """HF module paths of the projections named ``targets`` (e.g. ``q_proj``) in every decoder layer."""
    out = []
    for name in cfg.layer_names():
        if layer_kind(name) != "decoder":
            continue
        for t in targets:
            sub = "self_attn" if t in ("q_proj", "k_proj", "v_proj", "o_proj", "qkv_proj") else "mlp"
            out.append(f"{name}.{sub}.{t}")
    return out


def default_targets(cfg: ModelConfig) -> Tuple[str, ...]:
    """Every target the model has (MoE: the attention projections)."""
    attn = ("qkv_proj", "o_proj") if cfg.fused_projections else ("q_proj", "k_proj", "v_proj", "o_proj")
    if cfg.is_moe:
        return attn
    return attn + (("gate_up_proj", "down_proj") if cfg.fused_projections else ("gate_proj", "up_proj", "down_proj"))


def write_synthetic_adapter(cfg: ModelConfig, out_dir: str, r: int = 8, targets: Optional[Sequence[str]] = None,
                            seed: int = 0, dtype: torch.dtype = torch.float16, alpha: Optional[float] = None,
                            std: float = 0.05, **config) -> str:
    """A random adapter in PEFT's saved form (tests and measurements): normal ``A`` and ``B`` of
    standard deviation ``std`` on ``targets`` (default: every target the model has) of every decoder
    layer; extra ``config`` fields go into ``adapter_config.json``."""
    from .utils.safetensors_io import save_file
    os.makedirs(out_dir, exist_ok=True)
    targets = tuple(default_targets(cfg) if targets is None else targets)
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for module in target_modules(cfg, targets):
        _, _, rows, cols = _module_slot(cfg, _check_module(cfg, module), module)
        sd[f"{PREFIX}{module}.lora_A.weight"] = (torch.randn(r, cols, generator=g) * std).to(dtype)
        sd[f"{PREFIX}{module}.lora_B.weight"] = (torch.randn(rows, r, generator=g) * std).to(dtype)
    conf = {"peft_type": "LORA", "task_type": "CAUSAL_LM", "r": r, "lora_alpha": float(2 * r if alpha is None else alpha),
            "target_modules": list(targets), "bias": "none", "fan_in_fan_out": False, "use_rslora": False,
            "use_dora": False, "modules_to_save": None, "rank_pattern": {}, "alpha_pattern": {}, "lora_dropout": 0.0}
    conf.update(config)
    with open(os.path.join(out_dir, CONFIG_NAME), "w") as f:
        json.dump(conf, f, indent=1, sort_keys=True)
    save_file(sd, os.path.join(out_dir, WEIGHTS_NAME))
    return out_dir
