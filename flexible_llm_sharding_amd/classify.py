"""Reward and classifier heads per suffix (``--score_mode classify``): the definition.

A ``*ForSequenceClassification`` / ``*ForTokenClassification`` checkpoint is the decoder this
project runs plus a linear head ``score.weight [L, H]`` (``score.bias [L]`` optional).  Let
``y16[r, :]`` be the final-norm rows in fp16 as ``fls_rmsnorm`` writes them (the rows embed mode
pools), ``w16 = fp16_rne(score.weight)`` (an fp16 checkpoint's bits as they are) and
``b = float32(score.bias)`` (0 when absent).  Then

    z[r, l] = sum_k float32(y16[r, k]) * float32(w16[l, k]) + b[l]          (fp32 accumulation)

and ``--classify_activation none | softmax | sigmoid`` is applied to ``z[r, :]`` in fp32 (softmax
max-subtracted; refused with L = 1, where it is the constant 1).

``--classify_rows last`` returns the row of each suffix's last token — the row the LM head would
score; HF's sequence classification without padding — as one float32 ``[n_s, L]`` array per prompt.
``all`` returns every suffix token in order (token classification, process reward models) as a
list of ``n_s`` float32 ``[len_s, L]`` arrays per prompt; prefix rows are never returned.

On the GPU ``csrc/kernels/classify.hip`` (``fls_classify_rows``) computes it; a row's bits depend on
that row, ``w16``, ``b`` and H only, so neither the other suffixes of a call nor its split into
micro-batches change a value.  The CPU backend computes the same sums in fp32 on fp32 norm rows.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from . import embed

ROWS = ("last", "all")
ACTIVATIONS = ("none", "softmax", "sigmoid")
MAX_LABELS = 64
SYNTHETIC_LABELS = 2           # labels of a --synthetic head when the preset names none (HF's default)
LAYER = "score"


@dataclass(frozen=True)
class ClassifyParams:
    rows: str = "last"
    activation: str = "none"
    num_labels: int = 0          # 0: not resolved against a head yet

    def resolved(self, num_labels: int) -> "ClassifyParams":
        check_classify_values(self.rows, self.activation)
        L = int(num_labels)
        if not 1 <= L <= MAX_LABELS:
            raise ValueError(f"score.weight: {L} labels, 1..{MAX_LABELS} are served")
        if self.activation == "softmax" and L == 1:
            raise ValueError("--classify_activation softmax over one label is the constant 1: use none or sigmoid")
        return ClassifyParams(self.rows, self.activation, L)

    @classmethod
    def from_args(cls, args) -> "ClassifyParams":
        return cls(getattr(args, "classify_rows", None) or "last", getattr(args, "classify_activation", None) or "none")


def check_classify_values(rows, activation) -> None:
    if rows not in ROWS:
        raise ValueError(f"--classify_rows must be one of {ROWS}, got {rows!r}")
    if activation not in ACTIVATIONS:
        raise ValueError(f"--classify_activation must be one of {ACTIVATIONS}, got {activation!r}")


def layer_names(cfg, score_mode: str = "next_token") -> List[str]:
    """The layer files a run of ``score_mode`` needs: embed's list (the pass ends at ``model.norm``;
    ``lm_head`` need not exist) plus, for classify, ``"score"``."""
    if score_mode == "classify":
        return embed.layer_names(cfg, "embed") + [LAYER]
    return embed.layer_names(cfg, score_mode)


def pass_layer_names(cfg, score_mode: str = "next_token") -> List[str]:
    """The layers a runner of ``score_mode`` plans, streams and runs.  A classify pass is an embed
    pass: the head is no streamed layer (it lives in a device buffer of its own, loaded once)."""
    return embed.layer_names(cfg, "embed" if score_mode == "classify" else score_mode)


def reference(y16, w, b, params: ClassifyParams) -> np.ndarray:
    """The definition in numpy float64: ``y16`` [rows, H] (fp16 values), ``w`` [L, H] (rounded to
    fp16 unless it is fp16), ``b`` [L] or None -> float64 [rows, L]."""
    y = np.asarray(y16).astype(np.float64)
    w = np.asarray(w)
    w = (w if w.dtype == np.float16 else w.astype(np.float32).astype(np.float16)).astype(np.float64)
    z = y @ w.T
    if b is not None:
        z = z + np.asarray(b).astype(np.float32).astype(np.float64)[None, :]
    if params.activation == "softmax":
        if z.shape[1] == 1:
            raise ValueError("--classify_activation softmax over one label is the constant 1: use none or sigmoid")
        e = np.exp(z - z.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)
    if params.activation == "sigmoid":
        return 1.0 / (1.0 + np.exp(-z))
    if params.activation != "none":
        raise ValueError(f"--classify_activation must be one of {ACTIVATIONS}, got {params.activation!r}")
    return z


@dataclass
class Head:
    """A validated head on the host: ``w16`` fp16 [L, H] contiguous, ``bias`` fp32 [L] or None."""
    w16: torch.Tensor
    bias: Optional[torch.Tensor]

    @property
    def num_labels(self) -> int:
        return int(self.w16.shape[0])

    def to(self, device) -> "Head":
        """A device buffer of its own (at most 64 x H fp16 plus the bias)."""
        return Head(self.w16.to(device).contiguous(), None if self.bias is None else self.bias.to(device).contiguous())


def check_head(cfg, sd: dict, where: str = LAYER) -> Head:
    """``score.weight`` / ``score.bias`` of a layer file, validated against the model -> :class:`Head`."""
    from . import quant
    w = sd.get("score.weight")
    extra = sorted(k for k in sd if k not in ("score.weight", "score.bias"))
    float_types = (torch.float16, torch.bfloat16, torch.float32)
    if w is None or extra or w.dtype not in float_types:
        names = ", ".join(f.label for f in quant.ALL_FORMATS)
        if w is None and not extra:
            raise ValueError(f"{where}: score.weight is missing")
        raise TypeError(f"{where}: score.weight must be a plain fp16 / bf16 / fp32 tensor (a quantised head — "
                        f"{names} — is not served; found {extra or str(w.dtype)})")
    H = cfg.hidden_size
    if w.dim() != 2 or w.shape[1] != H:
        raise ValueError(f"{where}: score.weight has shape {tuple(w.shape)}, [L, {H}] (L labels x the hidden size) expected")
    L = int(w.shape[0])
    want = getattr(cfg, "num_labels", None)
    if want and L != int(want):
        raise ValueError(f"{where}: score.weight has {L} rows, the config's num_labels is {want}")
    if not 1 <= L <= MAX_LABELS:
        raise ValueError(f"{where}: score.weight has {L} labels, 1..{MAX_LABELS} are served")
    b = sd.get("score.bias")
    if b is not None:
        if b.dtype not in float_types:
            raise TypeError(f"{where}: score.bias must be fp16 / bf16 / fp32, got {b.dtype}")
        if b.dim() != 1 or b.shape[0] != L:
            raise ValueError(f"{where}: score.bias has shape {tuple(b.shape)}, [{L}] expected")
        b = b.float().contiguous()
        if not bool(torch.isfinite(b).all()):
            raise ValueError(f"{where}: score.bias holds non-finite values")
    w16 = w.to(torch.float16).contiguous()           # (bf16 / fp32: round to nearest even; fp16: the bits)
    if not bool(torch.isfinite(w16.float()).all()):
        raise ValueError(f"{where}: score.weight holds non-finite values (as fp16)")
    return Head(w16, b)


def load_head(cfg, model_path: str) -> Head:
    """The head of a converted model directory (``score.safetensors``)."""
    from .utils.layer_format import layer_file
    from .utils.safetensors_io import load_file
    path = layer_file(model_path, LAYER)
    if not os.path.exists(path):
        raise ValueError(f"--score_mode classify needs {path} (score.weight [L, H]): the checkpoint has no "
                         "classifier head")
    return check_head(cfg, load_file(path), path)


def synthetic_head(cfg, seed: int = 0, num_labels: Optional[int] = None, bias: bool = True) -> dict:
    """A seeded ``score`` layer (state dict) for synthetic checkpoints: weight ~ N(0, 1/H), so
    logits of unit-RMS norm rows are ~ N(0, 1); a small bias."""
    L = int(num_labels or getattr(cfg, "num_labels", None) or SYNTHETIC_LABELS)
    g = torch.Generator().manual_seed(seed * 1000003 + 999983)
    sd = {"score.weight": (torch.randn(L, cfg.hidden_size, generator=g) * cfg.hidden_size ** -0.5).to(torch.float16)}
    if bias:
        sd["score.bias"] = (0.1 * torch.randn(L, generator=g)).to(torch.float16)
    return sd


def head_for(cfg, source) -> Head:
    """The head that belongs to a runner's weight source: the ``score.safetensors`` next to its
    layer files, or the seeded one of a synthetic store."""
    for s in (source, getattr(source, "files", None)):
        path = getattr(s, "model_path", None)
        if path:
            return load_head(cfg, path)
    seed = getattr(source, "synthetic_seed", None)
    if seed is not None:
        return check_head(cfg, synthetic_head(cfg, seed), "the synthetic score layer")
    raise ValueError("--score_mode classify: the weight source names no model directory to read "
                     "score.safetensors from (pass classify_head=classify.load_head(cfg, path))")
