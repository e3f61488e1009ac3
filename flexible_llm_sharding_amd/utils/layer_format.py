"""Per-layer checkpoint conversion (``prepare_weights.py``) and layer-file paths.

Reference: ``/root/reference/prepare_weights.py:12-49``.  Each parameter maps
to the layer ``'.'.join(name.replace('.weight','').split('.')[:3])``
(``prepare_weights.py:21``); every non-``.bin`` file (config, tokenizer) is
copied; each layer is written to ``{out}/{layer}.safetensors`` keeping full HF
names and dtype.

Fixes over the reference: ``model.safetensors.index.json`` and
single-file checkpoints are supported besides ``pytorch_model.bin.index.json``;
layers are processed in source-shard order and source tensors are evicted as
soon as their layer is written.  ``.bin`` shards are read with
``torch.load(weights_only=True)`` (never unpickling arbitrary objects).
"""
from __future__ import annotations

import glob
import json
import os
import shutil
from collections import OrderedDict, defaultdict
from typing import Dict, List

import torch

from .. import quant
from .safetensors_io import load_file, save_file


def canonical_param(name: str) -> str:
    """The tensor's name in a causal-LM checkpoint.  ``AutoModel.save_pretrained`` (the published
    embedding checkpoints) writes the bare model's names — ``embed_tokens.weight``, ``layers.N.*``,
    ``norm.weight`` — which get the ``model.`` prefix here, so their layer files are the usual ones.
    A classifier head is ``score.*`` in either naming (``score.safetensors``, classify.py)."""
    if name.startswith("model.score."):
        return name[len("model."):]    # (a head saved under the body's prefix)
    return "model." + name if name.startswith(("embed_tokens.", "layers.", "norm.")) else name


def layer_of_param(name: str) -> str:
    """prepare_weights.py:21 — first three dotted components after stripping '.weight' (of the
    canonical name: a prefix-less ``layers.0.self_attn.q_proj.weight`` belongs to ``model.layers.0``)."""
    name = canonical_param(name)
    if name.startswith("score."):
        return "score"                 # the classifier head (classify.py): score.weight and score.bias together
    return ".".join(name.replace(".weight", "").split(".")[:3])


def normalize_expert_names(model_type: str, sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """MoE state dicts in transformers-v5 form (``mlp.experts.gate_up_proj`` [E, 2I, H] /
    ``mlp.experts.down_proj`` [E, H, I], Mixtral's router as ``mlp.gate``) -> the per-expert tensors
    of the released checkpoints (Mixtral ``block_sparse_moe.experts.e.w1/w3/w2``, Qwen3-MoE
    ``mlp.experts.e.gate_proj/up_proj/down_proj``), the one form the per-layer files hold
    (``models.layout.placements``).  Other keys pass through."""
    if model_type not in ("mixtral", "qwen3_moe", "qwen2_moe"):
        return sd
    out = {}
    for k, v in sd.items():
        if k.endswith(".mlp.experts.gate_up_proj") or k.endswith(".mlp.experts.down_proj"):
            p = k[:-len(".mlp.experts.gate_up_proj")] if k.endswith("gate_up_proj") else k[:-len(".mlp.experts.down_proj")]
            for e in range(v.shape[0]):
                if model_type == "mixtral":
                    b = f"{p}.block_sparse_moe.experts.{e}"
                    names = (f"{b}.w1.weight", f"{b}.w3.weight", f"{b}.w2.weight")
                else:
                    b = f"{p}.mlp.experts.{e}"
                    names = (f"{b}.gate_proj.weight", f"{b}.up_proj.weight", f"{b}.down_proj.weight")
                if k.endswith("gate_up_proj"):
                    g, u = v[e].chunk(2, 0)
                    out[names[0]], out[names[1]] = g.contiguous(), u.contiguous()
                else:
                    out[names[2]] = v[e].contiguous()
        elif model_type == "mixtral" and k.endswith(".mlp.gate.weight"):
            out[k[:-len(".mlp.gate.weight")] + ".block_sparse_moe.gate.weight"] = v
        else:
            out[k] = v
    return out


def layer_file(model_path: str, layer_name: str) -> str:
    return os.path.join(model_path, f"{layer_name}.safetensors")


def _weight_map(src: str) -> Dict[str, str]:
    for idx in ("pytorch_model.bin.index.json", "model.safetensors.index.json"):
        p = os.path.join(src, idx)
        if os.path.exists(p):
            with open(p) as f:
                return json.load(f)["weight_map"]
    for single in ("model.safetensors", "pytorch_model.bin"):
        p = os.path.join(src, single)
        if os.path.exists(p):
            if single.endswith(".safetensors"):
                from .safetensors_io import read_header
                names = read_header(p)[0].keys()
            else:
                names = torch.load(p, map_location="cpu", weights_only=True).keys()
            return {n: single for n in names}
    raise FileNotFoundError(f"{src}: no weight index / checkpoint found")


def _load_shard(path: str) -> Dict[str, torch.Tensor]:
    if path.endswith(".safetensors"):
        return load_file(path)
    return torch.load(path, map_location="cpu", weights_only=True)


def split_into_layers(src_dir: str, out_dir: str, verbose: bool = True, quantize: str = None,
                      fp8_scale: str = "channel", int4_group: int = 128, int4_scale_dtype=torch.float16,
                      nf4_block: int = 64, nf4_double_quant: bool = True) -> List[str]:
    """Convert an HF checkpoint directory into per-layer safetensors files.

    An FP8 (e4m3fn) source checkpoint passes through unchanged: its scale tensors (``weight_scale``,
    ``weight_scale_inv``, ``input_scale``) follow their weight into the layer file.
    ``quantize="fp8"`` writes the decoder layers' projection weights as FP8 with ``fp8_scale``
    scales (fp8.quantize_state_dict).  An INT4 (W4A16) source checkpoint passes through too, its
    ``weight_packed`` / ``weight_scale`` / ``weight_shape`` tensors in their weight's layer file;
    ``quantize="int4"`` writes the same weights as INT4 in groups of ``int4_group`` with
    ``int4_scale_dtype`` scales (int4.quantize_state_dict).  A bitsandbytes 4-bit source checkpoint
    passes through with its bytes unchanged, the companions of a weight (``X.weight.absmax``,
    ``.quant_map``, ``.nested_*``, ``.quant_state.bitsandbytes__nf4``) in its layer file;
    ``quantize="nf4"`` writes that form from float weights (nf4.quantize_state_dict).  An MXFP4
    source checkpoint (U8 ``weight`` and U8 ``weight_scale``) passes through with its bytes unchanged;
    ``quantize="mxfp4"`` writes that form from float weights (mxfp4.quantize_state_dict).  A GPTQ or
    AWQ source checkpoint (``qweight`` / ``qzeros`` / ``scales`` / ``g_idx``) passes through with its
    bytes unchanged and keeps its ``quantization_config`` (``config.json`` is copied);
    ``quantize="gptq"`` / ``"awq"`` writes those forms from float weights in groups of ``int4_group``
    (gptq.quantize_state_dict)."""
    if quantize is not None:
        quant.quantize_format(quantize)         # (an unknown name is refused before anything is written)
    os.makedirs(out_dir, exist_ok=True)
    for fn in glob.glob(os.path.join(src_dir, "*")):
        base = os.path.basename(fn)
        if os.path.isdir(fn):
            continue
        if ".bin" in base or base.endswith(".safetensors") or base.endswith(".index.json"):
            continue
        shutil.copy(fn, os.path.join(out_dir, base))

    wmap = _weight_map(src_dir)
    layer_params: Dict[str, List[str]] = defaultdict(list)
    for p in wmap:
        layer_params[layer_of_param(p)].append(p)
    # (a checkpoint with neither lm_head nor tied embeddings — a bare embedding model — has no head
    # file: it runs in --score_mode embed only)
    tied = ("lm_head" not in layer_params and "model.embed_tokens.weight" in {canonical_param(p) for p in wmap}
            and _tied(src_dir))
    model_type = _config(src_dir).get("model_type", "llama")
    # deterministic order: by the (sorted) source shards each layer needs
    shard_order = {s: i for i, s in enumerate(sorted(set(wmap.values())))}
    layers = sorted(layer_params, key=lambda l: (max(shard_order[wmap[p]] for p in layer_params[l]), l))
    # last layer that needs each shard -> evict after it
    last_use = {}
    for l in layers:
        for p in layer_params[l]:
            last_use[wmap[p]] = l

    cache: "OrderedDict[str, Dict[str, torch.Tensor]]" = OrderedDict()
    written = []
    it = layers
    if verbose:
        try:
            from tqdm import tqdm
            it = tqdm(layers, desc="split_into_layers")
        except Exception:  # pragma: no cover
            pass
    for l in it:
        need = sorted({wmap[p] for p in layer_params[l]})
        for s in need:
            if s not in cache:
                cache[s] = _load_shard(os.path.join(src_dir, s))
        sd = {}
        for p in layer_params[l]:
            sd[canonical_param(p)] = cache[wmap[p]][p]
        assert len(sd) == len(layer_params[l]), f"Should have {len(layer_params[l])} keys for {l}"
        out_sd = normalize_expert_names(model_type, sd)
        if quantize and l != "score":              # (the head stays as it is: a quantised one is refused)
            out_sd = quant.quantize_state_dict(out_sd, quantize, fp8_scale, int4_group, int4_scale_dtype, nf4_block,
                                               nf4_double_quant)
        save_file(out_sd, layer_file(out_dir, l))
        written.append(l)
        if tied and l == "model.embed_tokens":
            # tie_word_embeddings checkpoints store no lm_head: give the head its own layer file so
            # the per-layer format stays complete (the reference would fail to open lm_head here)
            save_file({"lm_head.weight": sd["model.embed_tokens.weight"].clone()}, layer_file(out_dir, "lm_head"))
            written.append("lm_head")
        for s in need:
            if last_use.get(s) == l:
                cache.pop(s, None)
    return written


def _config(src_dir: str) -> dict:
    try:
        with open(os.path.join(src_dir, "config.json")) as f:
            return json.load(f)
    except (OSError, ValueError):
        return {}


def _tied(src_dir: str) -> bool:
    return bool(_config(src_dir).get("tie_word_embeddings", False))
