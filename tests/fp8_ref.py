"""Shared fixtures of the FP8 tests: an FP8 checkpoint of a tiny preset and its fp16 twin.

The twin (fp8.write_twin) is the same directory with every FP8 tensor replaced by
``w16 = fp16(fp32(e4m3fn(b)) * scale)`` and the scale tensors removed; the whole feature is that a
run on the FP8 checkpoint equals the same run on the twin bit for bit.
"""
import os

import torch

from flexible_llm_sharding_amd import fp8
from flexible_llm_sharding_amd.config import preset
from flexible_llm_sharding_amd.utils.layer_format import layer_file
from flexible_llm_sharding_amd.utils.safetensors_io import load_file, save_file
from flexible_llm_sharding_amd.utils.synthetic import synthetic_prompts, write_synthetic_checkpoint

EXTREME_SCALES = (1.0, 2.0 ** -20, 3.7e-3, 448.0, 2.0 ** 12)


def torch_dequant(bits: torch.Tensor, scale_full: torch.Tensor) -> torch.Tensor:
    """The issue's one-line definition with torch's own casts (scale broadcast by the caller)."""
    return (bits.view(torch.float8_e4m3fn).float() * scale_full).half()


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """fp16 tensors equal bit for bit, NaN patterns compared with isnan."""
    a, b = a.cpu(), b.cpu()
    na, nb = torch.isnan(a), torch.isnan(b)
    if not torch.equal(na, nb):
        return False
    return torch.equal(a.view(torch.int16)[~na], b.view(torch.int16)[~nb])


def scales_to(path: str, dtype) -> None:
    """Rewrite the layer files of ``path`` with their scale tensors stored as ``dtype``."""
    for fn in sorted(os.listdir(path)):
        if fn.endswith(".safetensors"):
            sd = load_file(os.path.join(path, fn))
            if any(fp8.is_scale_name(k) for k in sd):
                save_file({k: (v.to(dtype) if fp8.is_scale_name(k) else v) for k, v in sd.items()},
                          os.path.join(path, fn))


def make_pair(root, name: str, scale: str, seed: int = 3, scale_dtype=None):
    """(cfg, fp8 dir, twin dir) of preset ``name`` quantised with ``scale`` scales."""
    cfg = preset(name)
    q, t = os.path.join(str(root), f"{name}_{scale}_fp8"), os.path.join(str(root), f"{name}_{scale}_twin")
    write_synthetic_checkpoint(cfg, q, seed=seed, std=0.05, quantize="fp8", fp8_scale=scale)
    if scale_dtype is not None:
        scales_to(q, scale_dtype)
    fp8.write_twin(q, t)
    return cfg, q, t


def prompts_for(cfg, n: int = 3, seed: int = 5):
    return synthetic_prompts(n, 24, 3, 6, cfg.vocab_size, seed=seed, vary=True)


def decoder_names(cfg):
    return [n for n in cfg.layer_names() if n.startswith("model.layers.")]


def file_tensor_bytes(path: str, name: str) -> int:
    """Bytes of the tensors of a layer file that are not scale tensors."""
    sd = load_file(layer_file(path, name))
    return sum(v.numel() * v.element_size() for k, v in sd.items() if not fp8.is_scale_name(k))
