"""Independent oracle and shared fixtures of the INT4 tests.

The oracle unpacks with numpy integer arithmetic on the little-endian byte stream and rounds through
numpy's float32 multiply and float16 cast; it does not import ``int4.py``.  The fixtures build an
INT4 checkpoint of a tiny preset and its fp16 twin (they use the package's writer and ``write_twin``).
"""
import os

import numpy as np
import torch

EXTREME = (-1.0, -3.7e-3, 0.0, -0.0, 2.0 ** -24, 65504.0, float("inf"), 1.0, 2.0 ** -14)
EXTREME_F32_ONLY = (1.0 + 2.0 ** -11, 1e-8)        # an exact fp16 tie; products that are fp16 subnormals


def scale_f32(scale: torch.Tensor) -> np.ndarray:
    """fp32 values of an fp16 / bf16 / fp32 scale tensor (widening is exact)."""
    return scale.detach().cpu().to(torch.float32).numpy()


def ref_unpack(packed: torch.Tensor, n: int) -> np.ndarray:
    """q (int32, -8..7) of the first ``n`` row-major elements: element i is in byte i // 2 of the
    little-endian byte stream, an even i in the low nibble."""
    by = np.frombuffer(packed.detach().cpu().contiguous().numpy().astype("<i4").tobytes(), dtype=np.uint8)
    i = np.arange(n, dtype=np.int64)
    b = by[i // 2].astype(np.int32)
    u = np.where(i % 2 == 0, b & 15, b >> 4)
    return u - 8


def ref_dequant(packed: torch.Tensor, scale: torch.Tensor, shape) -> torch.Tensor:
    out, inn = shape
    s = scale_f32(scale).reshape(out, -1)
    g = inn // s.shape[1]
    i = np.arange(out * inn, dtype=np.int64)
    q = ref_unpack(packed, out * inn).astype(np.float32)
    sc = s[i // inn, (i % inn) // g].astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        w = (q * sc).astype(np.float32).astype(np.float16)
    return torch.from_numpy(w.reshape(out, inn))


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """fp16 tensors equal bit for bit; NaN equals NaN of any payload."""
    a, b = a.cpu(), b.cpu()
    if a.shape != b.shape or a.dtype != torch.float16 or b.dtype != torch.float16:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    if not torch.equal(na, nb):
        return False
    return torch.equal(a.view(torch.int16)[~na], b.view(torch.int16)[~nb])


def ulp16(x: torch.Tensor) -> torch.Tensor:
    """Spacing of fp16 at ``|x|`` (fp64): 2^-24 below 2^-14, else 2^(floor(log2 |x|) - 10)."""
    a = x.abs().to(torch.float64).clamp_min(2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(a)) - 10)


def lanes(n: int) -> torch.Tensor:
    """Nibbles that put each of the 16 values into each of the 32 positions of a thread's vector (so
    into both halves of every byte): element i holds (i // 32 + i % 32) % 16."""
    i = torch.arange(n, dtype=torch.int64)
    return ((i // 32 + i % 32) % 16).to(torch.uint8)


def words_of(nibbles: torch.Tensor, rows: int, cols: int) -> torch.Tensor:
    """int32 words [rows, cols / 8] of row-major nibbles 0..15 (numpy, independent of int4.pack)."""
    u = nibbles.numpy().astype(np.uint8).reshape(-1, 2)
    by = (u[:, 0] | (u[:, 1] << 4)).astype(np.uint8)
    return torch.from_numpy(np.frombuffer(by.tobytes(), dtype="<i4").copy()).reshape(rows, cols // 8)


def scales(rows: int, n_col_groups: int, dtype, g: torch.Generator, extreme: bool) -> torch.Tensor:
    n = rows * n_col_groups
    if extreme:
        pool = torch.tensor(EXTREME + (EXTREME_F32_ONLY if dtype == torch.float32 else ()), dtype=torch.float32)
        s = pool[torch.randint(0, len(pool), (n,), generator=g)]
    else:
        s = (torch.rand(n, generator=g) + 0.5) * 2e-2
    return s.to(dtype).reshape(rows, n_col_groups)


def kernel_shapes(g: int, T: int):
    """(rows, cols) of the kernel-test counts g, T - g, T, T + g, 2T + g, 5T - g and 1024 x 2048 (plus
    200 x 352 at g = 32), each with cols a multiple of g; ``g == 0`` means per channel (g = cols)."""
    out = []
    gg = 256 if g == 0 else g
    for n in (gg, T - gg, T, T + gg, 2 * T + gg, 5 * T - gg):
        G = n // gg
        d = 1 if g == 0 else next(d for d in (5, 3, 2, 1) if G % d == 0)
        out.append((G // d, gg * d))
    if g == 32:
        out.append((200, 352))
    return out + [(1024, 2048)]


# ------------------------------------------------------------------ checkpoints
def make_pair(root, name: str, group: int, scale_dtype=torch.float16, seed: int = 3):
    """(cfg, int4 dir, twin dir) of preset ``name`` in groups of ``group`` (0: per channel)."""
    from flexible_llm_sharding_amd import int4
    from flexible_llm_sharding_amd.config import preset
    from flexible_llm_sharding_amd.utils.synthetic import write_synthetic_checkpoint
    cfg = preset(name)
    tag = f"{name}_g{group}_{str(scale_dtype).split('.')[-1]}"
    q, t = os.path.join(str(root), tag + "_int4"), os.path.join(str(root), tag + "_twin")
    write_synthetic_checkpoint(cfg, q, seed=seed, std=0.05, quantize="int4", int4_group=group,
                               int4_scale_dtype=scale_dtype)
    int4.write_twin(q, t)
    return cfg, q, t


def prompts_for(cfg, n: int = 3, seed: int = 5):
    from flexible_llm_sharding_amd.utils.synthetic import synthetic_prompts
    return synthetic_prompts(n, 24, 3, 6, cfg.vocab_size, seed=seed, vary=True)


def decoder_names(cfg):
    return [n for n in cfg.layer_names() if n.startswith("model.layers.")]


def file_tensor_bytes(path: str, name: str) -> int:
    """Bytes of a layer file's tensors that a pass moves: all but the 16-byte ``weight_shape``
    tensors, which are read once when the file is planned."""
    from flexible_llm_sharding_amd.utils.layer_format import layer_file
    from flexible_llm_sharding_amd.utils.safetensors_io import load_file
    sd = load_file(layer_file(path, name))
    return sum(v.numel() * v.element_size() for k, v in sd.items() if not k.endswith(".weight_shape"))
