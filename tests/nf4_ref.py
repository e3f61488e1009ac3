"""Independent oracle and shared fixtures of the NF4 (bitsandbytes 4-bit) tests.

The oracle is plain loops over ``np.float32`` operations on the stored tensors: one nibble, one
multiply, one cast per weight; for a U8 absmax one multiply and one add per block, each rounded on
its own.  It does not import ``nf4.py``.  The fixtures build an NF4 checkpoint of a tiny preset and
its fp16 twin (they use the package's writer and ``write_twin``).
"""
import os

import numpy as np
import torch

# the published NF4 code book, typed here
NF4 = (-1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453,
       -0.28444138169288635, -0.18477343022823334, -0.09105003625154495, 0.0,
       0.07958029955625534, 0.16093020141124725, 0.24611230194568634, 0.33791524171829224,
       0.44070982933044434, 0.5626170039176941, 0.7229568362236023, 1.0)

# block scales that reach every special result: sign of zero, fp16 subnormals (1e-6 .. 6e-5 times a
# code entry), results that vanish (1e-8), the largest finite fp16, overflow (1e5, 3e38), an exact
# fp16 rounding tie with the entry 1.0 (1 + 2^-11) and its neighbour above
EXTREME = (-1.0, -3.7e-3, 0.0, -0.0, 2.0 ** -24, 65504.0, 1e5, 3e38, 1.0, 2.0 ** -14, 1.0 + 2.0 ** -11,
           1.0 + 2.0 ** -11 + 2.0 ** -23, 1e-8, 1e-6, 6e-5, -65520.0)


def ref_scales(absmax: np.ndarray, code2=None, nested=None, b2: int = 0, offset: float = 0.0) -> np.ndarray:
    """fp32 ``s_k`` of every block."""
    out = np.zeros(len(absmax), dtype=np.float32)
    off = np.float32(offset)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(len(absmax)):
            if absmax.dtype == np.float32:
                out[k] = absmax[k]
            else:
                assert absmax.dtype == np.uint8
                p = np.float32(code2[int(absmax[k])]) * np.float32(nested[k // b2])        # rounded to fp32
                out[k] = np.float32(p) + off                                             # rounded again
    return out


def ref_dequant(packed: np.ndarray, code, absmax: np.ndarray, n: int, block: int, code2=None, nested=None,
                b2: int = 0, offset: float = 0.0) -> torch.Tensor:
    """fp16 [n]: flat element i is the HIGH nibble of byte i // 2 for an even i, the low one for an odd i."""
    assert packed.dtype == np.uint8 and len(packed) * 2 == n and len(absmax) * block == n
    s = ref_scales(absmax, code2, nested, b2, offset)
    c = [np.float32(x) for x in code]
    out = np.zeros(n, dtype=np.float16)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(n):
            by = int(packed[i // 2])
            u = (by >> 4) if i % 2 == 0 else (by & 15)
            out[i] = np.float16(np.float32(c[u] * s[i // block]))
    return torch.from_numpy(out)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """fp16 tensors equal bit for bit; NaN equals NaN of any payload."""
    a, b = a.cpu().reshape(-1), b.cpu().reshape(-1)
    if a.shape != b.shape or a.dtype != torch.float16 or b.dtype != torch.float16:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    if not torch.equal(na, nb):
        return False
    return torch.equal(a.view(torch.int16)[~na], b.view(torch.int16)[~nb])


def lanes(n: int) -> np.ndarray:
    """Nibbles that put each of the 16 values into each of the 32 positions of a thread's vector (so
    into both halves of every byte): element i holds (i // 32 + i % 32) % 16."""
    i = np.arange(n, dtype=np.int64)
    return ((i // 32 + i % 32) % 16).astype(np.uint8)


def pack(nibbles: np.ndarray) -> np.ndarray:
    """Packed bytes of flat nibbles 0..15: the even element in the high nibble."""
    u = nibbles.astype(np.uint8).reshape(-1, 2)
    return ((u[:, 0] << 4) | u[:, 1]).astype(np.uint8)


def full_mantissa_code(rng: np.random.Generator) -> np.ndarray:
    """An arbitrary sorted code book: -1, 0, 1 and 13 random fp32 values with all 24 mantissa bits in use."""
    v = rng.uniform(-1, 1, 13).astype(np.float32)
    v = (v.view(np.uint32) | np.uint32(1)).view(np.float32)             # (the last mantissa bit set)
    return np.sort(np.concatenate([v, np.array([-1.0, 0.0, 1.0], dtype=np.float32)])).astype(np.float32)


def f32_absmax(n_blocks: int, rng: np.random.Generator, extreme: bool) -> np.ndarray:
    if extreme:
        pool = np.array(EXTREME, dtype=np.float32)
        return pool[(np.arange(n_blocks) + rng.integers(0, len(pool))) % len(pool)]     # (every entry, in turn)
    return ((rng.random(n_blocks) + 0.5) * 2e-2).astype(np.float32)


def u8_absmax(n_blocks: int, b2: int, rng: np.random.Generator, extreme: bool):
    """(absmax U8, code2 fp32 [256], nested fp32, offset) of a double-quantised tensor.  ``extreme``:
    code2 and the nested values come from the special pool, so that ``s_k`` takes the special values
    (with offset -0.0 a product of -0 stays -0)."""
    q = rng.integers(0, 256, n_blocks).astype(np.uint8)
    nb = -(-n_blocks // b2)
    if extreme:
        pool = np.array([x for x in EXTREME if abs(x) < 1e30], dtype=np.float32)
        code2 = pool[np.arange(256) % len(pool)]
        nested = np.array([1.0, -1.0, 2.0 ** -14, 1.0 + 2.0 ** -23], dtype=np.float32)[np.arange(nb) % 4]
        return q, code2.astype(np.float32), nested, -0.0
    code2 = np.sort(rng.uniform(-1, 1, 256)).astype(np.float32)
    nested = ((rng.random(nb) + 0.5) * 1e-2).astype(np.float32)
    return q, code2, nested, 0.021


def t(x: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(x))


# ------------------------------------------------------------------ checkpoints
def make_pair(root, name: str, double_quant: bool, block: int = 64, seed: int = 3):
    """(cfg, nf4 dir, twin dir) of preset ``name``."""
    from flexible_llm_sharding_amd import nf4
    from flexible_llm_sharding_amd.config import preset
    from flexible_llm_sharding_amd.utils.synthetic import write_synthetic_checkpoint
    cfg = preset(name)
    tag = f"{name}_b{block}_{'dq' if double_quant else 'f32'}"
    q, tw = os.path.join(str(root), tag + "_nf4"), os.path.join(str(root), tag + "_twin")
    if not os.path.isdir(tw):
        write_synthetic_checkpoint(cfg, q, seed=seed, std=0.05, quantize="nf4", nf4_block=block,
                                   nf4_double_quant=double_quant)
        nf4.write_twin(q, tw)
    return cfg, q, tw


def prompts_for(cfg, n: int = 3, seed: int = 5):
    from flexible_llm_sharding_amd.utils.synthetic import synthetic_prompts
    return synthetic_prompts(n, 24, 3, 6, cfg.vocab_size, seed=seed, vary=True)


def moved_bytes(path: str, name: str) -> int:
    """Bytes of a layer file's tensors that a pass moves: everything but the small tables of the
    4-bit weights (code books, nested absmax, quant state), which are read once when the file is planned."""
    from flexible_llm_sharding_amd.utils.layer_format import layer_file
    from flexible_llm_sharding_amd.utils.safetensors_io import load_file
    sd = load_file(layer_file(path, name))
    small = (".quant_map", ".nested_absmax", ".nested_quant_map")
    return sum(v.numel() * v.element_size() for k, v in sd.items()
               if not k.endswith(small) and ".quant_state." not in k)
