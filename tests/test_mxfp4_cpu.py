"""MXFP4 checkpoints without a GPU: literal known answers, the converter, the landing layout against the
native host code and an in-place emulation, ``main.py`` on the torch backend against the twin, refusals."""
import ctypes
import json
import os
import pickle
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from flexible_llm_sharding_amd import mxfp4
from flexible_llm_sharding_amd.config import preset
from flexible_llm_sharding_amd.models.layout import pack_layer
from flexible_llm_sharding_amd.runtime.stream import LayerPlan
from flexible_llm_sharding_amd.utils.layer_format import layer_file
from flexible_llm_sharding_amd.utils.safetensors_io import load_file, save_file
from flexible_llm_sharding_amd.utils.synthetic import synthetic_prompts, write_synthetic_checkpoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = mxfp4.TAIL
COUNTS = [32, T, T + 32, 5 * T + 64, 8192 * 28672]
Q = "model.layers.0.self_attn.q_proj.weight"


def test_known_answer():
    packed = torch.zeros(4, 16, dtype=torch.uint8)
    packed[0, :8] = torch.tensor([0x10, 0x32, 0x54, 0x76, 0x98, 0xBA, 0xDC, 0xFE], dtype=torch.uint8)
    packed[1, 0], packed[2, 0], packed[3, 0] = 0xFE, 0x07, 0x13
    w = mxfp4.dequantize(packed, torch.tensor([[128], [255], [142], [103]], dtype=torch.uint8), (4, 32))
    got = w.view(torch.int16).numpy().view(np.uint16).tolist()
    want = [0.0, 1, 2, 3, 4, 6, 8, 12, -0.0, -1, -2, -3, -4, -6, -8, -12]
    assert got[0][:16] == [int(np.float16(x).view(np.uint16)) for x in want] and got[0][8] == 0x8000
    assert got[1] == [0x7E00] * 32 and got[2][0] == 0x7C00                   # e = 255 is NaN; 6 * 2^15 overflows
    assert got[3][:2] == [0x0002, 0x0000]                                    # 1.5 * 2^-24 and 0.5 * 2^-24: ties to even


def test_converter_rule_and_error_bound():
    g = torch.Generator().manual_seed(4)
    w = (torch.randn(48, 96, generator=g) * 0.05).to(torch.float16)
    w[0, :32] = 0                                                            # an all-zero block
    w[1, 0], w[1, 1], w[1, 2] = 4.0, 2.5, -0.25                              # scale 1: ties go to the even code
    packed, scale = mxfp4.quantize(w)
    assert (packed.dtype, tuple(packed.shape), scale.dtype, tuple(scale.shape)) == (torch.uint8, (48, 48), torch.uint8, (48, 3))
    assert int(scale[0, 0]) == 127 and int(scale[1, 0]) == 127 and mxfp4.unpack(packed)[1, :3].tolist() == [6, 4, 8]
    back = mxfp4.dequantize(packed, scale, w.shape)
    step = torch.exp2(scale.to(torch.float64) - 127).repeat_interleave(32, 1)
    assert bool(((w.double() - back.double()).abs() <= 2 * step).all())
    again = mxfp4.quantize(back)                                             # the twin converts to the same bytes
    assert torch.equal(again[0], packed) and torch.equal(again[1], scale)


def test_native_host_code_mirrors_the_schedule():
    from flexible_llm_sharding_amd import _native
    k = _native.kernels()
    assert k.fls_dequant_mxfp4_tail() == T
    out = (ctypes.c_uint64 * 6)()
    for n in COUNTS:
        lay = mxfp4.region_layout(n)
        assert k.fls_dequant_mxfp4_launches(n) == len(lay)
        for j, s in enumerate(lay):
            assert k.fls_dequant_mxfp4_segment(n, j, ctypes.addressof(out)) == 0 and tuple(out) == tuple(s), (n, j)
        assert k.fls_dequant_mxfp4_segment(n, len(lay), ctypes.addressof(out)) != 0
    assert len(mxfp4.region_layout(8192 * 28672)) == 9 and k.fls_dequant_mxfp4_launches(48) < 0 and k.fls_dequant_mxfp4_launches(0) == 0


@pytest.mark.parametrize("n", COUNTS[:-1])
def test_in_place_emulation(n):
    """Launch by launch on the byte buffer, all of a launch's reads before its writes: never a written byte read."""
    rng = np.random.default_rng(n)
    packed = torch.from_numpy(rng.integers(0, 256, (n // 32, 16)).astype(np.uint8))
    scale = torch.from_numpy(rng.integers(100, 150, (n // 32, 1)).astype(np.uint8))
    want = mxfp4.dequantize(packed, scale, (n // 32, 32)).reshape(-1)
    region = torch.full((2 * n,), 0x5A, dtype=torch.uint8)
    mxfp4.land(region, packed.reshape(-1), scale.reshape(-1), n, 32, 1)
    assert (region[:mxfp4.landing_span(n, 32, 1)[0]] == 0x5A).all()
    emu = region.clone()
    for s in mxfp4.region_layout(n):
        blocks = (s.b - s.a) // 32
        p = emu[s.packed_off:s.packed_off + blocks * 16].clone().reshape(blocks, 16)
        e = emu[s.scale_off:s.scale_off + blocks].clone().reshape(blocks, 1)
        emu[2 * s.a:2 * s.b] = mxfp4.dequantize(p, e, (blocks, 32)).reshape(-1).view(torch.uint8)
    assert torch.equal(emu.view(torch.int16), want.view(torch.int16))
    from flexible_llm_sharding_amd.ops import get_ops
    get_ops(torch.device("cpu")).dequant_mxfp4(region, n)                    # the torch backend, same landed bytes
    assert torch.equal(region.view(torch.int16), want.view(torch.int16))


# --------------------------------------------------------- main.py
def test_main_mxfp4_equals_twin(tmp_path):
    d, env = tmp_path, dict(os.environ, PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="1")
    q, twin, pp = str(d / "q"), str(d / "twin"), str(d / "prompts.pkl")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "prepare_weights.py"), "tiny", q, "--synthetic",
                        "--quantize", "mxfp4", "--std", "0.05"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    mxfp4.write_twin(q, twin)
    cfg = preset("tiny")
    pickle.dump(synthetic_prompts(4, 24, 3, 6, cfg.vocab_size, seed=5, vary=True), open(pp, "wb"))
    outs = {}
    for tag, path, extra in (("twin", twin, []), ("host", q, ["--weight_cache", "host"]), ("stream", q, ["--weight_cache", "stream"])):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--model_path", path, "--prompt_pickle", pp,
                            "--output_file", str(d / f"{tag}.pkl"), "--num_gen_token", "2", "--metrics_json",
                            str(d / f"{tag}.json")] + extra, cwd=str(d), env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        outs[tag] = open(d / f"{tag}.pkl", "rb").read()
    assert outs["host"] == outs["twin"] == outs["stream"]
    m, mt = json.load(open(d / "stream.json")), json.load(open(d / "twin.json"))
    assert m["mxfp4_tensors"] == 14 and m["int4_tensors"] == 0 and mt["mxfp4_tensors"] == 0
    moved = sum(v.numel() * v.element_size() for n in cfg.layer_names() for v in load_file(layer_file(q, n)).values())
    assert m["weight_file_bytes"] == moved < mt["weight_file_bytes"]


# -------------------------------------------------------------------- refusals
N = "model.layers.0.input_layernorm.weight"
U8 = torch.uint8
# tensors put into layer 0 of the tiny preset (q_proj is [256, 256]: bytes [256, 128], scales [256, 8]) -> the name refused
REFUSED = {
    "packed_shape": ({Q: torch.zeros(256, 127, dtype=U8)}, Q),
    "packed_flat": ({Q: torch.zeros(256 * 128, 1, dtype=U8)}, Q),
    "scale_dtype": ({Q + "_scale": torch.ones(256, 8, dtype=torch.float16)}, Q),
    "scale_shape": ({Q + "_scale": torch.zeros(256, 16, dtype=U8)}, Q),
    "scale_inv": ({Q + "_scale_inv": torch.ones(256, 1)}, Q),
    "zero_point": ({Q + "_zero_point": torch.zeros(256, 8, dtype=U8)}, Q),
    "input_scale": ({Q[:-len(".weight")] + ".input_scale": torch.ones(1)}, Q),
    "not_2d": ({N: torch.zeros(1, 128, dtype=U8), N + "_scale": torch.zeros(1, 8, dtype=U8)}, N),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_refused_mxfp4_tensors(tmp_path, case):
    cfg, d = preset("tiny"), str(tmp_path / "m")
    write_synthetic_checkpoint(cfg, d, seed=1, std=0.05, quantize="mxfp4")
    p = layer_file(d, "model.layers.0")
    tensors, name = REFUSED[case]
    save_file({**load_file(p), **tensors}, p)
    with pytest.raises(TypeError, match=name):
        LayerPlan(cfg, "model.layers.0", p)
    with pytest.raises(TypeError, match=name):
        pack_layer(cfg, "model.layers.0", load_file(p))
    # in % 32 != 0 (no preset has such a projection: the check itself)
    infos = {Q: types.SimpleNamespace(dtype=U8, shape=(8, 24)), Q + "_scale": types.SimpleNamespace(dtype=U8, shape=(8, 1))}
    with pytest.raises(TypeError, match="q_proj.weight.*32"):
        mxfp4.check_entry(Q, infos, (8, 48))
