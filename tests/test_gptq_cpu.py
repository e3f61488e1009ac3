"""GPTQ / AWQ checkpoints without a GPU: literal known answers for both layouts, the converter, the
layouts against the native host code, ``main.py`` on the torch backend against the twin, refusals."""
import ctypes
import json
import os
import pickle
import subprocess
import sys
import types

import pytest
import torch

from flexible_llm_sharding_amd import gptq
from flexible_llm_sharding_amd.config import preset
from flexible_llm_sharding_amd.models.layout import pack_layer
from flexible_llm_sharding_amd.runtime.stream import LayerPlan
from flexible_llm_sharding_amd.utils.layer_format import layer_file
from flexible_llm_sharding_amd.utils.safetensors_io import load_file, save_file
from flexible_llm_sharding_amd.utils.synthetic import synthetic_prompts, write_synthetic_checkpoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = "model.layers.0.self_attn.q_proj"
Q = S + ".weight"
I32 = torch.int32


def _i32(x: int) -> int:
    return x - (1 << 32) if x >> 31 else x


def test_known_answer_gptq():
    """out 8, in 32, one group.  Word [r, o] holds inputs 8r .. 8r + 7 of output o; zs = 15 is z = 0."""
    qweight, scales = torch.zeros(4, 8, dtype=I32), torch.ones(1, 8, dtype=torch.float16)
    qweight[0, 0], qweight[1, 3] = 0x76543210, _i32(0xF0000000)
    qzeros = torch.tensor([[0x0000600F]], dtype=I32)              # zs: o = 0 -> 15 (z = 0), o = 3 -> 6 (z = 7), others 0 (z = 1)
    scales[0, 0], scales[0, 3] = 0.5, 2.0
    w = gptq.dequantize(qweight, qzeros, scales)
    assert gptq.layout_of(qweight.shape, scales.shape) == "gptq"
    assert w[0, :9].tolist() == [0, .5, 1, 1.5, 2, 2.5, 3, 3.5, 0]
    assert w[3, 15] == 16 and w[3, 14] == -14 and w[1].eq(-1).all()


def test_known_answer_awq():
    """out 8, in 32, one group.  Nibble i of word [k, 0] is output P[i] = (0, 2, 4, 6, 1, 3, 5, 7)[i]; z = zs."""
    qweight, scales = torch.zeros(32, 1, dtype=I32), torch.ones(1, 8, dtype=torch.float16)
    qweight[5, 0] = 0x76543210
    qzeros = torch.tensor([[0x00000030]], dtype=I32)              # nibble 1 -> output 2: z = 3
    scales[0, 2] = 0.25
    w = gptq.dequantize(qweight, qzeros, scales)
    assert gptq.layout_of(qweight.shape, scales.shape) == "awq"
    assert w[:, 5].tolist() == [0, 4, -0.5, 5, 2, 6, 3, 7] and w[2, 4] == -0.75 and w[0, 4] == 0


@pytest.mark.parametrize("layout", gptq.LAYOUTS)
def test_round_trip_and_writer(layout):
    g = torch.Generator().manual_seed(1)
    u = torch.randint(0, 16, (24, 96), generator=g).to(torch.uint8)
    z = torch.randint(0, 16, (3, 24), generator=g).to(torch.uint8)
    assert torch.equal(gptq.unpack(gptq.pack(u, layout), layout), u)
    assert torch.equal(gptq.zero_points(gptq.pack_zero_points(z, layout), layout), z)
    w = torch.randn(24, 96, generator=g) * 0.05
    w[3] = 0                                                       # an all-zero group: s = 1
    w[5, :32] = w[5, :32].abs()                                    # one-sided groups keep 0 in range
    for group in (32, 0):
        qw, qz, s = gptq.quantize(w, layout, group)
        back = gptq.dequantize(qw, qz, s).to(torch.float64)
        step = s.t().to(torch.float64).repeat_interleave(96 // s.shape[0], 1)
        # half a step of rounding; the fp16 rounding of s shortens the 15 steps by at most 15 s 2^-11;
        # the result is rounded to fp16 (relative 2^-11 of at most 15 s)
        assert bool(((back - w.to(torch.float64)).abs() <= step * (0.5 + 30 * 2.0 ** -11)).all())
        assert back[3].eq(0).all()
    sd = gptq.quantize_state_dict({Q: w.half(), "model.norm.weight": torch.ones(4)}, layout, 32)
    assert (S + ".g_idx" in sd) == (layout == "gptq") and Q not in sd
    twin = gptq.dequantize_state_dict(sd)
    assert sorted(twin) == sorted([Q, "model.norm.weight"]) and twin[Q].shape == (24, 96)


def test_layouts_equal_native():
    from flexible_llm_sharding_amd import _native
    k, seg, inp = _native.kernels(), (ctypes.c_uint64 * 6)(), (ctypes.c_uint64 * 4)()
    assert k.fls_dequant_w4z_tail() == gptq.TAIL
    for out, inn, g in [(8, 32, 32), (72, 96, 32), (64, 128, 128), (136, 320, 64), (520, 1024, 1024), (8192, 28672, 128)]:
        n, lay = out * inn, gptq.region_layout(out * inn, g)
        assert k.fls_dequant_w4z_launches(n, g) == len(lay)
        for j, s in enumerate(lay):
            assert k.fls_dequant_w4z_segment(n, g, j, ctypes.addressof(seg)) == 0 and tuple(seg) == tuple(s)
        (q0, qn), (s0, sn), (z0, zn) = gptq.input_layout(out, inn, g)
        assert k.fls_repack_w4_input(out, inn, g, ctypes.addressof(inp)) == 0 and tuple(inp) == (q0, s0, z0, z0 + zn)
        assert q0 + qn <= s0 and s0 + sn <= z0 and z0 + zn <= lay[0].scale_off and gptq.landing_span(out, inn, g) == (0, z0 + zn)
    assert k.fls_dequant_w4z_launches(96, 64) < 0 and k.fls_repack_w4_input(12, 32, 32, ctypes.addressof(inp)) < 0


# --------------------------------------------------------- main.py
@pytest.mark.parametrize("layout,group", [("gptq", "128"), ("awq", "0")])
def test_main_equals_twin(tmp_path, layout, group):
    d, env = tmp_path, dict(os.environ, PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="1")
    q, twin, pp = str(d / "q"), str(d / "twin"), str(d / "prompts.pkl")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "prepare_weights.py"), "tiny", q, "--synthetic", "--quantize",
                        layout, "--int4_group", group, "--std", "0.05"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    gptq.write_twin(q, twin)
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
    assert m[f"{layout}_tensors"] == 14 and m["int4_tensors"] == 0 and mt["gptq_tensors"] == mt["awq_tensors"] == 0
    moved = sum(v.numel() * v.element_size() for n in cfg.layer_names() for k, v in load_file(layer_file(q, n)).items()
                if not k.endswith(".g_idx"))                      # (read when the file is planned, never copied)
    assert m["weight_file_bytes"] == moved < mt["weight_file_bytes"]


# -------------------------------------------------------------------- refusals
N = "model.layers.0.input_layernorm"
# tensors put into (None: taken out of) layer 0 of the tiny preset, GPTQ at g = 128 (q_proj is [256, 256]:
# qweight [32, 256], qzeros [2, 32], scales [2, 256], g_idx [256]) -> what the message names
REFUSED = {
    "act_order": ({S + ".g_idx": torch.arange(256, dtype=I32).flip(0) // 128}, "q_proj.weight.*desc_act"),
    "qweight_dtype": ({S + ".qweight": torch.zeros(32, 256, dtype=torch.float16)}, "q_proj.qweight has dtype"),
    "eight_bit_shape": ({S + ".qweight": torch.zeros(64, 256, dtype=I32)}, "q_proj.qweight has shape"),
    "scales_dtype": ({S + ".scales": torch.ones(2, 256)}, "q_proj.scales has dtype"),
    "group_16": ({S + ".scales": torch.ones(16, 256, dtype=torch.float16), S + ".qzeros": torch.zeros(16, 32, dtype=I32)},
                 "q_proj.scales has shape"),
    "qzeros_shape": ({S + ".qzeros": torch.zeros(2, 256, dtype=I32)}, "q_proj.qzeros has shape"),
    "no_qzeros": ({S + ".qzeros": None}, "q_proj.weight.*has no .*qzeros"),
    "stored_twice": ({Q: torch.zeros(256, 256, dtype=torch.float16)}, "q_proj.weight is stored twice"),
    "not_2d": ({N + ".weight": None, N + ".qweight": torch.zeros(32, 8, dtype=I32)}, "input_layernorm.weight.*2-D"),
}


@pytest.fixture(scope="module")
def gptq_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("gptq_cpu") / "m")
    write_synthetic_checkpoint(preset("tiny"), d, seed=1, std=0.05, quantize="gptq")
    return d


@pytest.mark.parametrize("case", list(REFUSED))
def test_refused_tensors(gptq_dir, tmp_path, case):
    cfg, p = preset("tiny"), str(tmp_path / "layer.safetensors")
    tensors, message = REFUSED[case]
    sd = {**load_file(layer_file(gptq_dir, "model.layers.0")), **tensors}
    save_file({k: v for k, v in sd.items() if v is not None}, p)
    with pytest.raises(TypeError, match=message):
        LayerPlan(cfg, "model.layers.0", p)
    with pytest.raises(TypeError, match=message):
        pack_layer(cfg, "model.layers.0", load_file(p))


@pytest.mark.parametrize("qc", [{"bits": 8}, {"bits": 4, "checkpoint_format": "gptq_v2"}, {"desc_act": True},
                                {"quant_method": "awq", "bits": 4, "version": "gemv"}])
def test_refused_quantization_config(tmp_path, qc):
    json.dump({"quantization_config": qc}, open(tmp_path / "config.json", "w"))
    with pytest.raises(TypeError, match="quantization_config"):
        gptq.check_quantization_config(str(tmp_path))
    json.dump({"quantization_config": {"quant_method": "awq", "bits": 4, "version": "GEMM"}}, open(tmp_path / "config.json", "w"))
    gptq.check_quantization_config(str(tmp_path))


def test_refused_shapes_and_flags(gptq_dir, tmp_path):
    from flexible_llm_sharding_amd import api, lora
    ns = types.SimpleNamespace
    for shape, qshape in (((12, 32), (4, 12)), ((8, 48), (6, 8))):        # out % 8, in % 32 (no preset has such a projection)
        infos = {S + ".qweight": ns(dtype=I32, shape=qshape), S + ".qzeros": ns(dtype=I32, shape=(1, 1)),
                 S + ".scales": ns(dtype=torch.float16, shape=(1, shape[0]))}
        with pytest.raises(TypeError, match="q_proj.weight.*out % 8"):
            gptq.check_entry(Q, infos, shape)
    cfg = preset("tiny")
    with pytest.raises(ValueError, match="dp_weight_shard true does not serve an GPTQ"):
        api.check_fp8_dp_shard(ns(model_path=gptq_dir, synthetic=None, score_mode="next_token"), cfg)
    adapter = lora.LoraAdapter.load(cfg, lora.write_synthetic_adapter(cfg, str(tmp_path / "adapter"), r=4, seed=1))
    with pytest.raises(TypeError, match="qweight.*fp16 twin"):
        lora.write_twin(gptq_dir, adapter, str(tmp_path / "merged"))
