"""``--score_mode classify`` without a GPU: the definition on a known answer, the converter's
``score.safetensors``, every refusal, the CLI's output file, and HF's classification classes
(within the 2e-3 of tests/test_engine_cpu.py::test_causal_prefix_matches_hf_transformers, which is
absolute on probabilities: the comparison runs on softmax outputs)."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from flexible_llm_sharding_amd import classify
from flexible_llm_sharding_amd.classify import ClassifyParams, check_head, layer_names, reference
from flexible_llm_sharding_amd.config import ModelConfig, preset
from flexible_llm_sharding_amd.engine import ShardedRunner
from flexible_llm_sharding_amd.runtime.stream import FileLayerSource
from flexible_llm_sharding_amd.utils.cli import parse_args
from flexible_llm_sharding_amd.utils.layer_format import split_into_layers
from flexible_llm_sharding_amd.utils.safetensors_io import load_file, save_file
from flexible_llm_sharding_amd.utils.synthetic import synthetic_layer_state_dict, write_synthetic_checkpoint
from flexible_llm_sharding_amd.utils.tokenizer import load_tokenizer, tokenize_prompts, write_synthetic_tokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL_HF = 2e-3
ATOL_ORACLE = 1e-4        # tests/test_engine_cpu.py::test_engine_matches_oracle (fp32 runs that batch differently)
PROMPTS = [("wd we wf wg", ("wh wi", "wj")), ("wk wl", ("wm wn wo",))]


def test_reference_on_a_known_answer():
    y = np.array([[1, 2, 0, -1], [0, 0, 0, 0]], dtype=np.float16)
    w = np.array([[1, 1, 5, 1], [2, 0, 0, 3]], dtype=np.float32)
    assert reference(y, w, None, ClassifyParams("last", "none", 2)).tolist() == [[2, -1], [0, 0]]
    assert reference(y, w, [0.5, 1], ClassifyParams("last", "none", 2)).tolist() == [[2.5, 0], [0.5, 1]]
    assert reference(y, w, None, ClassifyParams("last", "sigmoid", 2))[1].tolist() == [0.5, 0.5]
    assert reference(y, w, None, ClassifyParams("last", "softmax", 2))[1].tolist() == [0.5, 0.5]
    cfg = preset("tiny")
    assert layer_names(cfg, "classify") == cfg.layer_names()[:-1] + ["score"]


@pytest.mark.parametrize("bare", [False, True])
def test_converter_writes_the_score_layer(tmp_path, bare):
    cfg = preset("tiny")
    sd = dict(classify.synthetic_head(cfg, 3, num_labels=3))
    for n in cfg.layer_names()[:-1]:
        sd.update({(k[len("model."):] if bare else k): v for k, v in synthetic_layer_state_dict(cfg, n, seed=2).items()})
    src, out = tmp_path / "src", tmp_path / "out"
    src.mkdir()
    cfg.save(str(src))
    save_file(sd, str(src / "model.safetensors"))
    assert sorted(split_into_layers(str(src), str(out), verbose=False)) == sorted(layer_names(cfg, "classify"))
    head = load_file(str(out / "score.safetensors"))
    assert sorted(head) == ["score.bias", "score.weight"] and torch.equal(head["score.weight"], sd["score.weight"])


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("classify_model"))
    write_synthetic_checkpoint(preset("tiny"), d, seed=1, std=0.15, score_labels=3)
    os.remove(os.path.join(d, "lm_head.safetensors"))
    cfg = ModelConfig.from_pretrained(d)
    assert cfg.num_labels == 3
    return d, cfg, load_tokenizer(d)


def _runner(model, **kw):
    d, cfg, tok = model
    return ShardedRunner(cfg, FileLayerSource(cfg, d, names=classify.pass_layer_names(cfg, "classify")), "cpu", tok,
                         score_mode="classify", **kw)


H = preset("tiny").hidden_size
BAD_HEADS = [
    ({"score.weight": torch.zeros(3, H, 1)}, ValueError, "score.weight"),
    ({"score.weight": torch.zeros(3, H + 1)}, ValueError, "score.weight"),
    ({"score.weight": torch.zeros(2, H)}, ValueError, "num_labels"),
    ({"score.weight": torch.zeros(3, H), "score.bias": torch.zeros(2)}, ValueError, "score.bias"),
    ({"score.weight": torch.full((3, H), float("inf"))}, ValueError, "score.weight"),
    ({"score.weight": torch.full((3, H), 1e6)}, ValueError, "score.weight"),          # inf once it is fp16
    ({"score.weight": torch.zeros(3, H), "score.bias": torch.full((3,), float("nan"))}, ValueError, "score.bias"),
    ({"score.weight": torch.zeros(3, H, dtype=torch.uint8), "score.weight_scale": torch.ones(3)}, TypeError, "score.weight"),
    ({"score.qweight": torch.zeros(3, H // 8, dtype=torch.int32)}, TypeError, "score.weight"),
    ({}, ValueError, "score.weight"),
]


@pytest.mark.parametrize("sd,exc,match", BAD_HEADS)
def test_a_bad_head_is_refused(model, sd, exc, match):
    with pytest.raises(exc, match=match):
        check_head(model[1], sd)


def test_label_count_and_missing_file_are_refused(model, tmp_path):
    d, cfg, tok = model
    plain = preset("tiny")                                      # no num_labels: L itself is checked
    for L in (0, 65):
        with pytest.raises(ValueError, match="1..64"):
            check_head(plain, {"score.weight": torch.zeros(L, H)})
    with pytest.raises(ValueError, match="softmax"):
        ShardedRunner(plain, FileLayerSource(cfg, d, names=classify.pass_layer_names(cfg, "classify")), "cpu", tok,
                      score_mode="classify", classify_activation="softmax",
                      classify_head=check_head(plain, {"score.weight": torch.zeros(1, H)}))
    write_synthetic_checkpoint(plain, str(tmp_path), seed=1)
    with pytest.raises(ValueError, match="score.safetensors"):
        ShardedRunner(plain, FileLayerSource(plain, str(tmp_path)), "cpu", tok, score_mode="classify")


@pytest.mark.parametrize("kw,flag", [({"hip_graphs": True}, "--hip_graphs"), ({"prefix_kv_cache": True}, "--prefix_kv_cache"),
                                     ({"suffix_kv_cache": True}, "--suffix_kv_cache"), ({"resume_dir": "ck"}, "--resume_dir"),
                                     ({"score_top_k": 4}, "--score_top_k"), ({"sampling": object()}, "--do_sample"),
                                     ({"embed_pooling": "mean"}, "--embed_pooling"), ({"classify_rows": "first"}, "--classify_rows"),
                                     ({"classify_activation": "tanh"}, "--classify_activation")])
def test_runner_refuses(model, kw, flag):
    with pytest.raises(ValueError, match=flag):
        _runner(model, **kw)
    with pytest.raises(ValueError, match="--classify_rows needs --score_mode classify"):
        ShardedRunner(model[1], FileLayerSource(model[1], model[0], names=model[1].layer_names()[:-1]), "cpu", model[2],
                      score_mode="embed", classify_rows="all")


@pytest.mark.parametrize("extra,flag", [(["--num_gen_token", "2"], "--num_gen_token"), (["--do_sample"], "--do_sample"),
                                        (["--top_k", "5"], "--do_sample"), (["--score_top_k", "4"], "--score_top_k"),
                                        (["--lookup_decoding", "2"], "--lookup_decoding"), (["--hip_graphs"], "--hip_graphs"),
                                        (["--prefix_kv_cache", "true"], "--prefix_kv_cache"),
                                        (["--suffix_kv_cache", "true"], "--suffix_kv_cache"), (["--resume_dir", "x"], "--resume_dir"),
                                        (["--embed_dim", "8"], "--embed_dim"), (["--embed_normalize", "false"], "--embed_normalize")])
def test_cli_refuses(extra, flag):
    base = ["--model_path", "m", "--prompt_pickle", "p.pkl", "--output_file", "o.pkl"]
    with pytest.raises(ValueError, match=flag):
        parse_args(base + ["--score_mode", "classify"] + extra)
    for stray in (["--classify_rows", "all"], ["--classify_activation", "sigmoid"]):
        with pytest.raises(ValueError, match=stray[0] + " needs --score_mode classify"):
            parse_args(base + stray)
    from flexible_llm_sharding_amd.api import build_runner
    from flexible_llm_sharding_amd.parallel.comm import Comm
    with pytest.raises(ValueError, match="model parallel"):
        build_runner(parse_args(base + ["--score_mode", "classify"]), preset("tiny"), "cpu", Comm(0, 2), None)


@pytest.mark.parametrize("rows", ["last", "all"])
def test_main_writes_the_logits(model, tmp_path, rows):
    d, cfg, tok = model
    pp, out, mj = tmp_path / "prompts.pkl", tmp_path / "out.pkl", tmp_path / "m.json"
    pickle.dump(PROMPTS, open(pp, "wb"))
    env = dict(os.environ, PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--model_path", d, "--prompt_pickle", str(pp),
                        "--output_file", str(out), "--score_mode", "classify", "--classify_rows", rows, "--metrics_json",
                        str(mj), "--num_batch", "2"], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    res = pickle.load(open(out, "rb"))
    assert {k: v for k, v in res.items() if k != "logits"} == {"rows": rows, "activation": "none", "num_labels": 3}
    lens = [[len(s) for s in tp.suffixes] for tp in tokenize_prompts(tok, PROMPTS, 4096)]
    want = _runner(model, classify_rows=rows)(PROMPTS)
    for o, q, ls in zip(res["logits"], want, lens):
        if rows == "last":
            assert o.dtype == np.float32 and o.shape == (len(ls), 3) and np.abs(o - q).max() <= ATOL_ORACLE
        else:
            assert [a.shape for a in o] == [(n, 3) for n in ls] and all(np.abs(a - b).max() <= ATOL_ORACLE for a, b in zip(o, q))
    assert pickle.load(open(tmp_path / "prompts_updated.pkl", "rb")) == PROMPTS
    m = json.load(open(mj))
    assert (m["score_mode"], m["classify_rows"], m["num_labels"]) == ("classify", rows, 3)


@pytest.mark.parametrize("cls,rows", [("LlamaForSequenceClassification", "last"), ("LlamaForTokenClassification", "all")])
def test_hf_classification_models(tmp_path, cls, rows):
    transformers = pytest.importorskip("transformers")
    cfg = preset("tiny")
    hf_cfg = transformers.LlamaConfig(
        hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size, num_attention_heads=cfg.num_attention_heads,
        num_key_value_heads=cfg.num_key_value_heads, num_hidden_layers=cfg.num_hidden_layers, vocab_size=cfg.vocab_size,
        rms_norm_eps=cfg.rms_norm_eps, rope_theta=cfg.rope_theta, max_position_embeddings=cfg.max_position_embeddings,
        tie_word_embeddings=False, num_labels=3)
    torch.manual_seed(0)
    hf = getattr(transformers, cls)(hf_cfg).float().eval()
    sd = {}
    for n in cfg.layer_names()[:-1]:
        sd.update(synthetic_layer_state_dict(cfg, n, seed=1, std=0.15, dtype=torch.float32))
    hf.model.load_state_dict({k[len("model."):]: v for k, v in sd.items()})
    with torch.no_grad():
        hf.score.weight.copy_((torch.randn(3, cfg.hidden_size) * cfg.hidden_size ** -0.5).half().float())
    src, out = str(tmp_path / "hf"), str(tmp_path / "layers")
    hf.save_pretrained(src)
    write_synthetic_tokenizer(src, cfg.vocab_size)
    assert "score" in split_into_layers(src, out, verbose=False)
    ours, tok = ModelConfig.from_pretrained(out), load_tokenizer(out)
    assert ours.num_labels == 3
    r = ShardedRunner(ours, FileLayerSource(ours, out, names=classify.pass_layer_names(ours, "classify")), "cpu", tok,
                      score_mode="classify", classify_rows=rows, classify_activation="softmax", prefix_attention="causal")
    for prompt in [(p, s[:1]) for p, s in PROMPTS]:
        tp = tokenize_prompts(tok, [prompt], 4096)[0]
        with torch.no_grad():
            logits = hf(torch.tensor([tp.prefix + tp.suffixes[0]])).logits[0]
        want = torch.softmax(logits if rows == "last" else logits[len(tp.prefix):], -1).numpy()
        got = r([prompt])[0]
        got = got if rows == "last" else got[0]
        assert got.shape == want.reshape(-1, 3).shape and np.abs(got - want.reshape(-1, 3)).max() <= ATOL_HF
