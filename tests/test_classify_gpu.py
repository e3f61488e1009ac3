"""``fls_classify_rows`` on an MI355X against ``classify.reference`` (float64), and the engine's
classify mode against the torch-CPU backend's run of the same checkpoint.

Kernel bound (``none``): 2 H 2^-24 sum_k |y_k w_k| + 2^-24 |b|, the fp32 accumulation bound with a
factor 2 for the MFMA's internal order; through the activation (Lipschitz 1/4 for sigmoid, 1 in the
max norm for softmax) plus 4 fp32 ulps of the result.  Engine bound: E = max |embed ``last`` rows, GPU
- CPU backend|, measured in the run (tests/test_embed_gpu.py's engine-vs-oracle error and its factor
2 for other rows): a logit errs by at most 2 E ||w_l||_1 plus the kernel bound.  Prefixes of 560
tokens keep every micro-batch above 512 rows, where the GEMMs are row-independent (ibid.)."""
import os
import pickle
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from flexible_llm_sharding_amd import _native  # noqa: E402
from flexible_llm_sharding_amd.api import run_all  # noqa: E402
from flexible_llm_sharding_amd.classify import ClassifyParams, pass_layer_names, reference  # noqa: E402
from flexible_llm_sharding_amd.config import ModelConfig, preset  # noqa: E402
from flexible_llm_sharding_amd.parallel.comm import Comm  # noqa: E402
from flexible_llm_sharding_amd.runtime.stream import FileLayerSource  # noqa: E402
from flexible_llm_sharding_amd.engine import ShardedRunner  # noqa: E402
from flexible_llm_sharding_amd.ops import get_ops  # noqa: E402
from flexible_llm_sharding_amd.runtime.weights import HostStore  # noqa: E402
from flexible_llm_sharding_amd.utils.safetensors_io import load_file  # noqa: E402
from flexible_llm_sharding_amd.utils.synthetic import write_synthetic_checkpoint  # noqa: E402
from flexible_llm_sharding_amd.utils.tokenizer import load_tokenizer, synthetic_word  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
U = 2.0 ** -24

# (rows, L, H, gather, wide stride, base offset in bytes, activation): every value of every axis,
# both load paths (H = 200, an odd stride or a 2-byte offset take the 2-byte loads), 1..4 label tiles
CASES = [
    (1, 1, 32, 0, 0, 0, "none"), (15, 2, 32, 1, 0, 0, "softmax"), (16, 16, 32, 0, 1, 0, "sigmoid"),
    (17, 17, 32, 1, 1, 0, "none"), (130, 64, 32, 0, 0, 2, "softmax"), (1, 2, 200, 1, 0, 0, "sigmoid"),
    (15, 16, 200, 0, 1, 0, "none"), (16, 17, 200, 1, 1, 2, "softmax"), (17, 64, 200, 0, 0, 0, "sigmoid"),
    (130, 1, 200, 1, 0, 0, "none"), (1, 16, 4128, 0, 0, 0, "softmax"), (15, 17, 4128, 1, 1, 0, "sigmoid"),
    (16, 64, 4128, 0, 0, 0, "none"), (17, 1, 4128, 1, 0, 0, "sigmoid"), (130, 2, 4128, 0, 1, 0, "none"),
    (1, 17, 4128, 0, 1, 2, "none"), (15, 64, 4128, 1, 0, 2, "none"), (16, 1, 4128, 0, 0, 0, "none"),
    (17, 2, 4128, 0, 0, 0, "softmax"), (130, 16, 4128, 1, 0, 0, "sigmoid"), (130, 17, 4128, 0, 0, 0, "softmax"),
    (130, 64, 4128, 1, 1, 0, "softmax"), (1, 64, 32, 1, 0, 0, "none"), (15, 1, 32, 0, 1, 2, "sigmoid"),
    (16, 2, 32, 1, 0, 0, "none"), (17, 16, 32, 0, 0, 0, "softmax"), (130, 17, 32, 1, 0, 0, "sigmoid"),
    (16, 16, 200, 0, 0, 0, "softmax"), (17, 17, 200, 1, 0, 2, "none"), (130, 64, 200, 0, 1, 0, "none"),
    (17, 33, 4128, 1, 0, 0, "softmax"), (16, 48, 200, 0, 0, 0, "none"),
]


def _inputs(rows, L, H, seed=0):
    g = np.random.default_rng(seed + 1000 * rows + 10 * L + H)
    y = g.standard_normal((rows, H)).astype(np.float16)
    w = (g.standard_normal((L, H)) / np.sqrt(H)).astype(np.float16)
    b = g.standard_normal(L).astype(np.float32)
    return y, w, b


def _place(y, gather, wide, offset):
    """y on the device as a [rows, H] view with the case's row stride and base offset, stored
    permuted with the index that undoes it when the case gathers."""
    rows, H = y.shape
    ld = H + ((3 if H % 8 else 8) if wide else 0)
    idx = None
    if gather:
        perm = np.random.default_rng(1).permutation(rows)
        stored = np.empty_like(y)
        stored[perm] = y
        y, idx = stored, torch.from_numpy(perm.astype(np.int32)).to(DEV)
    buf = torch.zeros(rows * ld + 16, dtype=torch.float16, device=DEV)
    view = buf[offset // 2:offset // 2 + rows * ld].view(rows, ld)[:, :H]
    view.copy_(torch.from_numpy(y).to(DEV))
    return view, idx


def _bound(y, w, b, act, ref):
    mag = np.abs(y.astype(np.float64)) @ np.abs(w.astype(np.float64)).T
    t = 2 * y.shape[1] * U * mag + U * np.abs(b.astype(np.float64))[None, :]
    ulps = 4 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    if act == "sigmoid":
        return t / 4 + ulps
    if act == "softmax":
        return t.max(axis=1, keepdims=True) + ulps
    return t


@pytest.mark.parametrize("rows,L,H,gather,wide,offset,act", CASES)
def test_classify_rows_matches_fp64(rows, L, H, gather, wide, offset, act):
    ops = get_ops(DEV)
    y, w, b = _inputs(rows, L, H)
    x, idx = _place(y, gather, wide, offset)
    guard = 64
    canvas = torch.full((rows * L + 2 * guard,), -7.25, dtype=torch.float32, device=DEV)
    out = canvas[guard:guard + rows * L].view(rows, L)
    got = ops.classify_rows(x, torch.from_numpy(w).to(DEV), torch.from_numpy(b).to(DEV), act, row_idx=idx, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    host = canvas.cpu().numpy()
    assert (host[:guard] == -7.25).all() and (host[guard + rows * L:] == -7.25).all()     # the canaries
    got = host[guard:guard + rows * L].reshape(rows, L).astype(np.float64)
    ref = reference(y, w, b, ClassifyParams("last", act, L))
    err, bound = np.abs(got - ref), _bound(y, w, b, act, ref)
    print(f"rows {rows} L {L} H {H} {act}: worst error / bound {float((err / bound).max()):.3g}")
    assert (err <= bound).all(), float((err / bound).max())


@pytest.mark.parametrize("L", [1, 17])
def test_a_rows_bits_depend_on_the_row_alone(L):
    """Row r alone, inside 130 rows, and at another position through the index: identical bits."""
    ops = get_ops(DEV)
    y, w, b = _inputs(130, L, 4128, seed=3)
    wd, bd = torch.from_numpy(w).to(DEV), torch.from_numpy(b).to(DEV)
    act = "sigmoid" if L == 1 else "softmax"
    x = torch.from_numpy(y).to(DEV)
    full = ops.classify_rows(x, wd, bd, act)
    for r in (0, 15, 16, 77, 129):
        alone = ops.classify_rows(x[r:r + 1], wd, bd, act)
        assert torch.equal(alone.view(torch.int32), full[r:r + 1].view(torch.int32)), r
    perm = torch.from_numpy(np.random.default_rng(2).permutation(130).astype(np.int32)).to(DEV)
    moved = ops.classify_rows(x, wd, bd, act, row_idx=perm)
    assert torch.equal(moved.view(torch.int32), full[perm.long()].view(torch.int32))
    # the 2-byte-load path (a base 2 bytes off) computes the same bits as the 16-byte one
    xs, _ = _place(y, 0, 0, 2)
    assert torch.equal(ops.classify_rows(xs, wd, bd, act).view(torch.int32), full.view(torch.int32))


def test_bad_arguments_are_refused():
    k = _native.kernels()
    x = torch.zeros(4, 64, dtype=torch.float16, device=DEV)
    w = torch.zeros(2, 64, dtype=torch.float16, device=DEV)
    out = torch.zeros(4, 2, dtype=torch.float32, device=DEV)
    good = dict(x=x.data_ptr(), ld=64, idx=None, rows=4, H=64, w=w.data_ptr(), L=2, b=None, act=0, out=out.data_ptr())

    def call(**kw):
        return k.fls_classify_rows(*dict(good, **kw).values(), None)
    assert call() == 0
    assert call(rows=0, x=None) == 0                       # nothing to do: no launch, no check
    for kw in (dict(x=None), dict(w=None), dict(out=None), dict(L=0), dict(L=65), dict(H=0), dict(act=3), dict(act=-1),
               dict(rows=-1), dict(ld=63)):
        assert call(**kw) != 0, kw
    torch.cuda.synchronize()
    ops = get_ops(DEV)
    with pytest.raises(ValueError, match="softmax"):
        ops.classify_rows(x, w[:1], None, "softmax")
    with pytest.raises(TypeError, match="w16"):
        ops.classify_rows(x, w[:, :32], None)


# ------------------------------------------------------------------ engine
SUFFIX_LENS = [1, 7, 16, 33, 40]
PREFIX = 560
LABELS = 3


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("classify_gpu_model"))
    cfg = preset("tiny", hidden_size=512, intermediate_size=1024)
    write_synthetic_checkpoint(cfg, d, seed=5, std=0.05, score_labels=LABELS)
    cfg = ModelConfig.from_pretrained(d)
    tok = load_tokenizer(d)
    rng = np.random.default_rng(17)

    def words(n):
        return " ".join(synthetic_word(int(i)) for i in rng.integers(3, cfg.vocab_size, n))

    prompts = [(words(PREFIX - 1), tuple(words(n) for n in SUFFIX_LENS)) for _ in range(3)]
    os.remove(os.path.join(d, "lm_head.safetensors"))          # the mode needs no LM head
    names = pass_layer_names(cfg, "classify")
    store = HostStore.from_source(FileLayerSource(cfg, d, names=names), names=names)
    runs = {}

    def run(device, mode="classify", **kw):
        key = (str(device), mode, tuple(sorted(kw.items())))
        if key not in runs:
            r = ShardedRunner(cfg, store, device, tok, score_mode=mode, **kw)
            runs[key] = (r(prompts), r.score_d2h_bytes)
            r.close()
        return runs[key]
    return d, cfg, tok, prompts, store, run


@pytest.mark.parametrize("rows", ["last", "all"])
def test_engine_matches_the_cpu_backend(model, rows):
    d, cfg, tok, prompts, store, run = model
    E = max(float(np.abs(a - b).max()) for a, b in zip(run(DEV, "embed", embed_normalize=False)[0],
                                                       run("cpu", "embed", embed_normalize=False)[0]))
    head = load_file(os.path.join(d, "score.safetensors"))
    w, b = head["score.weight"].numpy().astype(np.float64), head["score.bias"].float().numpy().astype(np.float64)
    # the kernel bound with sum_k |y_k w_k| <= ||y||_2 ||w_l||_2 and ||y||_2 <= sqrt(H) max |norm weight|
    # (y = x / rms(x) * g, and ||x / rms(x)||_2 = sqrt(H))
    gmax = float(load_file(os.path.join(d, "model.norm.safetensors"))["model.norm.weight"].float().abs().max())
    H = cfg.hidden_size
    bound = (2 * E * np.abs(w).sum(axis=1) + 2 * H * U * np.sqrt(H) * gmax * np.linalg.norm(w, axis=1) + U * np.abs(b))
    (got, d2h), (want, _) = run(DEV, classify_rows=rows), run("cpu", classify_rows=rows)
    n_rows = 0
    for g, q in zip(got, want):
        g, q = (g, q) if rows == "all" else ([g], [q])
        assert [a.shape[0] for a in g] == (SUFFIX_LENS if rows == "all" else [len(SUFFIX_LENS)])
        assert all(a.shape == (c.shape[0], LABELS) for a, c in zip(g, q))
        for a, c in zip(g, q):
            assert a.dtype == np.float32 and (np.abs(a.astype(np.float64) - c) <= bound[None, :]).all()
            n_rows += a.shape[0]
    print(f"E {E:.3g}, bound {bound}")
    assert d2h == 4 * LABELS * n_rows                           # only the [*, L] floats cross to the host


def test_last_is_the_same_in_one_and_two_batches(model):
    d, cfg, tok, prompts, store, run = model
    one = run(DEV, classify_rows="last")[0]
    r = ShardedRunner(cfg, store, DEV, tok, score_mode="classify")
    two = run_all(SimpleNamespace(data_parallel=False, num_batch=2), r, Comm(0, 1), prompts)
    r.close()
    assert len(two) == 3 and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(one, two))


_WORKER = r"""
import pickle, sys, numpy as np, torch
sys.path.insert(0, {root!r})
from flexible_llm_sharding_amd.classify import pass_layer_names
from flexible_llm_sharding_amd.config import ModelConfig
from flexible_llm_sharding_amd.engine import ShardedRunner
from flexible_llm_sharding_amd.runtime.stream import FileLayerSource
from flexible_llm_sharding_amd.runtime.weights import HostStore
from flexible_llm_sharding_amd.utils.tokenizer import load_tokenizer
cfg, tok = ModelConfig.from_pretrained({path!r}), load_tokenizer({path!r})
names = pass_layer_names(cfg, "classify")
store = HostStore.from_source(FileLayerSource(cfg, {path!r}, names=names), names=names)
r = ShardedRunner(cfg, store, torch.device("cuda", 0), tok, max_vram_gb=1.5, score_mode="classify",
                  classify_activation="softmax")
out = r(pickle.load(open({prompts!r}, "rb")))
assert r.vram_plan["estimated_peak_bytes"] <= 1.5e9
np.save({out!r}, np.concatenate(out))
r.close()
"""


def test_under_a_vram_cap(model, tmp_path):
    """--max_vram_gb 1.5 (a fresh process: the allocator limit is process-wide): the uncapped bits."""
    d, cfg, tok, prompts, store, run = model
    want = np.concatenate(run(DEV, classify_activation="softmax")[0])
    pp, out = str(tmp_path / "prompts.pkl"), str(tmp_path / "capped.npy")
    pickle.dump(prompts, open(pp, "wb"))
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info(0)                   # this process's own use is not the worker's
    p = subprocess.run([sys.executable, "-c", _WORKER.format(root=ROOT, path=d, prompts=pp, out=out)],
                       capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, FLS_VRAM_SHARED_GB=str((total - free) / 1e9)))
    assert p.returncode == 0, p.stderr[-3000:]
    assert np.array_equal(np.load(out).view(np.uint32), want.view(np.uint32))
