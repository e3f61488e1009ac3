"""Pooled embeddings on an MI355X: the ``fls_pool_rows`` kernel against float64 on identical
fp16 rows, its row-exactness, and the engine's embed mode against the next-token mode (bitwise),
the fp32 CPU oracle, a VRAM cap, a micro-batch split, streamed weights and a model directory
without a head.

Kernel bound (tests/embed_ref.py): tau = 8 x the error of a float32 emulation of the kernel's
documented summation order, per group of cases, from the CPU alone: 4.9e-7 for unnormalised means
of values of order 1, 3.3e-7 for their normalised form, 7.5e-3 for means of rows of +-65504
(float32 spacing at 65504 is 2^-8 = 3.9e-3), 5.9e-8 for those normalised.
GPU error observed on an MI355X (``test_pool_rows_matches_fp64`` prints it per case): in all 40
cases exactly the emulation's own error — 1.4e-11 to 6.2e-8 (unit, raw), 0 to 4.1e-8 (unit,
normalised), 9.3e-4 (+-65504, raw), 7.4e-9 (+-65504, normalised).

Engine shapes.  The tiny model of tests/test_loglik_gpu.py, 3 prompts x 5 suffixes of 1, 7, 16, 33
and 40 tokens.  The prefixes hold 560 tokens, so that every micro-batch of every run — the whole
call and each third of it — has more than 512 rows: in the default (not row-exact) mode the GEMMs of
at most 512 rows split K by a rule that depends on the row count (split-K, skinny), and only the
tile kernels above that are row-independent (engine.py "exact K/V reuse"; --exact_reuse's help says
the same of the small-M kernels).  The bitwise comparisons of runs that split the call differently
therefore hold for calls of this size, as they do in tests/test_vram_gpu.py.

Engine bound: E_last = max |e_gpu - e_oracle| of the ``last`` pooling, unnormalised, D = H — which
test (a) shows to be the parent commit's final-norm rows bit for bit, so E_last is the parent
path's error — is measured in the run and printed (observed on an MI355X: 3.51e-3, on rows whose
entries reach about 4; ``mean`` came to at most 0.5 of its bound, reached by the one-token suffixes,
whose mean is their last row, normalised outputs to at most 0.25 of theirs); ``mean`` must stay within 2 E_last (a mean of
rows cannot err more than its worst row; the factor 2 because it runs over other rows than the
measured ones) and normalised outputs within 2 (2 E_last) / ||e_oracle|| (the bound of
|| a/||a|| - b/||b|| ||).
"""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import embed_ref as er  # noqa: E402

from flexible_llm_sharding_amd.config import preset  # noqa: E402
from flexible_llm_sharding_amd.embed import layer_names  # noqa: E402
from flexible_llm_sharding_amd.engine import ShardedRunner  # noqa: E402
from flexible_llm_sharding_amd.models.reference import reference_embeddings  # noqa: E402
from flexible_llm_sharding_amd.ops import get_ops  # noqa: E402
from flexible_llm_sharding_amd.runtime.stream import FileLayerSource  # noqa: E402
from flexible_llm_sharding_amd.runtime.weights import HostStore  # noqa: E402
from flexible_llm_sharding_amd.utils.synthetic import load_full_state_dict, write_synthetic_checkpoint  # noqa: E402
from flexible_llm_sharding_amd.utils.tokenizer import load_tokenizer, synthetic_word, tokenize_prompts  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)

# ------------------------------------------------------------------ kernel
CASES = er.kernel_cases()
TAU = er.group_tau(CASES)


def _on_gpu(case: er.PoolCase, rows=None):
    """(x view [n, H] on the device with the case's row stride and base offset, row_idx or None)
    for ``rows`` of the case (default: all), stored permuted when the case gathers."""
    x = case.x if rows is None else case.x[rows]
    n, H = x.shape
    ld = case.ld or H
    idx = None
    if case.gather:
        perm = np.random.default_rng(1).permutation(n)
        stored = np.empty_like(x)
        stored[perm] = x
        x, idx = stored, torch.from_numpy(perm.astype(np.int32)).to(DEV)
    buf = torch.zeros(max(n, 1) * ld + case.offset + 8, dtype=torch.float16, device=DEV)
    assert buf.data_ptr() % 256 == 0
    view = buf[case.offset:case.offset + n * ld].view(n, ld)[:, :H]
    view.copy_(torch.from_numpy(np.ascontiguousarray(x)).to(DEV))
    return view, idx


def _run(case: er.PoolCase, x=None, idx=None, seg_start=None) -> np.ndarray:
    ops = get_ops(DEV)
    if x is None:
        x, idx = _on_gpu(case)
    ss = torch.from_numpy(case.seg_start if seg_start is None else seg_start).to(DEV)
    out = ops.pool_rows(x, ss, case.D, case.normalize, row_idx=idx)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_pool_rows_matches_fp64(case):
    got = _run(case)
    assert got.dtype == np.float32 and got.shape == (len(case.lens), case.D) and np.isfinite(got).all()
    err = float(np.abs(got.astype(np.float64) - case.ref()).max())
    print(f"{case.name}: gpu err {err:.3g} emulation err {case.emu_err():.3g} tau {TAU[case.group]:.3g}")
    assert err <= TAU[case.group], (case.name, err, TAU[case.group])
    for i, n in enumerate(case.lens):
        if n == 0:
            assert not got[i].any(), case.name            # an empty segment: zeros


@pytest.mark.parametrize("case", [c for c in CASES if c.name.startswith(("ragged_H520", "ragged_H4096", "edges", "big"))],
                         ids=lambda c: c.name)
def test_pool_rows_is_row_exact(case):
    """Bitwise: every segment launched alone equals the joint launch; gathered rows equal
    contiguous ones; two runs of the same launch are equal."""
    x, idx = _on_gpu(case)
    joint = _run(case, x, idx)
    assert np.array_equal(_run(case, x, idx).view(np.uint32), joint.view(np.uint32))
    ss = case.seg_start
    for i, n in enumerate(case.lens):
        xi, ii = _on_gpu(case, rows=np.arange(ss[i], ss[i + 1]))
        alone = _run(case, xi, ii, seg_start=np.asarray([0, n], dtype=np.int32))
        assert np.array_equal(alone.view(np.uint32), joint[i:i + 1].view(np.uint32)), (case.name, i)
    # the other storage: contiguous for a gathering case, gathered for a contiguous one
    import dataclasses
    other = dataclasses.replace(case, gather=not case.gather, _cache={})
    assert np.array_equal(_run(other).view(np.uint32), joint.view(np.uint32)), case.name


@pytest.mark.parametrize("H", [64, 520, 4096, 8192])
def test_one_row_segments_are_the_rmsnorm_rows(H):
    """n = 1, normalise off, D = H: float32(ops.rmsnorm(x, w, eps)) bit for bit."""
    ops = get_ops(DEV)
    g = torch.Generator(device="cpu").manual_seed(H)
    x = (torch.randn(37, H, generator=g) * 2).to(torch.float16).to(DEV)
    x[3, :8] = -0.0                                 # (a lone row keeps its signed zeros)
    w = (1 + 0.1 * torch.randn(H, generator=g)).to(torch.float16).to(DEV)
    y = ops.rmsnorm(x, w, 1e-5)
    ss = torch.arange(38, dtype=torch.int32, device=DEV)
    got = ops.pool_rows(y, ss, 0, False)
    assert torch.equal(got.view(torch.int32), y.float().view(torch.int32))
    idx = torch.randperm(37, generator=g).to(torch.int32).to(DEV)
    got = ops.pool_rows(ops.rmsnorm(x, w, 1e-5), ss, 0, False, row_idx=idx)
    assert torch.equal(got.view(torch.int32), y.float()[idx.long()].view(torch.int32))


def test_pool_rows_refuses_bad_arguments():
    ops = get_ops(DEV)
    x = torch.zeros(4, 64, dtype=torch.float16, device=DEV)
    ss = torch.tensor([0, 4], dtype=torch.int32, device=DEV)
    for d in (-1, 65):
        with pytest.raises(ValueError, match="dim"):
            ops.pool_rows(x, ss, d)
    with pytest.raises(TypeError):
        ops.pool_rows(x.float(), ss)
    with pytest.raises(TypeError, match="seg_start"):
        ops.pool_rows(x, ss.long())
    # a row list that runs past the rows is cut off, an index outside them clamped: nothing is read out of range
    far = torch.tensor([0, 9], dtype=torch.int32, device=DEV)
    assert torch.equal(ops.pool_rows(x, far, 0, False), torch.zeros(1, 64, device=DEV))
    bad = torch.tensor([-5, 100], dtype=torch.int32, device=DEV)
    assert torch.equal(ops.pool_rows(x, torch.tensor([0, 2], dtype=torch.int32, device=DEV), 0, False, row_idx=bad),
                       torch.zeros(1, 64, device=DEV))


# ------------------------------------------------------------------ engine
SUFFIX_LENS = [1, 7, 16, 33, 40]
PREFIX = 560


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("embed_gpu_model"))
    cfg = preset("tiny", hidden_size=512, intermediate_size=1024)
    assert cfg.head_dim == 128 and cfg.num_attention_heads // cfg.num_key_value_heads == 2
    write_synthetic_checkpoint(cfg, d, seed=5, std=0.05)
    tok = load_tokenizer(d)
    rng = np.random.default_rng(17)

    def words(n):
        return " ".join(synthetic_word(int(i)) for i in rng.integers(3, cfg.vocab_size, n))

    prompts = [(words(PREFIX - 1), tuple(words(L) for L in SUFFIX_LENS)) for _ in range(3)]
    tps = tokenize_prompts(tok, prompts, 4096)
    assert [[len(u) for u in tp.suffixes] for tp in tps] == [SUFFIX_LENS] * 3 and all(len(tp.prefix) == PREFIX for tp in tps)
    sd = load_full_state_dict(cfg, d)
    state = {"store": HostStore.from_model_path(cfg, d), "runs": {}, "oracle": {}}
    return d, cfg, tok, prompts, sd, state


def _embed(model, pooling, normalize=False, dim=0, **kw):
    """The embeddings of one run, computed once per configuration and shared (never modified)."""
    d, cfg, tok, prompts, sd, state = model
    key = (pooling, normalize, dim, tuple(sorted(kw.items())))
    if key not in state["runs"]:
        r = ShardedRunner(cfg, state["store"], DEV, tok, score_mode="embed", embed_pooling=pooling,
                          embed_normalize=normalize, embed_dim=dim, **kw)
        out = r(prompts)
        state["runs"][key] = (out, int(r.stats["micro_batches"]), r.score_d2h_bytes, list(r.names))
        r.close()
    return state["runs"][key]


def _oracle(model, pooling, normalize=False, dim=0):
    d, cfg, tok, prompts, sd, state = model
    key = (pooling, normalize, dim)
    if key not in state["oracle"]:
        state["oracle"][key] = reference_embeddings(cfg, sd, tok, prompts, pooling, dim, normalize)
    return state["oracle"][key]


def _e_last(model) -> float:
    out = _embed(model, "last")[0]
    return max(float(np.abs(o - q).max()) for o, q in zip(out, _oracle(model, "last")))


def test_last_rows_are_the_parents_hidden_states(model):
    """(a) ``last``, normalise off, D = H: the returned rows, cast to fp16 (exact: they are fp16
    values) and put through ``ops.lm_head_softmax`` with the checkpoint's head, are the next-token
    run's scores bit for bit."""
    d, cfg, tok, prompts, sd, state = model
    out, mb, d2h, names = _embed(model, "last")
    assert mb == 1 and names[-1] == "model.norm" and d2h == 4 * cfg.hidden_size * 15
    nt = ShardedRunner(cfg, state["store"], DEV, tok)
    scores = nt(prompts)
    ops = get_ops(DEV)
    head = sd["lm_head.weight"].to(torch.float16).to(DEV)
    rows = np.concatenate(out)
    assert rows.dtype == np.float32 and np.array_equal(rows.astype(np.float16).astype(np.float32), rows)
    probs = ops.lm_head_softmax(torch.from_numpy(rows.astype(np.float16)).to(DEV), head,
                                logits_scaling=cfg.logits_scaling).cpu().numpy()
    want = np.concatenate([s[:, 0] for s in scores])
    assert want.dtype == np.float16 and np.array_equal(probs.view(np.uint16), want.view(np.uint16))
    nt.close()


@pytest.mark.parametrize("pooling,normalize,dim", [("mean", False, 0), ("mean", True, 0), ("last", True, 0),
                                                   ("mean", True, 100), ("last", False, 7)])
def test_engine_embed_within_the_parent_paths_error(model, pooling, normalize, dim):
    """(b) E_last is measured (and printed) on the rows test (a) pins to the parent's; ``mean``
    unnormalised within 2 E_last, normalised outputs within 2 (2 E_last) / ||e_oracle||."""
    d, cfg, tok, prompts, sd, state = model
    E = _e_last(model)
    out = _embed(model, pooling, normalize, dim)[0]
    ref = _oracle(model, pooling, normalize, dim)
    raw = _oracle(model, pooling, False, dim)
    D = dim or cfg.hidden_size
    other = _oracle(model, "mean" if pooling == "last" else "last", normalize, dim)
    worst = 0.0
    for o, q, u, q2 in zip(out, ref, raw, other):
        assert o.dtype == np.float32 and o.shape == (5, D) == q.shape
        err = np.abs(o - q).max(axis=1)
        bound = 2 * E / np.linalg.norm(u.astype(np.float64), axis=1) * 2 if normalize else np.full(5, 2 * E)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (pooling, normalize, dim, err, bound)
        # the oracle tells the two poolings of a suffix of several tokens apart by far more than the bound
        assert (np.abs(q - q2).max(axis=1)[1:] >= 20 * bound[1:]).all(), (np.abs(q - q2).max(axis=1), bound)
    print(f"E_last {E:.3g}; {pooling} normalize {normalize} D {D}: worst error / bound {worst:.3g}")


@pytest.mark.parametrize("pooling", ["last", "mean"])
def test_split_and_streamed_runs_are_bitwise_the_whole_run(model, pooling, tmp_path):
    """(c) a run forced into 3 micro-batches, a run with streamed weights and a run whose norm
    phase works in chunks of at most 50 rows equal the uncapped one-micro-batch run bit for bit."""
    d, cfg, tok, prompts, sd, state = model
    whole, mb, _, _ = _embed(model, pooling, True)
    assert mb == 1
    split, mb3, _, _ = _embed(model, pooling, True, token_budget=PREFIX + sum(SUFFIX_LENS))
    assert mb3 == 3
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(whole, split))
    r = ShardedRunner(cfg, FileLayerSource(cfg, d, names=layer_names(cfg, "embed")), DEV, tok, score_mode="embed",
                      embed_pooling=pooling)
    assert r._streamed_weights
    streamed = r(prompts)
    r.close()
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(whole, streamed))
    # the normed rows pooled 50 rows (of whole suffixes) at a time instead of all at once
    r = ShardedRunner(cfg, state["store"], DEV, tok, score_mode="embed", embed_pooling=pooling)
    r.ctx.pool_chunk = 50
    chunked = r(prompts)
    r.close()
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(whole, chunked))


_WORKER = r"""
import json, sys, threading, numpy as np, torch
sys.path.insert(0, {root!r})
from flexible_llm_sharding_amd.config import ModelConfig
from flexible_llm_sharding_amd.engine import ShardedRunner
from flexible_llm_sharding_amd.runtime.weights import HostStore
from flexible_llm_sharding_amd.utils.tokenizer import load_tokenizer
import pickle
cap = {cap}
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
cfg = ModelConfig.from_pretrained({path!r})
tok = load_tokenizer({path!r})
prompts = pickle.load(open({prompts!r}, "rb"))
peak, n = [0], [0]
stop = threading.Event()
def sample():
    torch.cuda.set_device(dev)
    while not stop.is_set():
        free, total = torch.cuda.mem_get_info(dev)
        peak[0] = max(peak[0], total - free)
        n[0] += 1
        stop.wait(0.002)
th = threading.Thread(target=sample, daemon=True)
th.start()
res, plans = {{}}, {{}}
for pooling in ("last", "mean"):
    store = HostStore.from_model_path(cfg, {path!r})
    r = ShardedRunner(cfg, store, dev, tok, max_vram_gb=cap, score_mode="embed", embed_pooling=pooling)
    for _ in range(2):
        out = r(prompts)
        torch.cuda.synchronize()
    res[pooling] = np.concatenate(out)
    plans[pooling] = dict(r.vram_plan, mb=r.stats["micro_batches"])
    r.close()
stop.set()
th.join()
np.savez({out!r}, **res)
print(json.dumps({{"peak": peak[0], "samples": n[0], "plans": plans}}))
"""


def test_embed_under_a_vram_cap(model, tmp_path):
    """(c) --max_vram_gb 1.5 (a fresh process: the allocator limit is process-wide): the sampled
    peak and the plan's estimate stay under the cap, and both poolings equal the uncapped run's
    bit for bit.  Observed on an MI355X: peak 0.39 GB, estimates 0.53 and 0.55 GB, one micro-batch."""
    import gc
    import pickle
    d, cfg, tok, prompts, sd, state = model
    want = {p: np.concatenate(_embed(model, p, True)[0]) for p in ("last", "mean")}
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info(0)
    shared = total - free                      # this process's own use: not the worker's
    cap = 1.5
    pp, out = str(tmp_path / "prompts.pkl"), str(tmp_path / "capped.npz")
    pickle.dump(prompts, open(pp, "wb"))
    code = _WORKER.format(root=ROOT, cap=cap, path=d, prompts=pp, out=out)
    env = dict(os.environ, FLS_VRAM_SHARED_GB=str(shared / 1e9))
    env.pop("FLS_SPLITK", None)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    meta = json.loads(p.stdout.strip().splitlines()[-1])
    print(f"capped run: peak {(meta['peak'] - shared) / 1e9:.3f} GB of {cap}, plans {meta['plans']}")
    assert meta["samples"] > 20, meta
    assert meta["peak"] - shared <= cap * 1e9, (meta, shared)
    got = np.load(out)
    for pooling in ("last", "mean"):
        assert meta["plans"][pooling]["estimated_peak_bytes"] <= cap * 1e9, meta
        assert np.array_equal(got[pooling].view(np.uint32), want[pooling].view(np.uint32)), pooling


def test_headless_directory_gives_the_same_bytes(model, tmp_path):
    """(d) the checkpoint with lm_head.safetensors removed: the same bytes in embed mode, and the
    default mode refuses it."""
    d, cfg, tok, prompts, sd, state = model
    hd = str(tmp_path / "headless")
    shutil.copytree(d, hd)
    os.remove(os.path.join(hd, "lm_head.safetensors"))
    names = layer_names(cfg, "embed")
    for pooling in ("last", "mean"):
        want = _embed(model, pooling, True)[0]
        store = HostStore.from_source(FileLayerSource(cfg, hd, names=names), names=names)
        r = ShardedRunner(cfg, store, DEV, tok, score_mode="embed", embed_pooling=pooling)
        got = r(prompts)
        r.close()
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(want, got)), pooling
    with pytest.raises(FileNotFoundError, match="missing layer files"):
        FileLayerSource(cfg, hd)
