"""Every attention kernel path against the fp64 reference, per (row, head), on inputs where the loss
of any one visible key moves its row by >= 4 tau (tests/attention_rows.py; the CPU side of the
argument is tests/test_attention_rows_cpu.py), in the forms production calls the kernel in: the
output aliasing the Q columns, an explicit scale, padding items, the pruned last layer's work items
over unwritten Q cells, and a K/V cache whose unreferenced rows hold NaN.

Every launch asserts: (1) row_err(y, ref64) <= tau on every queried (row, head), y finite there;
(2) the in-place form (out = the Q columns of qkv) is bitwise the out-of-place result and leaves
the K and V columns bitwise alone; (3) rows no work item queries keep a sentinel bit pattern in
`out`, their own Q cells when in place.

Measured on an MI355X when these tests were added (tau from the CPU, largest row_err from the GPU,
smallest min_single_key_effect of the cases run on the path; no step had to be added to
emulated_fp16):

    path                                              tau      row_err  one key
    attn_fwd       WPH 2, HPB 1 / 2 / 4               3.3e-3   4.9e-4   1.9e-2
    attn_fwd       WPH 4, HPB 1 / 2                   3.1e-3   3.9e-4   3.5e-2
    attn_fwd_pers  WPH 2, HPB 1 / 2 / 4               3.3e-3   4.9e-4   1.9e-2
    attn_fwd_pers  WPH 4, HPB 1 / 2                   3.1e-3   3.9e-4   3.5e-2
    attn_fwd       hd 96, WPH 2 / 4                   3.0e-3   4.1e-4   3.7e-2
    attn_fwd R2    WPH 2 (HPB 1 / 4), WPH 1 (4 / 8)   2.9e-3   3.4e-4   2.5e-2
    same, split-KV + attn_split_combine               2.9e-3   3.4e-4   2.5e-2
    attn_fwd R2    hd 96 (never splits)               2.5e-3   3.4e-4   4.6e-2
    attn_decode    unsplit                            2.9e-3   3.4e-4   2.5e-2
    attn_decode    split-KV + attn_split_combine      2.9e-3   3.4e-4   2.5e-2
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import attention_rows as ar  # noqa: E402
from flexible_llm_sharding_amd.ops.hip_backend import HipOps  # noqa: E402
from flexible_llm_sharding_amd import _native  # noqa: E402

DEV = torch.device("cuda", 0)
SENTINEL = 0x5A5A        # fp16 bit pattern (207.25) no attention output of these inputs can take


@pytest.fixture(scope="module")
def ops():
    o = HipOps()
    assert _native.loaded_libraries().get("k"), "libfls_kernels.so not loaded"
    return o


def _bits(x):
    return x.contiguous().view(torch.int16)


def _check(ops, c, work, q_block, ref, queried, qkv=None, work2=None, tag=""):
    """One out-of-place and one in-place launch; assertions 1-3; -> the out-of-place output (CPU)."""
    m = c.b.device_tensors(DEV)
    qkv = c.qkv if qkv is None else qkv
    T, qs = qkv.shape[0], c.nh * c.hd
    kw = {"seg_lo": m["seg_lo"], "scale": c.scale, "q_block": q_block}
    if c.kv0 is not None:
        kw["kv0"] = c.kv0.to(DEV)
    if work2 is not None:
        kw.update(work2=work2, r2win=m["r2win"])
    q = qkv.to(DEV)
    out = torch.full((T, qs), SENTINEL, dtype=torch.int16, device=DEV).view(torch.float16)
    y = ops.attention(q, work, c.nh, c.nkv, c.hd, out=out, **kw)
    inplace = q.clone()
    ops.attention(inplace, work, c.nh, c.nkv, c.hd, out=inplace[:, :qs], **kw)
    torch.cuda.synchronize()
    y, inplace = y.cpu(), inplace.cpu()
    # 1: every queried (row, head) within tau of fp64
    assert bool(torch.isfinite(y[queried]).all())
    err = float(ar.row_err(y[queried], ref[queried]).max())
    print(f"ROWS {tag} hd={c.hd} group={c.nh // c.nkv} q_block={q_block} tau={c.tau:.3e} err={err:.3e} "
          f"min_effect={c.min_effect:.3e}")
    assert err <= c.tau, (tag, err, c.tau)
    # 2: in place == out of place, K and V columns untouched
    assert torch.equal(_bits(inplace[queried, :qs]), _bits(y[queried]))
    assert torch.equal(_bits(inplace[:, qs:]), _bits(qkv[:, qs:]))
    # 3: rows no item queries are not written
    assert bool((_bits(y[~queried]) == torch.tensor(SENTINEL, dtype=torch.int16)).all())
    assert torch.equal(_bits(inplace[~queried, :qs]), _bits(qkv[~queried, :qs]))
    return y


def _padded(work):
    return torch.cat([work, torch.zeros(3, 8, dtype=torch.int32, device=DEV)])     # padding items (q_len 0)


def _hpbs(c):
    """0 (by group size) and every heads-per-block value valid for the group (hd 96: always 1)."""
    if c.hd == 96:
        return [0]
    return [0] + [h for h in (1, 2, 4) if (c.nh // c.nkv) % h == 0 and h <= (4 if c.q_block == 64 else 2)]


def _full_pass(ops, c, work, ref, queried, qkv=None, tag=""):
    """Persistent kernel on and off x every heads-per-block value; bitwise equal across the latter."""
    old_p, old_h = ops.k.fls_attention_set_persistent(1), ops.k.fls_attention_set_hpb(0)
    try:
        for pers in (1, 0):
            ops.k.fls_attention_set_persistent(pers)
            ys = []
            for hpb in _hpbs(c):
                ops.k.fls_attention_set_hpb(hpb)
                ys.append(_check(ops, c, work, c.q_block, ref, queried, qkv=qkv,
                                 tag=f"{tag} pers={pers} hpb={hpb}"))
            for y in ys[1:]:
                assert torch.equal(_bits(y), _bits(ys[0]))
    finally:
        ops.k.fls_attention_set_persistent(old_p)
        ops.k.fls_attention_set_hpb(old_h)


_FULL = ar.full_cases() + [ar.prefix_1k_case()]


@pytest.mark.parametrize("args", [c[1] for c in _FULL], ids=[c[0] for c in _FULL])
def test_full_pass_rows(ops, args):
    """Full pass, bidirectional and causal prefixes, 64- and 128-row items, hd 64 / 96 / 128, with
    padding items: attn_fwd_pers and attn_fwd at every heads-per-block value."""
    c = ar.flat_case(*args)
    work = _padded(c.b.device_tensors(DEV)["work"])
    _full_pass(ops, c, work, c.ref, torch.ones(c.b.num_tokens, dtype=torch.bool), tag="full")


_KV0 = ar.kv0_cases()


@pytest.mark.parametrize("args", [c[1] for c in _KV0], ids=[c[0] for c in _KV0])
def test_prefix_from_cache_rows(ops, args):
    """Range 0 read from a prefix K/V cache whose unreferenced rows hold NaN == the full packed pass."""
    c = ar.flat_case(*args)
    assert len(c.nan_rows) and bool(torch.isnan(c.kv0[torch.from_numpy(c.nan_rows)]).all())
    work = _padded(c.b.device_tensors(DEV)["work"])
    _full_pass(ops, c, work, c.ref, torch.ones(c.b.num_tokens, dtype=torch.bool), tag="kv0")


def _pruned_inputs(c):
    """The pruned last layer's inputs: Q of the non-scored rows is unwritten memory (NaN here); the
    expected values come from the scored rows' own segments over those inputs."""
    qs = c.nh * c.hd
    scored = torch.zeros(c.b.num_tokens, dtype=torch.bool)
    scored[torch.from_numpy(c.b.last_idx).long()] = True
    qkv = c.qkv.clone()
    qkv[~scored, :qs] = float("nan")
    ref, queried = ar.ref64(qkv, c.b.last_segments, c.nh, c.nkv, c.hd, kv0=c.kv0, scale=c.scale)
    assert torch.equal(queried, scored) and bool(torch.isfinite(ref[scored]).all())
    assert float(ar.row_err(ref[scored], c.ref[scored]).max()) < 1e-12      # == the full pass on those rows
    return qkv, ref, scored


_PRUNED = ar.pruned_cases()


@pytest.mark.parametrize("args", [c[1] for c in _PRUNED], ids=[c[0] for c in _PRUNED])
def test_pruned_last_layer_rows(ops, args):
    """work_last (one single-row item per scored row; reused steps: work2_last + r2win) over a qkv
    whose non-scored Q cells are NaN: scored rows within tau, the others bitwise untouched, in place
    and out of place."""
    c = ar.flat_case(*args)
    qkv, ref, scored = _pruned_inputs(c)
    assert 0 < int(scored.sum()) < c.b.num_tokens or c.b.all_rows_scored
    m = c.b.device_tensors(DEV)
    if c.kind != "reuse":
        _full_pass(ops, c, m["work_last"], ref, scored, qkv=qkv, tag="pruned")
        return
    old = ops.k.fls_attention_set_split(1)
    try:
        for q_block in (64, 8):
            for split in (1, 0):
                ops.k.fls_attention_set_split(split)
                _check(ops, c, m["work_last"], q_block, ref, scored, qkv=qkv, work2=m["work2_last"],
                       tag=f"pruned-r2 split={split}")
    finally:
        ops.k.fls_attention_set_split(old)


_REUSE = [(cid, args, qb, split) for cid, args in ar.reuse_cases()
          for qb in ((8, 32) if "decode" in cid else (64, 32, 8))
          for split in ((1, 0) if "decode" in cid else (1, 0, 3))]


@pytest.mark.parametrize("args,q_block,split", [c[1:] for c in _REUSE],
                         ids=[f"{c[0]}-q{c[2]}-split{c[3]}" for c in _REUSE])
def test_suffix_rows_from_cache_rows(ops, args, q_block, split):
    """Range 2 (work2 / r2win / kv0): the kept rows of every suffix, and the new rows' own keys, read
    from a K/V cache whose unreferenced rows hold NaN == the full packed pass on the new rows.
    q_block 64 / 32 / 8: attn_fwd with 2 waves and 1 wave per head, attn_decode (hd 96 falls back);
    split 1 / 0 / 3: unsplit, by grid size, three slices (+ attn_split_combine)."""
    c = ar.flat_case(*args)
    assert len(c.nan_rows) and bool(torch.isnan(c.kv0[torch.from_numpy(c.nan_rows)]).all())
    m = c.b.device_tensors(DEV)
    assert q_block != 32 or int(c.b.work[:, 1].max()) <= 32
    old = ops.k.fls_attention_set_split(split)
    try:
        _check(ops, c, m["work"], q_block, c.ref, torch.ones(c.b.num_tokens, dtype=torch.bool),
               work2=m["work2"], tag=f"r2 split={split}")
    finally:
        ops.k.fls_attention_set_split(old)
