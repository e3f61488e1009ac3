"""Per-row attention checks: inputs, references and the error bound (a plain helper module).

The attention tests of test_kernels_gpu.py compare one global norm on ``randn`` inputs.  A masking
defect that touches a few rows is diluted below their limit, and with unit-variance scores many keys
carry less softmax weight than fp16 output rounding, so no limit could catch their loss.  Here the
softmax is flattened (scores scaled by 1/16) so that every visible key moves its row by far more
than the kernel's rounding, and every (row, head) is compared on its own.

* :func:`ref64` - dense fp64 attention per segment, masks from the ``Segment`` fields only;
* :func:`emulated_fp16` - the same with the arithmetic the kernel is documented to do;
* :func:`min_single_key_effect` - the smallest change the loss of one visible key makes to a row;
* ``mutations`` - references with a known masking defect, for the self-checks of the bound;
* :func:`flat_case` - packed prompts + flat fp16 Q/K/V in the layouts the kernel is called with.

The bound of a case is ``tau = 8 * max row_err(emulated_fp16, ref64)``, from the CPU alone; a case
is usable when ``min_single_key_effect >= 4 * tau``.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from flexible_llm_sharding_amd.runtime.batch import PackedBatch, pack_prompts
from flexible_llm_sharding_amd.utils.tokenizer import TokenizedPrompt

# the suite's ragged ~780-row prompt set (test_attention_shared_prefix / _128_row_items)
SUITE = ((70, (5, 64, 1)), (1, (3,)), (130, (65, 17, 129)), (200, (33, 64)))
# one 1,024-token prefix (16 key tiles per item) next to two short prompts: the persistent kernel
PREFIX_1K = ((70, (5, 64, 1)), (1, (3,)), (1024, (64,) * 5))
# generation-like: kept rows of each suffix come from the K/V cache (range 2)
GEN = ((70, (5, 80, 1)), (130, (65, 17)), (9, (3, 140)))
GEN_KEEP = ((3, 70, 0), (64, 5), (0, 139))
# decode step: one new row per suffix after 40 kept ones, 600-row prefixes
DECODE = ((600, (41,) * 5),) * 3
DECODE_KEEP = ((40,) * 5,) * 3

TAU_FACTOR = 8.0        # hardware exp2, fp32 summation order, deferred rescale, fp32 split-KV merge
SEPARATION = 4.0        # min_single_key_effect >= SEPARATION * tau


# --------------------------------------------------------------------------- dense problems
def _split(x: torch.Tensor, nh: int, nkv: int, hd: int):
    T = x.shape[0]
    qs, ks = nh * hd, nkv * hd
    return (x[:, :qs].reshape(T, nh, hd), x[:, qs:qs + ks].reshape(T, nkv, hd),
            x[:, qs + ks:qs + 2 * ks].reshape(T, nkv, hd))


def segment_keys(segments, cached: bool):
    """Per segment: the candidate key columns and the boolean visibility mask [q_len, n_keys],
    from the Segment fields alone.  Columns: ``rng`` (0 prefix, 2 kept suffix rows, 1 the segment's
    own rows, 3 the row in front of the segment when that is the previous suffix of the same
    prompt: never visible, the `seg_lo` mutation turns it on), ``idx`` (index inside the range),
    ``buf`` (1: the K/V cache, 0: the packed rows) and ``row`` (row of that buffer).
    ``sfx0``: first packed row of the run of suffixes (one prompt) the segment belongs to."""
    prev, sfx0 = None, 0
    for sg in segments:
        parts = [(0, sg.r0_start, sg.r0_len, 1 if cached else 0)]
        if getattr(sg, "r2_len", 0):
            parts.append((2, sg.r2_start, sg.r2_len, 1))
        follows = False
        if sg.r1_len:
            parts.append((1, sg.r1_start, sg.r1_len, 0))
            follows = (prev is not None and prev.r1_len > 0 and prev.r0_start == sg.r0_start
                       and prev.r0_len == sg.r0_len and prev.q_start + prev.q_len == sg.q_start
                       and sg.q_off == 0)
            if follows:
                parts.append((3, sg.r1_start - 1, 1, 0))
            else:
                sfx0 = sg.q_start - sg.q_off
        rng = np.concatenate([np.full(n, r) for r, _, n, _ in parts])
        idx = np.concatenate([np.arange(n) for _, _, n, _ in parts])
        buf = np.concatenate([np.full(n, b) for _, _, n, b in parts])
        row = np.concatenate([np.arange(s, s + n) for _, s, n, _ in parts])
        qi = (np.arange(sg.q_len) + sg.q_off)[:, None]
        mask = np.ones((sg.q_len, rng.shape[0]), dtype=bool)
        mask &= ~((rng == 1)[None, :] & (idx[None, :] > qi))                     # own rows: causal
        if sg.r0_causal:
            mask &= ~((rng == 0)[None, :] & (idx[None, :] > qi))
        mask &= ~(rng == 3)[None, :]
        yield sg, {"rng": rng, "idx": idx, "buf": buf, "row": row, "sfx0": sfx0}, mask
        prev = sg


def _attend(q, K, V, mask, scale, arith):
    """q [n, nh, hd], K / V [k, nh, hd], mask [n, k] -> (o [n, nh, hd], p [nh, n, k])."""
    m = torch.from_numpy(mask)[None]
    if arith == "f64":
        s = torch.einsum("qhd,khd->hqk", q, K) * scale
        s = s.masked_fill(~m, float("-inf"))
        p = torch.softmax(s, dim=-1)
        return torch.einsum("hqk,khd->qhd", p, V), p
    # the kernel's arithmetic: fp32 scores and running sums, P = exp(s - max) rounded to fp16 for
    # the P.V product, fp32 accumulation, fp16 output
    s = torch.einsum("qhd,khd->hqk", q, K)                       # raw scores, fp32
    s = s.masked_fill(~m, float("-inf"))
    mx = s.max(dim=-1, keepdim=True).values
    p = torch.exp((s - mx) * np.float32(scale))
    l = p.sum(dim=-1)                                            # [nh, n]
    o = torch.einsum("hqk,khd->qhd", p.half().float(), V) / l.t()[:, :, None]
    return o.half().double(), p


def _run(qkv, segments, nh, nkv, hd, kv0, scale, arith, edit=None, want_effect=False):
    dt = torch.float64 if arith == "f64" else torch.float32
    T = qkv.shape[0]
    q_all, k_all, v_all = _split(qkv.to(dt), nh, nkv, hd)
    bufs = [(k_all, v_all)]
    if kv0 is not None:
        ks = nkv * hd
        c = kv0.to(dt)
        bufs.append((c[:, :ks].reshape(-1, nkv, hd), c[:, ks:2 * ks].reshape(-1, nkv, hd)))
    rep = nh // nkv
    scale = hd ** -0.5 if scale is None else scale
    out = torch.zeros(T, nh, hd, dtype=torch.float64)
    queried = torch.zeros(T, dtype=torch.bool)
    touched = torch.zeros(T, dtype=torch.bool)
    effect = torch.full((T, nh), float("inf"), dtype=torch.float64)
    for sg, cols, mask in segment_keys(segments, kv0 is not None):
        if edit is not None:
            mask, hit = edit(sg, cols, mask)
            touched[sg.q_start:sg.q_start + sg.q_len] = torch.from_numpy(hit)
        buf, row = torch.from_numpy(cols["buf"]), torch.from_numpy(cols["row"])
        K = torch.empty(row.shape[0], nkv, hd, dtype=dt)
        V = torch.empty_like(K)
        for b, (kk, vv) in enumerate(bufs):
            sel = buf == b
            K[sel], V[sel] = kk[row[sel]], vv[row[sel]]
        live = mask.any(0)                      # never-visible columns may hold anything (NaN)
        K, V, mask = K[torch.from_numpy(live)], V[torch.from_numpy(live)], mask[:, live]
        K, V = K.repeat_interleave(rep, dim=1), V.repeat_interleave(rep, dim=1)
        q = q_all[sg.q_start:sg.q_start + sg.q_len]
        o, p = _attend(q, K, V, mask, scale, arith)
        out[sg.q_start:sg.q_start + sg.q_len] = o
        queried[sg.q_start:sg.q_start + sg.q_len] = True
        if want_effect:
            # removing key j: o' - o = p_j / (1 - p_j) * (o - v_j)
            on = (o * o).sum(-1).t()                                         # [nh, n]
            d2 = (V * V).sum(-1).t()[:, None, :] - 2 * torch.einsum("qhd,khd->hqk", o, V) + on[:, :, None]
            e = p / (1 - p) * d2.clamp_min(0).sqrt() / on.sqrt()[:, :, None]
            m = torch.from_numpy(mask)
            e = e.masked_fill(~m[None], float("inf")).min(dim=-1).values     # [nh, n]
            e = e.masked_fill(torch.from_numpy(mask.sum(1) <= 1)[None], float("inf"))
            effect[sg.q_start:sg.q_start + sg.q_len] = e.t()
    return out, queried, touched, effect


def ref64(qkv, segments, nh, nkv, hd, kv0=None, scale=None):
    """Dense fp64 attention over the segments: ([T, nh, hd] fp64, [T] bool row is queried)."""
    out, queried, _, _ = _run(qkv, segments, nh, nkv, hd, kv0, scale, "f64")
    return out, queried


def emulated_fp16(qkv, segments, nh, nkv, hd, kv0=None, scale=None):
    """The kernel's documented arithmetic (csrc/kernels/attention.hip header), no kernel code:
    fp32 scores and sums, exp(s - max) rounded to fp16 before P.V, fp32 accumulation, fp16 output."""
    out, queried, _, _ = _run(qkv, segments, nh, nkv, hd, kv0, scale, "emu")
    return out, queried


def row_err(y, r):
    """[T, nh]: ||y - r|| / ||r|| per (row, head) over hd, in fp64."""
    y, r = y.double().reshape(r.shape[0], r.shape[1], -1), r.double()
    return (y - r).norm(dim=-1) / r.norm(dim=-1)


def min_single_key_effect(qkv, segments, nh, nkv, hd, kv0=None, scale=None):
    """[T, nh]: for each (row, head) with more than one visible key the smallest relative change
    of its output when one visible key j is removed, p_j / (1 - p_j) * ||v_j - o|| / ||o||
    (inf for the other rows)."""
    return _run(qkv, segments, nh, nkv, hd, kv0, scale, "f64", want_effect=True)[3]


# --------------------------------------------------------------------------- mutations
def _keeps_a_key(mask, new):
    """Apply `new` only to rows that keep at least one visible key; -> (mask, rows changed)."""
    ok = new.any(1)
    new = np.where(ok[:, None], new, mask)
    return new, (new != mask).any(1)


def _mut_diag(edge):
    def edit(sg, c, mask):                   # suffix rows on a tile edge lose their diagonal key
        new = mask.copy()
        if sg.r1_len:
            for i in range(sg.q_len):
                if (sg.q_start + i - c["sfx0"]) % edge == edge - 1:
                    new[i, (c["rng"] == 1) & (c["idx"] == sg.q_off + i)] = False
        return _keeps_a_key(mask, new)
    return edit


def _mut_r0_last(sg, c, mask):               # the last key of a non-causal range 0 is dropped
    new = mask.copy()
    if sg.r0_len and not sg.r0_causal:
        new[:, (c["rng"] == 0) & (c["idx"] == sg.r0_len - 1)] = False
    return _keeps_a_key(mask, new)


def _mut_key0(sg, c, mask):                  # one row per segment (its last) loses its first key
    new = mask.copy()
    new[-1, int(np.argmax(mask[-1]))] = False
    return _keeps_a_key(mask, new)


def _mut_seg_lo(sg, c, mask):                # first row of a non-first suffix sees the row before it
    new = mask.copy()
    new[0, c["rng"] == 3] = True
    return _keeps_a_key(mask, new)


def _mut_r2win(sg, c, mask):                 # each row's window of its own suffix shifted by one row
    new = mask.copy()
    if sg.r1_len:
        own = (c["rng"] == 2) | (c["rng"] == 1)
        for i in range(sg.q_len):
            new[i, int(np.argmax(mask[i] & own))] = False
            new[i, (c["rng"] == 1) & (c["idx"] == sg.q_off + i + 1)] = True
    return _keeps_a_key(mask, new)


mutations = {
    "diag64": _mut_diag(64),        # (a)
    "diag128": _mut_diag(128),      # (a)
    "r0_last": _mut_r0_last,        # (b)
    "key0": _mut_key0,              # (c)
    "seg_lo": _mut_seg_lo,          # (d) full passes only (a reused step has no range 1)
    "r2win": _mut_r2win,            # (e) reused steps only
}


def mutated_ref(name, qkv, segments, nh, nkv, hd, kv0=None, scale=None, arith="f64"):
    """ref64 (arith "emu": emulated_fp16, a stand-in for a kernel) with the masking defect `name`:
    ([T, nh, hd], [T] bool rows whose mask changed)."""
    out, _, touched, _ = _run(qkv, segments, nh, nkv, hd, kv0, scale, arith, edit=mutations[name])
    return out, touched


# --------------------------------------------------------------------------- cases
@dataclass
class Case:
    """One attention problem in the layout the kernel is called with.  ``b`` / ``qkv`` / ``kv0`` /
    ``scale`` feed the kernel; ``full`` / ``full_qkv`` are the same prompts as one packed pass with
    no cache (the expected values), ``rows`` the packed rows of that pass the kernel computes."""
    nh: int
    nkv: int
    hd: int
    q_block: int
    kind: str                        # "full" | "kv0" | "reuse"
    b: PackedBatch
    qkv: torch.Tensor                # [T, (nh + 2 nkv) hd] fp16
    kv0: Optional[torch.Tensor]      # K/V cache, fp16; rows no range references hold NaN
    nan_rows: Optional[np.ndarray]   # those rows
    scale: Optional[float]
    full: PackedBatch
    full_qkv: torch.Tensor
    rows: torch.Tensor               # [T] int64

    @functools.cached_property
    def ref(self):
        """[T, nh, hd] fp64: ref64 of the full packed pass on the kernel's rows."""
        r, queried = ref64(self.full_qkv, self.full.segments, self.nh, self.nkv, self.hd, scale=self.scale)
        assert bool(queried.all())
        return r[self.rows]

    @functools.cached_property
    def tau(self) -> float:
        e, _ = emulated_fp16(self.full_qkv, self.full.segments, self.nh, self.nkv, self.hd, scale=self.scale)
        return TAU_FACTOR * float(row_err(e[self.rows], self.ref).max())

    @functools.cached_property
    def min_effect(self) -> float:
        e = min_single_key_effect(self.full_qkv, self.full.segments, self.nh, self.nkv, self.hd, scale=self.scale)
        return float(e[self.rows].min())

    def mutated(self, name, arith="f64"):
        """(mutated reference on the kernel's rows, [T] bool rows it touches)."""
        m, touched = mutated_ref(name, self.full_qkv, self.full.segments, self.nh, self.nkv, self.hd,
                                 scale=self.scale, arith=arith)
        return m[self.rows], touched[self.rows]

    def applicable(self, name) -> bool:
        return {"seg_lo": self.kind != "reuse", "r2win": self.kind == "reuse"}.get(name, True)


def _tps(prompts) -> List[TokenizedPrompt]:
    return [TokenizedPrompt(list(range(lp)), [list(range(l)) for l in ls], max(ls), [l - 1 for l in ls])
            for lp, ls in prompts]


GAP = 3     # rows of the K/V cache between the regions of two prompts that no range references


@functools.lru_cache(maxsize=None)
def flat_case(nh, nkv, hd, prompts, mode="bidirectional", q_block=64, seed=0, via="q", kind="full",
              keep=None) -> Case:
    """Packed prompts (``pack_prompts``) + randn fp16 Q/K/V with a flat softmax.  ``via``: "q" - the
    Q columns times 2^-4 (exact in fp16), default scale; "scale" - Q left alone and
    scale = hd^-0.5 / 16 passed explicitly; None - the suite's plain randn inputs.
    ``kind``: "full" - every row packed; "kv0" - prefixes read from a K/V cache (range 0);
    "reuse" - also the first ``keep[j][s]`` rows of every suffix (range 2), only the rows after
    them computed.  The cache has GAP unreferenced rows in front of every prompt's prefix and
    suffix regions and at its end, filled with NaN."""
    tps = _tps(prompts)
    ids = list(range(len(tps)))
    qs, kv = nh * hd, 2 * nkv * hd
    offs = rows = None
    if kind != "full":
        offs, t = [], 0
        for lp, _ in prompts:
            t += GAP
            offs.append(t)
            t += lp
        rows = []
        for _, ls in prompts:
            t += GAP
            rows.append([])
            for l in ls:
                rows[-1].append(t)
                t += l
        t += GAP
    full = pack_prompts(tps, ids, mode, prefix_offsets=offs, q_block=q_block,
                        suffix_rows=rows if kind == "reuse" else None)
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(full.num_tokens, qs + kv, generator=g).half()
    scale = None
    if via == "q":
        qkv[:, :qs] *= 2.0 ** -4
    elif via == "scale":
        scale = hd ** -0.5 / 16
    elif via is not None:
        raise ValueError(via)
    if kind == "full":
        return Case(nh, nkv, hd, q_block, kind, full, qkv, None, None, scale, full, qkv,
                    torch.arange(full.num_tokens))
    cache = torch.full((t, kv), float("nan"), dtype=torch.float16)
    cache[torch.from_numpy(full.pfx_dst).long()] = qkv[torch.from_numpy(full.pfx_src).long(), qs:]
    if kind == "reuse":
        cache[torch.from_numpy(full.sfx_dst).long()] = qkv[torch.from_numpy(full.sfx_src).long(), qs:]
    nan_rows = np.flatnonzero(torch.isnan(cache).any(1).numpy())
    if kind == "reuse":
        b = pack_prompts(tps, ids, mode, prefix_offsets=offs, kv_cached=True, q_block=q_block,
                         suffix_rows=rows, suffix_keep=[list(k) for k in keep])
        sel = []
        sfx = [sg for sg in full.segments if sg.r1_len]
        for sg, c in zip(sfx, [c for ks in keep for c in ks]):
            sel.extend(range(sg.q_start + c, sg.q_start + sg.q_len))
        sel = torch.tensor(sel)
    else:
        b = pack_prompts(tps, ids, mode, prefix_offsets=offs, kv_cached=True, q_block=q_block)
        sel = torch.from_numpy(np.setdiff1d(np.arange(full.num_tokens), full.pfx_src))
    assert sel.shape[0] == b.num_tokens
    return Case(nh, nkv, hd, q_block, kind, b, qkv[sel].contiguous(), cache, nan_rows, scale, full, qkv, sel)


# --------------------------------------------------------------------------- masks of the work items
def key_codes(buf, row):
    return np.asarray(buf, dtype=np.int64) * (1 << 32) + np.asarray(row, dtype=np.int64)


def segment_masks(segments, cached: bool, n_rows: int, packed_to_cache=None):
    """Per packed row the sorted codes (buffer, row) of the keys `segments` make visible (None:
    row not queried).  ``packed_to_cache`` maps packed rows whose K/V the cache also holds (a reused
    step captures its new rows before the attention runs) to their cache rows."""
    out = [None] * n_rows
    for sg, c, mask in segment_keys(segments, cached):
        buf, row = c["buf"].copy(), c["row"].copy()
        if packed_to_cache is not None:
            p = buf == 0
            buf[p], row[p] = 1, packed_to_cache[row[p]]
        codes = key_codes(buf, row)
        for i in range(sg.q_len):
            out[sg.q_start + i] = np.sort(codes[mask[i]])
    return out


def work_item_masks(b: PackedBatch, work, work2, n_rows: int, reuse: bool):
    """The same from the work items, through runtime.batch.visible_keys (the kernel's semantics)."""
    from flexible_llm_sharding_amd.runtime.batch import visible_keys
    out = [None] * n_rows
    queried = np.zeros(n_rows, dtype=bool)
    for it in work:
        queried[it[0]:it[0] + it[1]] = True
    for r in np.flatnonzero(queried):
        codes = []
        for rng, lo, hi in visible_keys(work, b.seg_lo, int(r), work2, b.r2win if reuse else None):
            in_cache = rng == 2 or (rng == 0 and b.kv_cached)
            codes.append(key_codes(np.full(hi - lo + 1, 1 if in_cache else 0), np.arange(lo, hi + 1)))
        out[r] = np.sort(np.concatenate(codes))
    return out


# --------------------------------------------------------------------------- the cases of both test files
def _geom_id(nh, nkv, hd):
    return f"{nh}-{nkv}-{hd}"


FULL_GEOMETRIES = [(64, (8, 2, 128)), (64, (4, 2, 64)), (64, (3, 3, 64)), (64, (6, 2, 128)), (64, (8, 1, 64)),
                   (128, (4, 4, 128)), (128, (4, 2, 64)), (128, (6, 2, 64)), (64, (4, 4, 96)), (128, (4, 4, 96))]
KV0_GEOMETRIES = [(8, 1, 128), (4, 2, 64), (4, 4, 96)]
REUSE_GEOMETRIES = [(8, 1, 128), (16, 2, 128), (8, 2, 64), (4, 4, 64), (4, 4, 96)]
PRUNED_GEOMETRIES = [(64, (8, 2, 128)), (128, (4, 2, 64)), (64, (4, 4, 96))]


def _via(i):
    return ("q", "scale")[i % 2]


def full_cases():
    """(id, flat_case arguments) of the full-pass cases: every geometry x both prefix modes."""
    out = []
    for i, (qb, (nh, nkv, hd)) in enumerate(FULL_GEOMETRIES):
        for j, mode in enumerate(("bidirectional", "causal")):
            out.append((f"{_geom_id(nh, nkv, hd)}-q{qb}-{mode}",
                        (nh, nkv, hd, SUITE, mode, qb, 100 + i, _via(i + j), "full", None)))
    return out


def prefix_1k_case():
    return ("8-2-128-q64-prefix1k", (8, 2, 128, PREFIX_1K, "bidirectional", 64, 131, "scale", "full", None))


def kv0_cases():
    return [(f"{_geom_id(*g)}-kv0", (*g, SUITE, "bidirectional", 64, 200 + i, _via(i), "kv0", None))
            for i, g in enumerate(KV0_GEOMETRIES)]


def reuse_cases():
    out = [(f"{_geom_id(*g)}-reuse", (*g, GEN, "bidirectional", 64, 300 + i, _via(i), "reuse", GEN_KEEP))
           for i, g in enumerate(REUSE_GEOMETRIES)]
    out.append(("16-2-128-decode", (16, 2, 128, DECODE, "bidirectional", 64, 331, "scale", "reuse", DECODE_KEEP)))
    return out


def pruned_cases():
    """The pruned last layer (work_last): full passes, and reused steps (work2_last + r2win)."""
    out = [(f"{_geom_id(*g)}-q{qb}-pruned", (*g, SUITE, "bidirectional", qb, 100 + i, _via(i), "full", None))
           for i, (qb, g) in enumerate(PRUNED_GEOMETRIES)]
    return out + [c for c in reuse_cases() if c[0] in ("16-2-128-reuse", "4-4-96-reuse", "16-2-128-decode")]


def all_cases():
    seen, out = set(), []
    for cid, args in full_cases() + [prefix_1k_case()] + kv0_cases() + reuse_cases() + pruned_cases():
        if args not in seen:
            seen.add(args)
            out.append((cid, args))
    return out
