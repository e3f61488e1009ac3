"""Sliding-window forms of the per-row attention checks of attention_rows.py (a plain helper module).

The window is applied to the masks of ``attention_rows.segment_keys`` from the ``Segment`` fields
alone (``window``, and the positions the fields imply), so the fp64 and the emulated references, the
error bound ``tau`` and ``min_single_key_effect`` are attention_rows' own, over windowed masks.

* :func:`window_edit` - the mask edit: key at model position j visible to the query at i iff i - j < W;
  with ``delta`` / ``ranges`` the lower bound is off by one in the named key ranges (the mutations);
* :class:`WCase` - an ``attention_rows.Case`` re-packed with ``window=W`` in the kernel's layout;
* :func:`skipped_cache_rows` - K/V cache rows in 64-key tiles wholly before every lower bound of
  every work item: a kernel that skips those tiles never reads them.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

import attention_rows as ar
from flexible_llm_sharding_amd.runtime.batch import PackedBatch, pack_prompts, visible_keys

PROMPTS = ((200, (33, 64, 70)), (70, (5, 130)), (1, (3,)))
WINDOWS = (1, 63, 64, 65, 100, 150)
MODES = ("bidirectional", "causal")
# kept rows of every suffix (range 2), GEN_KEEP-style: some, most, none of a suffix
REUSE_KEEP = ((3, 40, 0), (4, 5), (0,))
# a decode step: one new row per suffix after the kept ones
DECODE_KEEP = tuple(tuple(l - 1 for l in ls) for _, ls in PROMPTS)
# (q_block, (nh, nkv, hd)) of the full / kv0 / reuse cases, and the decode geometry
GEOMETRIES = ((64, (8, 2, 128)), (128, (4, 2, 64)), (64, (4, 4, 96)))
DECODE_GEOMETRY = (64, (16, 2, 128))


def _positions(sg, c):
    """(query positions [q_len], key positions [n_keys]) of a segment's candidate columns."""
    suffix = sg.r1_len > 0
    r2l = getattr(sg, "r2_len", 0)
    qpos = np.arange(sg.q_len) + sg.q_off + (sg.r0_len + r2l if suffix else 0)
    rng, idx = c["rng"], c["idx"]
    kpos = np.where(rng == 0, idx, np.where(rng == 2, sg.r0_len + idx, sg.r0_len + r2l + idx))
    kpos = np.where(rng == 3, sg.r0_len + r2l - 1, kpos)          # (never visible)
    return qpos, kpos


def window_edit(delta: int = 0, ranges=(0, 1, 2)):
    """``edit`` for attention_rows._run: the segment's window W on every range; with ``delta`` the
    keys of ``ranges`` take W + delta instead (rows left without a key keep W).  ``hit``: rows whose
    mask differs from the W mask."""
    def edit(sg, c, mask):
        W = sg.window
        if not W:
            return mask, np.zeros(mask.shape[0], dtype=bool)
        qpos, kpos = _positions(sg, c)
        d = qpos[:, None] - kpos[None, :]
        base = mask & (d < W)
        if not delta:
            return base, np.zeros(mask.shape[0], dtype=bool)
        sel = np.isin(c["rng"], ranges)[None, :]
        new = mask & np.where(sel, d < W + delta, d < W)
        ok = new.any(1)
        new = np.where(ok[:, None], new, base)
        return new, (new != base).any(1)
    return edit


def run(qkv, segments, nh, nkv, hd, kv0=None, scale=None, arith="f64", delta=0, ranges=(0, 1, 2), effect=False):
    """attention_rows._run over windowed masks -> (out, queried, touched, effect)."""
    return ar._run(qkv, segments, nh, nkv, hd, kv0, scale, arith, edit=window_edit(delta, ranges),
                   want_effect=effect)


def _cache_layout(prompts):
    """The K/V cache rows attention_rows.flat_case gives every prefix and suffix."""
    offs, t = [], 0
    for lp, _ in prompts:
        t += ar.GAP
        offs.append(t)
        t += lp
    rows = []
    for _, ls in prompts:
        t += ar.GAP
        rows.append([])
        for l in ls:
            rows[-1].append(t)
            t += l
    return offs, rows


@dataclass
class WCase:
    """``base`` (attention_rows.Case: inputs, cache, layout) with every batch re-packed at window W."""
    base: ar.Case
    W: int
    b: PackedBatch          # the kernel's layout, windowed
    full: PackedBatch       # the same prompts as one packed pass, windowed
    mode: str = "bidirectional"
    seed: int = 0
    via: Optional[str] = "q"
    prompts: tuple = PROMPTS

    def __getattr__(self, name):        # nh, nkv, hd, q_block, kind, qkv, kv0, scale, rows, ...
        return getattr(self.base, name)

    def _full(self, **kw):
        c = self.base
        return run(c.full_qkv, self.full.segments, c.nh, c.nkv, c.hd, scale=c.scale, **kw)

    @property
    def _shared(self):
        return _full_refs(self.W, self.nh, self.nkv, self.hd, self.mode, self.seed, self.via, self.prompts)

    @property
    def ref(self):
        return self._shared["ref"][self.base.rows]

    @property
    def tau(self) -> float:
        return ar.TAU_FACTOR * float(self._shared["emu_err"][self.base.rows].max())

    @property
    def min_effect(self) -> float:
        return float(_full_effect(self.W, self.nh, self.nkv, self.hd, self.mode, self.seed, self.via,
                                  self.prompts)[self.base.rows].min())

    def mutated(self, delta, ranges, arith="emu"):
        """(reference with the lower bound of ``ranges`` off by ``delta``, rows it touches)."""
        m, _, touched, _ = self._full(arith=arith, delta=delta, ranges=ranges)
        return m[self.base.rows], touched[self.base.rows]


def _full_pass(W, nh, nkv, hd, mode, seed, via, prompts):
    base = ar.flat_case(nh, nkv, hd, prompts, mode, 64, seed, via, "full", None)
    full = pack_prompts(ar._tps(prompts), list(range(len(prompts))), mode, window=W)
    return base, full


@functools.lru_cache(maxsize=None)
def _full_refs(W, nh, nkv, hd, mode, seed, via, prompts):
    """fp64 reference and the emulated kernel's error of the windowed full packed pass, per (row,
    head): shared by the full / kv0 / reuse cases of one geometry (the same inputs and keys)."""
    base, full = _full_pass(W, nh, nkv, hd, mode, seed, via, prompts)
    r, queried, _, _ = run(base.qkv, full.segments, nh, nkv, hd, scale=base.scale)
    assert bool(queried.all())
    e = run(base.qkv, full.segments, nh, nkv, hd, scale=base.scale, arith="emu")[0]
    return {"ref": r, "emu_err": ar.row_err(e, r)}


@functools.lru_cache(maxsize=None)
def _full_effect(W, nh, nkv, hd, mode, seed, via, prompts):
    base, full = _full_pass(W, nh, nkv, hd, mode, seed, via, prompts)
    return run(base.qkv, full.segments, nh, nkv, hd, scale=base.scale, effect=True)[3]


@functools.lru_cache(maxsize=None)
def wcase(W, nh, nkv, hd, mode="bidirectional", q_block=64, seed=0, via="q", kind="full", keep=None,
          prompts=PROMPTS) -> WCase:
    base = ar.flat_case(nh, nkv, hd, prompts, mode, q_block, seed, via, kind, keep)
    tps, ids = ar._tps(prompts), list(range(len(prompts)))
    if kind == "full":
        full = pack_prompts(tps, ids, mode, q_block=q_block, window=W)
        return WCase(base, W, full, full, mode, seed, via, prompts)
    offs, rows = _cache_layout(prompts)
    full = pack_prompts(tps, ids, mode, prefix_offsets=offs, q_block=q_block,
                        suffix_rows=rows if kind == "reuse" else None, window=W)
    if kind == "reuse":
        b = pack_prompts(tps, ids, mode, prefix_offsets=offs, kv_cached=True, q_block=q_block, suffix_rows=rows,
                         suffix_keep=[list(k) for k in keep], window=W)
    else:
        b = pack_prompts(tps, ids, mode, prefix_offsets=offs, kv_cached=True, q_block=q_block, window=W)
    assert b.num_tokens == base.b.num_tokens and np.array_equal(b.ids, base.b.ids)
    return WCase(base, W, b, full, mode, seed, via, prompts)


def cases():
    """(id, wcase arguments) of every GPU case: geometry x kind x mode x window."""
    out = []
    for gi, (qb, (nh, nkv, hd)) in enumerate(GEOMETRIES):
        for kind, keep in (("full", None), ("kv0", None), ("reuse", REUSE_KEEP)):
            for mi, mode in enumerate(MODES):
                for W in WINDOWS:
                    out.append((f"{nh}-{nkv}-{hd}-q{qb}-{kind}-{mode}-W{W}",
                                (W, nh, nkv, hd, mode, qb, 400 + gi, ar._via(gi + mi), kind, keep)))
    qb, (nh, nkv, hd) = DECODE_GEOMETRY
    for mi, mode in enumerate(MODES):
        for W in WINDOWS:
            out.append((f"{nh}-{nkv}-{hd}-decode-{mode}-W{W}",
                        (W, nh, nkv, hd, mode, qb, 431, ar._via(mi), "reuse", DECODE_KEEP)))
    return out


# --------------------------------------------------------------------------- masks of the work items
def work_item_masks(b: PackedBatch, work, work2, n_rows: int, reuse: bool):
    """attention_rows.work_item_masks with the window's range-0 bounds (``b.r0_lo``)."""
    out = [None] * n_rows
    queried = np.zeros(n_rows, dtype=bool)
    for it in work:
        queried[it[0]:it[0] + it[1]] = True
    for r in np.flatnonzero(queried):
        codes = [np.zeros(0, dtype=np.int64)]
        for rng, lo, hi in visible_keys(work, b.seg_lo, int(r), work2, b.r2win if reuse else None, r0_lo=b.r0_lo):
            in_cache = rng == 2 or (rng == 0 and b.kv_cached)
            codes.append(ar.key_codes(np.full(hi - lo + 1, 1 if in_cache else 0), np.arange(lo, hi + 1)))
        out[r] = np.sort(np.concatenate(codes))
    return out


def segment_masks(segments, cached: bool, n_rows: int, packed_to_cache=None):
    """attention_rows.segment_masks over the windowed masks."""
    out = [None] * n_rows
    edit = window_edit()
    for sg, c, mask in ar.segment_keys(segments, cached):
        mask, _ = edit(sg, c, mask)
        buf, row = c["buf"].copy(), c["row"].copy()
        if packed_to_cache is not None:
            p = buf == 0
            buf[p], row[p] = 1, packed_to_cache[row[p]]
        codes = ar.key_codes(buf, row)
        for i in range(sg.q_len):
            out[sg.q_start + i] = np.sort(codes[mask[i]])
    return out


def walked_cache_rows(b: PackedBatch, n_cache_rows: int, items=("work", "work_last")) -> np.ndarray:
    """[n_cache_rows] bool: rows of the K/V cache inside a 64-key tile some work item walks (range
    0 from the tile of the item's smallest lower bound, none when that is past the range; range 2
    as work2 gives it)."""
    hit = np.zeros(n_cache_rows, dtype=bool)
    for name in items:
        work = getattr(b, name)
        r0i = b.r0_item if name == "work" else b.r0_item_last
        w2 = b.work2 if name == "work" else b.work2_last
        for it, w in enumerate(work.tolist()):
            q_len, q_off, r0s, r0l, r0c = w[1], w[2], w[3], w[4], w[5]
            kend0 = min(r0l, q_off + q_len) if r0c else r0l
            first = min(max(int(r0i[it, 0]), 0), r0l)
            if b.kv_cached and first < kend0:
                hit[r0s + first // 64 * 64:r0s + r0l] = True
            if w2 is not None and w2[it, 1] > 0:
                hit[int(w2[it, 0]):int(w2[it, 0] + w2[it, 1])] = True
    return hit


def skipped_cache_rows(c: WCase) -> np.ndarray:
    """Finite rows of the case's K/V cache that no work item of the windowed batch walks."""
    n = c.kv0.shape[0]
    finite = torch.isfinite(c.kv0).all(1).numpy()
    return np.flatnonzero(finite & ~walked_cache_rows(c.b, n))


def poisoned_cache(c: WCase) -> Optional[torch.Tensor]:
    kv0 = c.kv0.clone()
    kv0[torch.from_numpy(skipped_cache_rows(c)).long()] = float("nan")
    return kv0
