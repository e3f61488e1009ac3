"""The output path: from "the last layer produced ``probs`` for a micro-batch" to "the caller's
arrays exist on the host".

One :class:`Outputs` per runner, built from its fixed mode (``next_token`` / ``loglik`` / ``embed``,
``score_top_k``, sampling), with three entry points: :meth:`Outputs.pick` (the next token of every
row), :meth:`Outputs.start` (the device-to-host copy of a micro-batch's result -> a
:class:`Pending`) and :meth:`Outputs.collect` (finished copies split back into prompts, into the
call's :class:`CallResults`).  The streamed executors, graph replays and speculative steps all go
through these; the runner publishes a call's ``CallResults`` to its public attributes.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ..embed import EmbedParams
from ..sampling import draws as sample_draws
from ..topk import TOPK_DTYPE
from .batch import PackedBatch


@dataclass
class Pending:
    """A micro-batch's output in flight to the host."""
    batch: PackedBatch
    # host views of one pooled pinned buffer (without a GPU: host tensors).  Full rows: (rows,) or
    # (rows, int32 tokens); compact scores: the four parts of ``Outputs._compact``
    host: Tuple[torch.Tensor, ...]
    event: Optional[torch.cuda.Event] = None     # the copies' end (None: same-stream copies, CPU)
    pool_buf: Optional[torch.Tensor] = None      # the pooled buffer to recycle
    picked: Optional[torch.Tensor] = None        # the rows' tokens on the device (a speculative step reads them)
    # a drafted micro-batch (prompt-lookup decoding): accepted draft tokens per suffix, rows scored / kept
    accept: Optional[np.ndarray] = None
    rows: int = 0
    kept: int = 0


@dataclass
class CallResults:
    """What one call returns and leaves on the runner (``ShardedRunner._publish``)."""
    outputs: List = field(default_factory=list)
    tokens: List = field(default_factory=list)             # last_tokens
    token_probs: List = field(default_factory=list)        # last_token_probs (score_top_k)
    accept: List = field(default_factory=list)             # last_accept (drafted calls)
    token_logprobs: List = field(default_factory=list)     # last_token_logprobs (loglik)
    d2h_bytes: int = 0                                     # score_d2h_bytes
    lookup_rows: int = 0
    lookup_kept: int = 0
    pair_lens: Optional[List[List[int]]] = None            # loglik: scored tokens per prompt and suffix

    @classmethod
    def begin(cls, tps: Sequence, loglik: bool = False) -> "CallResults":
        """A new call on ``tps``: every field reset, one slot per prompt."""
        n = len(tps)
        return cls([None] * n, [None] * n, [None] * n, [None] * n, [None] * n if loglik else [],
                   pair_lens=[[len(s) for s in tp.suffixes] for tp in tps] if loglik else None)


class Outputs:
    def __init__(self, mode: str, score_top_k: int, sampling, embed: Optional[EmbedParams], ops, device,
                 get_store: Callable, d2h_stream):
        self.mode, self.score_top_k, self.sampling, self.embed = mode, int(score_top_k), sampling, embed
        self.ops, self.dev, self.get_store, self.d2h_stream = ops, device, get_store, d2h_stream
        self.cuda = device.type == "cuda"
        self._table = None
        if sampling is not None:
            # the weight table, uploaded once (every weight is <= 2^30: the uint32 values as int32)
            self._table = torch.from_numpy(sampling.table().view(np.int32)).to(device)
        self._split = {"loglik": self._split_loglik, "embed": self._split_embed}.get(mode, self._split_scores)

    # ------------------------------------------------------------------ pick
    def pick(self, batch: PackedBatch, probs: torch.Tensor, step: int, prompt_base: int = 0) -> torch.Tensor:
        """[rows] int32 on the device: the next token of every suffix of ``batch``.  Greedy: the
        row argmax.  Sampling: ``ops.sample_rows`` with the batch's draws of (seed, ``prompt_base``
        + prompt id, suffix, generation step ``step``) (they depend on no data: a small pinned H2D
        on the current stream, no synchronisation)."""
        if self.sampling is None:
            return self.ops.argmax_rows(probs)
        d = sample_draws(self.sampling.seed, [prompt_base + int(p) for p in batch.prompt_ids], batch.n_suffix, step)
        host = torch.from_numpy(d.view(np.int64))
        if self.cuda:
            # (a pinned tensor of the caching host allocator: not reused before the copy ran)
            pinned = torch.empty(host.shape, dtype=torch.int64, pin_memory=True)
            pinned.copy_(host)
            host = pinned.to(self.dev, non_blocking=True)
        return self.ops.sample_rows(probs, self._table, host, self.sampling.top_k, self.sampling.P)

    # ----------------------------------------------------------------- start
    def start(self, batch: PackedBatch, probs: torch.Tensor, step: int, stream, prompt_base: int = 0) -> Pending:
        """D2H of a micro-batch's result on ``stream`` (None: the current stream, so the copy is
        ordered before the next graph replay): its probabilities and their picked tokens (the token
        of each suffix: api.generation_loop needs no host pass over the [n_s, V] scores);
        ``score_top_k``: the K best entries and the tokens' probabilities instead; loglik / embed:
        the fp32 [n_pairs, 2] head state / [n_sfx, D] norm state as it is; a drafted micro-batch:
        its kept rows."""
        if batch.draft is not None:
            return self._start_drafted(batch, probs, stream)
        tok = self.pick(batch, probs, step, prompt_base) if self.mode == "next_token" else None
        return self._start_rows(batch, probs, tok, stream)

    def _start_rows(self, batch, probs: torch.Tensor, tok: Optional[torch.Tensor], stream, **lookup) -> Pending:
        if self.score_top_k:
            parts = self._compact(probs, tok)
        else:
            if not self.cuda:
                probs = probs.detach().to(torch.float16 if self.mode == "next_token" else torch.float32)
            parts = (probs,) if tok is None else (probs, tok)
        host, pool_buf, ev = self._to_host(parts, stream)
        return Pending(batch, host, ev, pool_buf, tok, **lookup)

    def _compact(self, rows: torch.Tensor, tok: torch.Tensor):
        """The compact scores of ``rows`` (topk.py) in the order they lie in the host buffer: ids
        int32 [rows, K], tokens int32 [rows], probabilities fp16 [rows, K], token probabilities
        fp16 [rows] (the int32 parts first, so every view stays aligned).  ``ops.topk_rows`` is a
        plain launch on the current stream: right behind a graph replay too."""
        ids, vals, pv = self.ops.topk_rows(rows, self.score_top_k, picked=tok)
        return ids, tok, vals, pv

    def _to_host(self, parts, stream):
        """Device tensors ``parts`` one after the other in one pooled pinned buffer, each at the
        next multiple of its element size (full rows: the rows, then their int32 tokens), copied on
        ``stream`` (None: the current stream) -> (host views, the pooled buffer, the event after the
        copies on ``stream``).  Without a GPU: (host tensors, None, None)."""
        if not self.cuda:
            return tuple(p.detach().cpu().contiguous() for p in parts), None, None
        spans, end = [], 0
        for p in parts:
            size = p.element_size()
            start = -(-end // size) * size
            end = start + p.numel() * size
            spans.append((start, end))
        pool_buf = self.get_store().host_buffer(end)
        views = tuple(pool_buf[a:b].view(p.dtype).view(p.shape) for (a, b), p in zip(spans, parts))
        if stream is None:
            for h, d in zip(views, parts):
                h.copy_(d, non_blocking=True)
            return views, pool_buf, None
        stream.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(stream):
            for h, d in zip(views, parts):
                h.copy_(d, non_blocking=True)
                d.record_stream(stream)
            ev = torch.cuda.Event()
            ev.record(stream)
        return views, pool_buf, ev

    def _start_drafted(self, batch: PackedBatch, probs: torch.Tensor, stream) -> Pending:
        """A drafted micro-batch's output: ``ops.verify_rows`` on its scored rows, then the D2H of
        the KEPT rows only (gathered into a compact device buffer, from there into the pooled
        pinned buffer; ``score_top_k``: ``topk_rows`` on the kept rows).  The host waits once, for
        the accepted counts (a few ints): they size the copy."""
        meta = batch.device_tensors(self.dev)
        tok, accept, keep, n_kept = self.ops.verify_rows(probs, meta["row_start"], meta["draft"])
        n_sfx = accept.shape[0]
        if self.cuda:
            # accept and n_kept are one [n_sfx + 1] vector on the device (ops.verify_rows): one copy,
            # and the host waits for that copy alone
            dev_ctrl = accept.as_strided((n_sfx + 1,), (1,))
            assert dev_ctrl[n_sfx:].data_ptr() == n_kept.data_ptr()
        else:
            dev_ctrl = torch.cat([accept, n_kept])
        (ctrl,), ctrl_buf, _ = self._to_host((dev_ctrl,), None)
        if self.cuda:
            done = torch.cuda.Event()
            done.record(torch.cuda.current_stream(self.dev))
            done.synchronize()
        acc = ctrl[:n_sfx].numpy().astype(np.int64)
        nk = int(ctrl[n_sfx])
        if ctrl_buf is not None:
            self.get_store().recycle_host(ctrl_buf)
        if nk != int(acc.sum()) + n_sfx:
            raise RuntimeError(f"verify_rows kept {nk} rows for accepted counts summing to {int(acc.sum())} "
                               f"over {n_sfx} suffixes")
        idx = keep[:nk]
        kept = self.gather_kept(probs, idx)                      # [kept, V]: what crosses PCIe
        tok_k = tok.index_select(0, idx.long()).contiguous()
        return self._start_rows(batch, kept, tok_k, stream, accept=acc, rows=int(probs.shape[0]), kept=nk)

    def gather_kept(self, probs: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
        """probs[idx] as a compact [len(idx), V] tensor: ``copy_rows`` (16 bytes per lane) where the
        rows allow it, ``index_select`` for a vocabulary that is no multiple of 8 (Granite's 49,155)."""
        if probs.shape[1] % 8 == 0 and probs.stride(0) % 8 == 0 and probs.data_ptr() % 16 == 0:
            return self.ops.gather_rows(probs, idx)
        return probs.index_select(0, idx.long())

    # --------------------------------------------------------------- collect
    def collect(self, pending: Sequence[Pending], res: CallResults) -> None:
        """Finished copies split back into prompts, into ``res`` (prompt order); their pooled
        buffers go back to the pool.  The caller has waited for the copies."""
        store = self.get_store()
        for p in pending:
            res.d2h_bytes += sum(h.numel() * h.element_size() for h in p.host)
            self._split(p, [h.numpy() for h in p.host], res)
            if p.pool_buf is not None:
                store.recycle_host(p.pool_buf)

    def _score_rows(self, host, r: int, n: int):
        """Rows r .. r + n of a micro-batch's host scores -> (the caller's array: fp16 [n, V], or
        ``TOPK_DTYPE`` [n, K]; the rows' int64 tokens; their fp16 probabilities or None)."""
        if self.score_top_k:
            ids, tok, vals, pv = host                            # Outputs._compact
            out = np.empty((n, self.score_top_k), dtype=TOPK_DTYPE)
            out["id"], out["p"] = ids[r:r + n], vals[r:r + n]
            return out, tok[r:r + n].astype(np.int64), pv[r:r + n].copy()
        rows, tok = host
        return rows[r:r + n].astype(np.float16, copy=True), tok[r:r + n].astype(np.int64), None

    def _split_scores(self, p: Pending, host, res: CallResults) -> None:
        """Per prompt a [n_s, 1, V] fp16 (``score_top_k``: ``TOPK_DTYPE`` [n_s, 1, K]) array, its
        [n_s, 1] tokens and (``score_top_k``) their probabilities.  A drafted micro-batch: per
        prompt LISTS with one [kept, ...] array per suffix — the rows of its accepted draft tokens
        and the one after them — and the accepted counts."""
        batch, acc = p.batch, p.accept
        n_rows = p.kept if acc is not None else int(sum(batch.n_suffix))
        assert all(h.shape[0] == n_rows for h in host), ([h.shape for h in host], n_rows)
        res.lookup_rows += p.rows
        res.lookup_kept += p.kept
        r = i = 0
        for j, pid in enumerate(batch.prompt_ids):
            ns = batch.n_suffix[j]
            if acc is None:
                out, tok, pv = self._score_rows(host, r, ns)
                res.outputs[pid] = np.expand_dims(out, axis=1)
                res.tokens[pid] = tok.reshape(ns, 1)
                res.token_probs[pid] = pv.reshape(ns, 1) if pv is not None else None
                r += ns
                continue
            per_sfx = []
            for a in acc[i:i + ns]:
                per_sfx.append(self._score_rows(host, r, int(a) + 1))
                r += int(a) + 1
            res.outputs[pid], res.tokens[pid], pvs = ([x[c] for x in per_sfx] for c in range(3))
            res.token_probs[pid] = pvs if self.score_top_k else None
            res.accept[pid] = acc[i:i + ns].copy()
            i += ns
        assert r == n_rows and (acc is None or i == acc.shape[0]), (r, n_rows, i)

    def _split_loglik(self, p: Pending, host, res: CallResults) -> None:
        """The [n_pairs, 2] (log-probability, greedy flag) rows of a finished micro-batch split back
        into suffixes (pairs are in prompt -> suffix -> token order): per prompt the [n_s, 3] float32
        (sum, token count, all-greedy) — sums in float64 — and the per-token values."""
        batch, (pairs,) = p.batch, host
        r = 0
        for j, pid in enumerate(batch.prompt_ids):
            s0, s1 = (int(v) for v in batch.prompt_scored[j])
            lens = res.pair_lens[pid]
            assert s0 == r and s1 - s0 == sum(lens), (s0, s1, r, lens)
            out = np.empty((len(lens), 3), dtype=np.float32)
            per_tok = []
            for s, n in enumerate(lens):
                lp = pairs[r:r + n, 0].astype(np.float32, copy=True)
                out[s] = (lp.astype(np.float64).sum(), n, float(bool((pairs[r:r + n, 1] == 1.0).all())))
                per_tok.append(lp)
                r += n
            res.outputs[pid] = out
            res.token_logprobs[pid] = per_tok

    def _split_embed(self, p: Pending, host, res: CallResults) -> None:
        """The [n_suffixes, D] float32 embeddings of a finished micro-batch (prompt -> suffix order)
        split back into prompts."""
        batch, (emb,) = p.batch, host
        assert emb.dtype == np.float32 and emb.shape == (int(sum(batch.n_suffix)), self.embed.dim), (emb.dtype, emb.shape)
        r = 0
        for j, pid in enumerate(batch.prompt_ids):
            ns = batch.n_suffix[j]
            res.outputs[pid] = emb[r:r + ns].copy()
            r += ns
