"""Plain-PyTorch implementation of every op (CPU path + numerics oracle).

Semantics follow the HF Llama block the reference drives
(``/root/reference/utils.py:266-290``): RMSNorm with fp32
statistics, RoPE rotate-half with fp16-rounded cos/sin tables, softmax in
fp32, SwiGLU MLP.  Weights are the packed images of :mod:`..models.layout`
(checkpoint row order: ``wqkv = [q; k; v]``, ``wgu = [gate; up]``), exactly
what the HIP kernels consume, so this backend is a drop-in oracle for them.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F


class TorchOps:
    name = "torch"
    fused_norm = False          # explicit RMSNorm (the oracle keeps HF's cast points)

    def __init__(self, compute_dtype: torch.dtype = torch.float32):
        self.cdt = compute_dtype

    # ---------------------------------------------------------------- helpers
    def _c(self, t: torch.Tensor) -> torch.Tensor:
        return t if t.dtype == self.cdt else t.to(self.cdt)

    # ------------------------------------------------------------------- ops
    def embed(self, ids: torch.Tensor, table: torch.Tensor, out_dtype, scale: float = 1.0, out=None) -> torch.Tensor:
        e = table.index_select(0, ids.long())
        if scale != 1.0:                       # Granite: GraniteModel scales the embeddings
            e = (self._c(e) * scale).to(table.dtype)
        e = e.to(out_dtype)
        if out is not None:
            out.copy_(e)
            return out
        return e

    def copy_rows(self, x, src_idx, y, dst_idx):
        rows = x.index_select(0, src_idx.long()) if src_idx is not None else x
        if dst_idx is not None:
            y.index_copy_(0, dst_idx.long(), rows.to(y.dtype))
        else:
            y.copy_(rows)
        return y

    def gather_rows(self, x, idx, out=None):
        return x.index_select(0, idx.long()) if out is None else self.copy_rows(x, idx, out, None)

    def scatter_rows(self, x, idx, y):
        return self.copy_rows(x, None, y, idx)

    def rmsnorm(self, x: torch.Tensor, w: torch.Tensor, eps: float, out=None) -> torch.Tensor:
        # LlamaRMSNorm: fp32 variance, normalise, cast back, scale by weight.
        xf = x.float()
        var = xf.pow(2).mean(-1, keepdim=True)
        y = (xf * torch.rsqrt(var + eps)).to(x.dtype)
        return (self._c(w) * self._c(y)).to(x.dtype)

    def linear(self, x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
        return (self._c(x) @ self._c(w).t()).to(x.dtype)

    def linear_residual(self, x: torch.Tensor, w: torch.Tensor, resid: torch.Tensor,
                        bias: torch.Tensor = None, alpha: float = 1.0) -> torch.Tensor:
        y = self._c(x) @ self._c(w).t()
        if bias is not None:
            y = y + self._c(bias)
        if alpha != 1.0:
            # Granite's residual_multiplier in HF GraniteDecoderLayer's roundings: x + fp16(fp16(y) * r)
            y = (self._c(y.to(resid.dtype)) * alpha).to(resid.dtype)
        return (self._c(resid) + self._c(y)).to(resid.dtype)

    def swiglu_up(self, x: torch.Tensor, wgu: torch.Tensor, out=None) -> torch.Tensor:
        y = self._c(x) @ self._c(wgu).t()                     # [T, 2I] = [gate | up]
        I = y.shape[1] // 2
        return (F.silu(y[:, :I]) * y[:, I:]).to(x.dtype)

    def qkv_rope(self, x: torch.Tensor, wqkv: torch.Tensor, positions: torch.Tensor,
                 cos: torch.Tensor, sin: torch.Tensor, n_q_heads: int, n_kv_heads: int,
                 head_dim: int, bias: torch.Tensor = None, out=None) -> torch.Tensor:
        y = self._c(x) @ self._c(wqkv).t()
        if bias is not None:
            y = y + self._c(bias)
        qk_cols = (n_q_heads + n_kv_heads) * head_dim
        T = y.shape[0]
        half = head_dim // 2
        qk = y[:, :qk_cols].reshape(T, n_q_heads + n_kv_heads, 2, half)   # HF rotate_half halves
        c = cos.index_select(0, positions.long()).to(self.cdt).reshape(T, 1, half)   # [T, 1, hd/2]
        s = sin.index_select(0, positions.long()).to(self.cdt).reshape(T, 1, half)
        x1, x2 = qk[:, :, 0, :], qk[:, :, 1, :]
        o1 = x1 * c - x2 * s
        o2 = x2 * c + x1 * s
        qk_out = torch.stack([o1, o2], dim=2).reshape(T, qk_cols)
        return torch.cat([qk_out, y[:, qk_cols:]], dim=1).to(x.dtype)

    def qkv_norm_rope(self, x: torch.Tensor, wqkv: torch.Tensor, positions: torch.Tensor, cos: torch.Tensor,
                      sin: torch.Tensor, n_q_heads: int, n_kv_heads: int, head_dim: int, qn: torch.Tensor,
                      kn: torch.Tensor, eps: float, bias: torch.Tensor = None, out=None) -> torch.Tensor:
        """Qwen3 projection: RMSNorm over head_dim on the q (q_norm) and k (k_norm) heads, then RoPE."""
        y = self._c(x) @ self._c(wqkv).t()
        if bias is not None:
            y = y + self._c(bias)
        y = y.to(x.dtype)
        T = y.shape[0]
        nqk = n_q_heads + n_kv_heads
        heads = y[:, :nqk * head_dim].reshape(T, nqk, head_dim).float()
        var = heads.pow(2).mean(-1, keepdim=True)
        normed = (heads * torch.rsqrt(var + eps)).to(x.dtype)
        w = torch.cat([qn.reshape(1, -1).expand(n_q_heads, -1), kn.reshape(1, -1).expand(n_kv_heads, -1)])
        normed = (self._c(w)[None] * self._c(normed)).to(x.dtype)
        half = head_dim // 2
        qk = self._c(normed).reshape(T, nqk, 2, half)
        c = cos.index_select(0, positions.long()).to(self.cdt).reshape(T, 1, half)
        s = sin.index_select(0, positions.long()).to(self.cdt).reshape(T, 1, half)
        x1, x2 = qk[:, :, 0, :], qk[:, :, 1, :]
        qk_out = torch.stack([x1 * c - x2 * s, x2 * c + x1 * s], dim=2).reshape(T, nqk * head_dim)
        return torch.cat([qk_out.to(x.dtype), y[:, nqk * head_dim:]], dim=1)

    def moe_ffn(self, h: torch.Tensor, x: torch.Tensor, wrouter: torch.Tensor, wgu: torch.Tensor,
                wdown: torch.Tensor, top_k: int, norm_topk: bool, round_w16: bool = False, m_out=None,
                y_out=None, shared=None) -> torch.Tensor:
        """x += sparse-MoE FFN of h, in place, in the order and rounding of HF's expert loop
        (transformers MixtralExperts / Qwen3MoeExperts): router Linear in the activation dtype,
        fp32 softmax, top-k, optional renormalisation (Qwen3-MoE rounds the weights to the
        activation dtype), each expert's weighted output rounded to the activation dtype and
        accumulated in expert order, plus the gated shared-expert output (Qwen2-MoE) in one more
        rounding, then added to the residual."""
        logits = self.linear(h, wrouter)
        w, idx = torch.topk(torch.softmax(logits.float(), dim=-1), top_k, dim=-1)
        if norm_topk:
            w = w / w.sum(-1, keepdim=True)
        if round_w16:
            w = w.to(h.dtype).float()
        acc = torch.zeros_like(x)
        for e in range(wgu.shape[0]):
            tok, slot = torch.where(idx == e)
            if tok.numel() == 0:
                continue
            y = self.linear(self.swiglu_up(h.index_select(0, tok), wgu[e]), wdown[e])
            acc.index_add_(0, tok, (y.float() * w[tok, slot, None]).to(x.dtype))
        if shared is not None:
            acc = (acc.float() + shared.float()).to(x.dtype)
        x.copy_((x.float() + acc.float()).to(x.dtype))
        return x

    def attention(self, qkv: torch.Tensor, segments, n_q_heads: int, n_kv_heads: int,
                  head_dim: int, kv0: torch.Tensor = None, q_block: int = 64, out=None,
                  scale: float = None) -> torch.Tensor:
        """Shared-prefix attention over packed segments (see runtime.batch).

        ``kv0`` ([P, 2 * n_kv * hd], K then V): range 0 of every segment indexes
        these rows instead of the packed QKV (prefix K/V cache)."""
        T = qkv.shape[0]
        qs = n_q_heads * head_dim
        ks = n_kv_heads * head_dim
        q_all = qkv[:, :qs].view(T, n_q_heads, head_dim)
        k_all = qkv[:, qs:qs + ks].view(T, n_kv_heads, head_dim)
        v_all = qkv[:, qs + ks:qs + 2 * ks].view(T, n_kv_heads, head_dim)
        if kv0 is not None:
            k0_all = kv0[:, :ks].reshape(-1, n_kv_heads, head_dim)
            v0_all = kv0[:, ks:2 * ks].reshape(-1, n_kv_heads, head_dim)
        else:
            k0_all, v0_all = k_all, v_all
        out = torch.empty(T, qs, dtype=qkv.dtype, device=qkv.device)
        rep = n_q_heads // n_kv_heads
        scale = head_dim ** -0.5 if scale is None else scale
        dev = qkv.device
        for sg in segments:
            q = self._c(q_all[sg.q_start:sg.q_start + sg.q_len])                # [q, nh, d]
            kr = [(sg.r0_start, sg.r0_len, sg.r0_causal, k0_all, v0_all)]
            if getattr(sg, "r2_len", 0):        # suffix K/V reuse: the suffix's kept rows, all visible
                kr.append((sg.r2_start, sg.r2_len, 0, k0_all, v0_all))
            if sg.r1_len:
                # (bidirectional suffixes: the segment is one suffix, every key of it visible)
                kr.append((sg.r1_start, sg.r1_len, 0 if getattr(sg, "r1_bidir", 0) else 1, k_all, v_all))
            ks_, vs_, masks = [], [], []
            qi = torch.arange(sg.q_len, device=dev) + sg.q_off
            for st, ln, causal, kk, vv in kr:
                ks_.append(kk[st:st + ln])
                vs_.append(vv[st:st + ln])
                kj = torch.arange(ln, device=dev)
                m = torch.ones(sg.q_len, ln, dtype=torch.bool, device=dev)
                if causal:
                    m = kj[None, :] <= qi[:, None]
                masks.append(m)
            W = getattr(sg, "window", 0)
            if W:
                # sliding window over model positions: prefix token p at p; token s of a suffix at
                # r0_len + s, its kept rows (range 2) first.  Only the past is cut off.
                r2l = getattr(sg, "r2_len", 0)
                qpos = qi + (sg.r0_len + r2l if sg.r1_len else 0)
                kpos = [torch.arange(sg.r0_len, device=dev)]
                if r2l:
                    kpos.append(sg.r0_len + torch.arange(r2l, device=dev))
                if sg.r1_len:
                    kpos.append(sg.r0_len + r2l + torch.arange(sg.r1_len, device=dev))
                masks = [torch.cat(masks, 1) & (qpos[:, None] - torch.cat(kpos)[None, :] < W)]
            k = self._c(torch.cat(ks_, 0)).repeat_interleave(rep, dim=1)        # [k, nh, d]
            v = self._c(torch.cat(vs_, 0)).repeat_interleave(rep, dim=1)
            mask = torch.cat(masks, 1)                                          # [q, k]
            s = torch.einsum("qhd,khd->hqk", q.float(), k.float()) * scale
            s = s.masked_fill(~mask[None], float("-inf"))
            p = torch.softmax(s, dim=-1)
            o = torch.einsum("hqk,khd->qhd", p, v.float())
            out[sg.q_start:sg.q_start + sg.q_len] = o.reshape(sg.q_len, qs).to(qkv.dtype)
        return out

    def gather_rmsnorm(self, x: torch.Tensor, idx: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
        return self.rmsnorm(x.index_select(0, idx.long()), w, eps)

    def lm_head_softmax(self, h: torch.Tensor, w: torch.Tensor, logits_scaling: float = 1.0) -> torch.Tensor:
        logits = (self._c(h) @ self._c(w).t()).to(h.dtype)   # fp16 logits like nn.Linear in fp16
        return self.softmax(logits, logits_scaling)

    def logprob_rows(self, logits: torch.Tensor, targets: torch.Tensor, logits_scaling: float = 1.0) -> torch.Tensor:
        """[rows, 2] fp32: (l[t] - logsumexp(l), l[t] == max(l)) with l the rows :meth:`softmax`
        normalises (fp16-rounded where the activations are fp16) and t = targets[row]."""
        if logits_scaling != 1.0:
            logits = logits / logits_scaling
        l = logits.float()
        lt = l.gather(1, targets.long()[:, None])[:, 0]
        lp = torch.log_softmax(l, dim=-1).gather(1, targets.long()[:, None])[:, 0]
        return torch.stack([lp, (lt == l.max(dim=-1).values).float()], dim=1)

    def lm_head_logprob(self, h: torch.Tensor, w: torch.Tensor, targets: torch.Tensor, logits_scaling: float = 1.0,
                        chunk_rows: int = 0, scratch=None) -> torch.Tensor:
        """HipOps.lm_head_logprob: head matmul -> :meth:`logprob_rows` in chunks of ``chunk_rows``
        rows (0: all rows at once)."""
        rows = h.shape[0]
        step = min(rows, chunk_rows) if chunk_rows > 0 else rows
        out = torch.empty(rows, 2, dtype=torch.float32, device=h.device)
        for s in range(0, rows, max(step, 1)):
            logits = (self._c(h[s:s + step]) @ self._c(w).t()).to(h.dtype)
            out[s:s + step] = self.logprob_rows(logits, targets[s:s + step], logits_scaling)
        return out

    def pool_rows(self, x: torch.Tensor, seg_start: torch.Tensor, dim: int = 0, normalize: bool = True,
                  row_idx: Optional[torch.Tensor] = None, out=None) -> torch.Tensor:
        """HipOps.pool_rows in fp32 (embed.py's definition): per segment of the row list
        (``x[row_idx]`` or ``x``) the mean of the first ``dim or H`` columns, optionally divided by
        max(its L2 norm, 1e-12); an empty segment gives zeros."""
        H = x.shape[1]
        D = int(dim) or H
        if isinstance(dim, bool) or not 1 <= D <= H:
            raise ValueError(f"dim in 1..{H} (0: {H}) expected, got {dim!r}")
        rows = x.index_select(0, row_idx.long()) if row_idx is not None else x
        ss = [int(v) for v in seg_start.tolist()]
        res = torch.zeros(len(ss) - 1, D, dtype=torch.float32, device=x.device)
        for i, (a, b) in enumerate(zip(ss[:-1], ss[1:])):
            if b > a:
                res[i] = rows[a:b, :D].float().sum(0) / float(b - a)
        if normalize:
            res = res / res.norm(dim=1, keepdim=True).clamp_min(1e-12)
        if out is not None:
            out.copy_(res)
            return out
        return res

    def classify_rows(self, x: torch.Tensor, w16: torch.Tensor, bias: Optional[torch.Tensor] = None,
                      activation: str = "none", row_idx: Optional[torch.Tensor] = None, out=None) -> torch.Tensor:
        """HipOps.classify_rows in fp32 (classify.py's definition): ``act(x[row] . w16[l] + bias[l])``."""
        from ..classify import ACTIVATIONS
        if activation not in ACTIVATIONS:
            raise ValueError(f"activation must be one of {ACTIVATIONS}, got {activation!r}")
        if activation == "softmax" and w16.shape[0] == 1:
            raise ValueError("softmax over one label is the constant 1")
        rows = x.index_select(0, row_idx.long()) if row_idx is not None else x
        z = rows.float() @ w16.float().t()
        if bias is not None:
            z = z + bias.float()
        if activation == "softmax":
            z = torch.softmax(z, dim=1)
        elif activation == "sigmoid":
            z = torch.sigmoid(z)
        if out is not None:
            out.copy_(z)
            return out
        return z

    def row_exact(self, on: bool = True):
        """HipOps.row_exact: nothing to select here (one matmul path)."""
        import contextlib
        return contextlib.nullcontext()

    def argmax_rows(self, probs: torch.Tensor) -> torch.Tensor:
        return probs.float().argmax(-1).to(torch.int32)

    def sample_rows(self, probs: torch.Tensor, table: torch.Tensor, draws: torch.Tensor, top_k: int,
                    P: int) -> torch.Tensor:
        """HipOps.sample_rows through the host sampler (sampling.sample_tokens: the same tokens).
        ``table``: int32 weights, ``draws``: the uint64 draws as int64."""
        from ..sampling import sample_tokens
        p16 = probs.detach().to(torch.float16).cpu().numpy()
        tok = sample_tokens(p16, table.cpu().numpy().view(np.uint32), int(top_k), int(P),
                            draws.cpu().numpy().view(np.uint64))
        return torch.from_numpy(tok.astype(np.int32)).to(probs.device)

    def topk_rows(self, probs: torch.Tensor, K: int, picked: Optional[torch.Tensor] = None):
        """HipOps.topk_rows through the host implementation (topk.topk_rows: the same entries)."""
        from ..topk import MAX_K, picked_keys, topk_rows
        if probs.dim() != 2:
            raise TypeError("probs must be a [rows, V] tensor")
        rows, V = probs.shape
        if picked is not None and (picked.dtype != torch.int32 or picked.numel() != rows):
            raise TypeError(f"picked must be an int32 vector of {rows} entries")
        if isinstance(K, bool) or int(K) != K or not 1 <= int(K) <= min(V, MAX_K):
            raise ValueError(f"K in 1..min(V, {MAX_K}) expected, got {K} at V = {V}")
        p16 = probs.detach().to(torch.float16).cpu().numpy()
        ids, vals = topk_rows(p16, int(K))
        pv = None
        if picked is not None:
            pv = torch.from_numpy(picked_keys(p16, picked.cpu().numpy()).view(np.float16)).to(probs.device)
        return (torch.from_numpy(ids).to(probs.device), torch.from_numpy(vals.view(np.float16)).to(probs.device), pv)

    def verify_rows(self, probs: torch.Tensor, row_start: torch.Tensor, draft: torch.Tensor):
        """HipOps.verify_rows on the host -> (tok [R], accept [n_sfx], keep [R], n_kept [1]), int32:
        the greedy id of every row (``argmax_rows``), per suffix the number of leading rows whose id
        equals their draft token, and the kept rows (rows 0 .. accept of every suffix, in suffix
        order) in ``keep[:n_kept]`` (lookup.verify_rows: the same entries)."""
        if probs.dim() != 2:
            raise TypeError("probs must be a [rows, V] tensor")
        rows = probs.shape[0]
        if row_start.dtype != torch.int32 or draft.dtype != torch.int32 or draft.numel() != rows:
            raise TypeError(f"row_start and draft must be int32 vectors (draft: {rows} entries)")
        dev = probs.device
        tok = self.argmax_rows(probs)                 # (the rule of this backend's greedy token)
        t, rs, dr = tok.cpu().numpy(), row_start.cpu().numpy(), draft.cpu().numpy()
        n = rs.shape[0] - 1
        accept = np.zeros(n, dtype=np.int32)
        keep = np.zeros(rows, dtype=np.int32)
        k = 0
        for i in range(n):
            a, r0, r1 = 0, int(rs[i]), int(rs[i + 1])
            while r0 + a < r1 - 1 and t[r0 + a] == dr[r0 + a]:
                a += 1
            accept[i] = a
            if r1 > r0:
                keep[k:k + a + 1] = np.arange(r0, r0 + a + 1)
                k += a + 1
        ctrl = torch.from_numpy(np.concatenate([accept, [k]]).astype(np.int32)).to(dev)   # [accept | n_kept], as HipOps
        return tok, ctrl[:n], torch.from_numpy(keep).to(dev), ctrl[n:]

    def softmax(self, logits: torch.Tensor, logits_scaling: float = 1.0) -> torch.Tensor:
        if logits_scaling != 1.0:                            # Granite: logits / logits_scaling
            logits = logits / logits_scaling
        return torch.softmax(logits.float(), dim=-1).to(torch.float16)

    def synchronize(self):
        pass

    def dequant_fp8(self, region: torch.Tensor, numel: int, scale: torch.Tensor, kind: int, cols: int) -> None:
        """The ``numel`` e4m3fn bytes in the upper half of the ``2 * numel``-byte ``region`` -> fp16 in
        place, by the host definition (fp8.dequantize).  ``scale``: flat fp32 of ``kind`` 0 tensor /
        1 channel / 2 block128 of the ``[numel / cols, cols]`` tensor."""
        from .. import fp8
        b = region.view(torch.uint8)
        if b.numel() != 2 * numel:
            raise ValueError("the region of an FP8 tensor is 2 bytes per weight")
        rows = numel // cols
        s = scale.detach().to("cpu").reshape(-1)
        if kind == fp8.KIND_CHANNEL:
            s = s.reshape(rows, 1)
        elif kind == fp8.KIND_BLOCK:
            s = s.reshape(-(-rows // fp8.BLOCK), -(-cols // fp8.BLOCK))
        else:
            s = s.reshape(1)
        w = fp8.dequantize(b[numel:].to("cpu").clone().view(rows, cols), s)
        b.view(torch.float16).copy_(w.reshape(-1))

    def lora_merge(self, w: torch.Tensor, a: torch.Tensor, bs: torch.Tensor, r: int) -> None:
        """``w`` (fp16 ``[rows, cols]``) += the adapter, in place, by the host definition
        (lora.merge_reference): ``a`` fp32 ``[R, cols]``, ``bs`` fp32 ``[rows, R]`` with the scale
        folded in, both padded with +0 to ``R`` = ``r`` rounded up to a multiple of 4."""
        from .. import lora
        lora.check_merge_args(w, a, bs, r)
        out = lora.merge_reference(w.detach().to("cpu"), a[:r].to("cpu"), bs[:, :r].to("cpu"), None)
        w.copy_(torch.from_numpy(out).to(w.device))

    def dequant_int4(self, region: torch.Tensor, numel: int, group: int, scale_dtype: torch.dtype) -> None:
        """The INT4 tensor of ``numel`` weights that landed in its ``2 * numel``-byte ``region``
        (int4.region_layout) -> fp16 in place, by the host definition (int4.dequantize)."""
        from .. import int4
        b = region.view(torch.uint8)
        if b.numel() != 2 * numel:
            raise ValueError("the region of an INT4 tensor is 2 bytes per weight")
        if numel == 0:
            return
        es = torch.empty((), dtype=scale_dtype).element_size()
        words, scales = int4.unland(b.to("cpu"), numel, group, es)
        rows = numel // group                      # (one row per group: the value depends on nothing else)
        w = int4.dequantize(words.view(torch.int32).view(rows, group // 8), scales.view(scale_dtype).view(rows, 1),
                            (rows, group))
        b.view(torch.float16).copy_(w.reshape(-1))

    def dequant_nf4(self, region: torch.Tensor, numel: int, block: int, absmax_kind: int, code: torch.Tensor,
                    code2=None, nested_absmax=None, nested_block: int = 0, offset: float = 0.0) -> None:
        """The bitsandbytes 4-bit tensor of ``numel`` weights that landed in its ``2 * numel``-byte
        ``region`` (nf4.region_layout) -> fp16 in place, by the host definition (nf4.dequantize)."""
        from .. import nf4
        b = region.view(torch.uint8)
        if b.numel() != 2 * numel:
            raise ValueError("the region of an NF4 tensor is 2 bytes per weight")
        if numel == 0:
            return
        u8 = absmax_kind == nf4.ABSMAX_U8
        packed, raw = nf4.unland(b.to("cpu"), numel, block, 1 if u8 else 4)
        w = nf4.dequantize(packed, code, raw if u8 else raw.view(torch.float32), (numel // block, block), block,
                           code2, nested_absmax, nested_block, offset)
        b.view(torch.float16).copy_(w.reshape(-1))

    def dequant_mxfp4(self, region: torch.Tensor, numel: int) -> None:
        """The MXFP4 tensor of ``numel`` weights that landed in its ``2 * numel``-byte ``region``
        (mxfp4.region_layout) -> fp16 in place, by the host definition (mxfp4.dequantize)."""
        from .. import mxfp4
        b = region.view(torch.uint8)
        if b.numel() != 2 * numel:
            raise ValueError("the region of an MXFP4 tensor is 2 bytes per weight")
        if numel == 0:
            return
        packed, scales = mxfp4.unland(b.to("cpu"), numel, mxfp4.BLOCK, mxfp4.SCALE_ES)
        rows = numel // mxfp4.BLOCK                # (one row per block: the value depends on nothing else)
        w = mxfp4.dequantize(packed.view(rows, mxfp4.BLOCK // 2), scales.view(rows, 1), (rows, mxfp4.BLOCK))
        b.view(torch.float16).copy_(w.reshape(-1))

    def dequant_gptq(self, region: torch.Tensor, out: int, inn: int, group: int, layout: str) -> None:
        """The GPTQ / AWQ (``layout``) weight ``[out, inn]`` whose qweight, scales and qzeros landed at
        the bottom of its ``2 * out * inn``-byte ``region`` (gptq.input_layout) -> fp16 in place, by the
        host definition (gptq.dequantize)."""
        from .. import gptq
        b = region.view(torch.uint8)
        if b.numel() != 2 * out * inn:
            raise ValueError("the region of a GPTQ / AWQ tensor is 2 bytes per weight")
        qweight, scales, qzeros = gptq.unland(b.to("cpu"), out, inn, group, layout)
        b.view(torch.float16).copy_(gptq.dequantize(qweight, qzeros, scales, layout).reshape(-1))

    # ------------------------------------------------------- synthetic init
    def fill_layer_random(self, buf: torch.Tensor, layout, seed: int, std: float = 0.02) -> None:
        """Random-init one packed layer in place (norm weights ~ 1, embeddings ~ N(0,1))."""
        g = torch.Generator(device=buf.device).manual_seed(int(seed))
        views = layout.views(buf, torch.float16)
        for name, v in views.items():
            mean, sd = fill_params(name, std)
            v.copy_(torch.randn(v.shape, generator=g, device=buf.device) * sd + mean)


def fill_params(slot_name: str, std: float):
    """(mean, std) of the synthetic distribution of a packed slot."""
    if slot_name in ("ln1", "ln2", "norm", "qn", "kn"):
        return 1.0, 0.1
    if slot_name == "embed":
        return 0.0, 1.0
    if slot_name in ("bqkv", "bo"):
        return 0.0, 10 * std
    return 0.0, std
