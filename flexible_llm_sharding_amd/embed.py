"""Pooled final hidden states per suffix (``--score_mode embed``): the definition.

For suffix ``s`` of a prompt let ``y_t`` (``t = 0 .. n-1``) be the final-norm rows of the suffix's
``n`` tokens: the rows ``ops.rmsnorm`` writes with ``model.norm``'s weight (fp16 on the GPU, HF's
cast points; fp32 on the CPU backend).  With ``H`` the hidden size the embedding ``e`` is

* ``pooling="last"``: ``e = float32(y_{n-1})`` — the row the LM head scores in the next-token mode;
* ``pooling="mean"``: ``e[c] = (sum_t float32(y_t[c])) / n`` over the suffix's own tokens (the prefix
  is the instruction or context: its rows are not pooled);
* ``dim=D`` (1..H; 0 = H): the first ``D`` columns are kept (Matryoshka truncation);
* ``normalize``: ``e / max(||e||_2, 1e-12)`` over the kept columns, in fp32
  (``torch.nn.functional.normalize``: an all-zero vector stays zero).

Summation order (``csrc/kernels/pooling.hip``; ``tests/embed_ref.py`` emulates it in float32):

* the mean of a column is ``((..((y_0 + y_1) + y_2) ..) + y_{n-1}) / n``: fp32 additions in row
  order starting from row 0 itself, then one fp32 division by ``float32(n)``.  ``last`` is the same
  rule on the one row ``y_{n-1}`` (``y / 1``: the row's own bits);
* the squared norm of the ``D`` kept fp32 values: thread ``t`` of 256 adds ``e[c]^2`` (one fused
  multiply-add each) for ``c = t, t + 256, ...`` in ascending order starting from 0; the 64 threads of a
  wave combine by the xor butterfly ``v += v[lane ^ o]`` for ``o = 32, 16, 8, 4, 2, 1``; the 4 wave
  sums are added in wave order starting from 0; then ``e[c] / max(sqrt(sum), 1e-12)``.

Both are functions of the suffix's rows alone, so a suffix's embedding does not depend on the other
suffixes of the call, on how the call is split into micro-batches or on the launch grid.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List

POOLINGS = ("last", "mean")
NORM_EPS = 1e-12


@dataclass(frozen=True)
class EmbedParams:
    pooling: str = "last"
    dim: int = 0                 # 0: the hidden size
    normalize: bool = True

    def resolved(self, hidden_size: int) -> "EmbedParams":
        """Validated against the model: ``dim`` in 1..H (0 -> H)."""
        check_embed_values(self.pooling, self.dim)
        d = int(self.dim) or int(hidden_size)
        if d > hidden_size:
            raise ValueError(f"--embed_dim must be in 1..{hidden_size} (the hidden size), got {d}")
        return EmbedParams(self.pooling, d, bool(self.normalize))

    @classmethod
    def from_args(cls, args) -> "EmbedParams":
        return cls(getattr(args, "embed_pooling", None) or "last", int(getattr(args, "embed_dim", None) or 0),
                   True if getattr(args, "embed_normalize", None) is None else bool(args.embed_normalize))


def check_embed_values(pooling, dim) -> None:
    if pooling not in POOLINGS:
        raise ValueError(f"--embed_pooling must be one of {POOLINGS}, got {pooling!r}")
    if isinstance(dim, bool) or int(dim) != dim or dim < 0:
        raise ValueError(f"--embed_dim must be an integer >= 0 (0: the hidden size), got {dim!r}")


def layer_names(cfg, score_mode: str = "next_token") -> List[str]:
    """The layers a runner of ``score_mode`` plans, loads and runs: ``cfg.layer_names()``, which
    in embed mode ends at ``model.norm`` (the LM head need not exist on disk)."""
    names = cfg.layer_names()
    return names[:-1] if score_mode == "embed" else names
