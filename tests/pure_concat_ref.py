"""Plain-torch restatement of the pure-concatenation mixin ("MoT via pure concatenation", modded-nanogpt/runs/711_*.py:224-232,
call site 314-316):

    x = norm(cat([E_tok[t], E_byte[b_0], ..., E_byte[b_{bpt-1}]], -1)),   norm(x) = F.rms_norm(x, (x.size(-1),))

with the variants the fused kernel accepts and the reference's fixture cannot cover: per-embedding norms and learned scalars (as
runs/71041 and 71081 apply them to the SUM mixin) and two id tensors (byte part E_byte[a] + E_byte[b], normalised as a sum when
norm_byte is set: FlexibleEmbedding's padded_and_pulled mode, train_gpt.py:371-379).  Nothing here comes from the reference; the
restatement is checked in float64 against the reference's own outputs in tests/golden/pure_concat.npz (tools/gen_golden_pure_concat.py
wrote them), and the GPU tests then use it in float64 as the exact result for shapes the fixture does not hold.

Inputs are regenerated from seeds (numpy's legacy RandomState); the integer inputs (tokens, byte ids before and after the pull)
are stored in the fixture, since producing them needs the oracle's pull.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

import golden_inputs as gi

GOLDEN = Path(__file__).resolve().parent / "golden" / "pure_concat.npz"

# name: (tok_dim, byte_dim, bpt, B, T, token vocab, two id tensors, seed)
CASES = {
    "d64_b4_bpt16": (64, 4, 16, 3, 16, 40, False, 7110),       # 48 tokens; EOT at a row start, in the middle, twice in a row
    "d512_b32_bpt16": (512, 32, 16, 1, 12, 16, False, 7111),   # run 711's own dims
    "d24_b8_bpt8": (24, 8, 8, 2, 20, 40, False, 7112),         # a token part that is no multiple of 64 columns, model_dim 88
    "d64_b4_bpt4": (64, 4, 4, 2, 16, 40, False, 7113),
    "d64_b4_bpt16_two_ids": (64, 4, 16, 2, 16, 40, True, 7114),  # byte part E[padded] + E[pulled]
}
QUANTITIES = ("out", "d_tok", "d_byte")


def case_tokens(name: str) -> np.ndarray:
    """Token ids with the EOT token (vocab - 1) at a row start, in the middle of a row and twice in a row."""
    Dt, Db, bpt, B, T, Vt, dual, seed = CASES[name]
    rs = np.random.RandomState(seed)
    toks = rs.randint(0, Vt - 1, size=(B, T)).astype(np.int32)
    toks[rs.random_sample((B, T)) < 0.1] = 0      # tokens without a valid byte (row 0 of the synthetic table)
    e = Vt - 1
    toks[0, 0] = e
    toks[0, T // 2] = e
    toks[B - 1, 3] = e
    toks[B - 1, 4] = e
    return toks


def case_ttb(name: str) -> np.ndarray:
    Dt, Db, bpt, B, T, Vt, dual, seed = CASES[name]
    return gi.synth_ttb(seed + 1, Vt, bpt, "left")


def case_tables(name: str):
    """(token table, byte table, upstream gradient) as float64 numpy arrays whose values are exactly representable in float32."""
    Dt, Db, bpt, B, T, Vt, dual, seed = CASES[name]
    f = lambda a: a.astype(np.float32).astype(np.float64)
    g = np.random.RandomState(seed + 4).standard_normal((B, T, Dt + bpt * Db))
    return f(gi.normal_table(seed + 2, Vt, Dt)), f(gi.normal_table(seed + 3, gi.BYTE_VOCAB, Db)), f(g)


def key(name: str, what: str) -> str:
    return f"{name}/{what}"


def load_golden():
    return np.load(GOLDEN)


def norm(x: torch.Tensor, eps: float | None) -> torch.Tensor:
    return F.rms_norm(x, (x.size(-1),), eps=eps)


def forward(tokens, ids_a, ids_b, Et, Eb, *, bpt: int, norm_tok=False, norm_byte=False, norm_out=True, scale_tok=None, scale_byte=None,
            eps: float | None = None) -> torch.Tensor:
    """tokens (B, T) int, ids_* (B, T*bpt) int (ids_b optional); Et / Eb / scale_* torch tensors of one floating dtype.
    eps None = torch.finfo(dtype).eps, as F.rms_norm(eps=None); the kernels use the float32 (or bfloat16) one: pass it."""
    tokens, ids_a = torch.as_tensor(tokens).long(), torch.as_tensor(ids_a).long()
    B, T = tokens.shape
    a = Et[tokens]                                              # (B, T, Dt)
    b = Eb[ids_a.reshape(B, T, bpt)]                            # (B, T, bpt, Db)
    if ids_b is not None:
        b = b + Eb[torch.as_tensor(ids_b).long().reshape(B, T, bpt)]
    if norm_tok:
        a = norm(a, eps)
    if norm_byte:
        b = norm(b, eps)
    if scale_tok is not None:
        a = a * scale_tok
    if scale_byte is not None:
        b = b * scale_byte
    x = torch.cat([a, b.reshape(B, T, bpt * Eb.shape[1])], dim=-1)
    return norm(x, eps) if norm_out else x


def run(tokens, ids_a, ids_b, Et, Eb, g, *, bpt: int, dtype=torch.float64, scale_tok=None, scale_byte=None, **kw) -> dict:
    """Forward and autograd with the upstream gradient g; numpy in, numpy out ("out", "d_tok", "d_byte", and "d_scale_tok" /
    "d_scale_byte" when the scalars are given as Python floats)."""
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    Et_, Eb_ = t(Et).requires_grad_(True), t(Eb).requires_grad_(True)
    st = None if scale_tok is None else t(scale_tok).requires_grad_(True)
    sb = None if scale_byte is None else t(scale_byte).requires_grad_(True)
    x = forward(tokens, ids_a, ids_b, Et_, Eb_, bpt=bpt, scale_tok=st, scale_byte=sb, **kw)
    x.backward(t(g).reshape(x.shape))
    r = {"out": x.detach().numpy(), "d_tok": Et_.grad.numpy(), "d_byte": Eb_.grad.numpy()}
    if st is not None:
        r["d_scale_tok"] = float(st.grad)
    if sb is not None:
        r["d_scale_byte"] = float(sb.grad)
    return r


def rel_err(got, ref) -> float:
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))
