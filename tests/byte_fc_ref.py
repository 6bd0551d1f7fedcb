"""Plain-torch restatement of the linear-on-bytes mixin (modded-nanogpt/runs/71051_*.py:225-229, parameter at 253, call site 312-314):

    u_n = cat_k E_byte[ids[n, k]]                       K = bpt * byte_dim columns, per-token byte order
    x_n = norm(E_tok[tok_n] + F.linear(u_n, byte_fc))   byte_fc (model_dim, K), no bias; norm(x) = F.rms_norm(x, (x.size(-1),))

in any floating dtype.  Run in bfloat16 it rounds where the reference's bfloat16 run rounds, because it is made of the same torch
operations: the linear's result (sums in fp32), the sum with the token row, and the normalised row (rms factor in fp32).  Nothing here
comes from the reference; the restatement is checked against the reference's own outputs and gradients in tests/golden/byte_fc.npz
(tools/gen_golden_byte_fc.py wrote them), and the GPU tests then use it in float64 as the exact result for shapes the fixture does
not hold.

Float inputs are regenerated from seeds (numpy's legacy RandomState) and rounded to bfloat16 values, so that the float64, float32 and
bfloat16 runs of a case see the same numbers and differ in their arithmetic only; the integer inputs (tokens, byte ids before and after
the pull) are stored in the fixture, since producing them needs the oracle's pull.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

import golden_inputs as gi

GOLDEN = Path(__file__).resolve().parent / "golden" / "byte_fc.npz"
F32_EPS = float(np.finfo(np.float32).eps)   # the kernels' epsilon for both dtypes (MotByteFcMixDesc.eps <= 0)

# name: (model_dim, byte_dim, bpt, B, T, token vocab, standard deviation of the tables, seed)
CASES = {
    "m64_b8_bpt8": (64, 8, 8, 2, 24, 40, 1.0, 71051),         # K == model_dim; EOT at a row start, mid-row and twice in a row
    "m128_b8_bpt16": (128, 8, 16, 2, 24, 128, 1.0, 71052),    # run 71051's bpt
    "m96_b24_bpt4": (96, 24, 4, 2, 24, 40, 1.0, 71053),       # widths that are multiples of neither 64 nor 128
    "m64_b4_bpt8": (64, 4, 8, 2, 24, 40, 1.0, 71054),         # K = 32 != model_dim (byte_dim 4: float32 only on the device)
    "m64_b8_bpt8_small": (64, 8, 8, 2, 24, 40, 0.02, 71055),  # rows of magnitude 0.02: where the float32 and bfloat16 epsilons differ
}
QUANTITIES = ("out", "d_tok", "d_byte", "d_byte_fc")


def bf16_values(a: np.ndarray) -> np.ndarray:
    """float64 array of the bfloat16 roundings (nearest-even) of `a`."""
    return torch.tensor(np.asarray(a, dtype=np.float32)).bfloat16().double().numpy()


def case_tokens(name: str) -> np.ndarray:
    """Token ids with the EOT token (vocab - 1) at a row start, in the middle of a row and twice in a row."""
    Dm, Db, bpt, B, T, Vt, std, seed = CASES[name]
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
    Dm, Db, bpt, B, T, Vt, std, seed = CASES[name]
    return gi.synth_ttb(seed + 1, Vt, bpt, "left")


def init_byte_fc(seed: int, Dm: int, K: int) -> np.ndarray:
    """uniform in +-sqrt(3) * 0.5 / sqrt(K): the run's init_linear (runs/71051_*.py:134-137), from numpy's generator"""
    bound = (3 ** 0.5) * 0.5 * (K ** -0.5)
    return np.random.RandomState(seed).uniform(-bound, bound, size=(Dm, K))


def make_inputs(seed: int, Vt: int, Dm: int, Db: int, bpt: int, B: int, T: int, std: float = 1.0):
    """(token table, byte table, byte_fc, upstream gradient): float64 arrays of bfloat16 values"""
    g = np.random.RandomState(seed + 4).standard_normal((B, T, Dm))
    return (bf16_values(std * gi.normal_table(seed + 2, Vt, Dm)), bf16_values(std * gi.normal_table(seed + 3, gi.BYTE_VOCAB, Db)),
            bf16_values(init_byte_fc(seed + 5, Dm, bpt * Db)), bf16_values(g))


def case_tables(name: str):
    Dm, Db, bpt, B, T, Vt, std, seed = CASES[name]
    return make_inputs(seed, Vt, Dm, Db, bpt, B, T, std)


def key(name: str, what: str) -> str:
    return f"{name}/{what}"


def load_golden():
    return np.load(GOLDEN)


def forward(tokens, ids, Et, Eb, W, *, bpt: int, norm_out: bool = True, eps: float | None = None) -> torch.Tensor:
    """tokens (B, T) int, ids (B, T*bpt) int; Et / Eb / W torch tensors of one floating dtype.  eps None = what F.rms_norm(eps=None)
    takes for that dtype; the kernels use the float32 epsilon for both dtypes: pass F32_EPS."""
    tokens, ids = torch.as_tensor(tokens).long(), torch.as_tensor(ids).long()
    B, T = tokens.shape
    u = Eb[ids.reshape(B, T, bpt)].reshape(B, T, bpt * Eb.shape[1])
    s = Et[tokens] + F.linear(u, W)
    return F.rms_norm(s, (s.size(-1),), eps=eps) if norm_out else s


def run(tokens, ids, Et, Eb, W, g, *, bpt: int, dtype=torch.float64, **kw) -> dict:
    """Forward and autograd with the upstream gradient g; numpy in, float64 numpy out: "out", "d_tok", "d_byte", "d_byte_fc"."""
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64).to(dtype)
    Et_, Eb_, W_ = t(Et).requires_grad_(True), t(Eb).requires_grad_(True), t(W).requires_grad_(True)
    x = forward(tokens, ids, Et_, Eb_, W_, bpt=bpt, **kw)
    x.backward(t(g).reshape(x.shape))
    n = lambda a: a.detach().double().numpy()
    return {"out": n(x), "d_tok": n(Et_.grad), "d_byte": n(Eb_.grad), "d_byte_fc": n(W_.grad)}


def as_concat_linear_weight(W) -> np.ndarray:
    """[I | byte_fc]: the weight with which embed_mix(mode="concat_linear") computes the same mixin (the emulation the benchmark's
    baseline uses): W' cat(tok, bytes) = tok + byte_fc bytes."""
    W = np.asarray(W)
    return np.concatenate([np.eye(W.shape[0], dtype=W.dtype), W], axis=1)


def rel_err(got, ref) -> float:
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))
