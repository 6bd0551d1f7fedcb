"""Plain-torch restatement of the three input streams of modded-nanogpt/runs/71081_mot-in_toks-valemb.py:302-304, 315:

    x0t = norm(E_t[tok])                       (T, D)   norm(x) = F.rms_norm(x, (x.size(-1),)), over D = token_dim
    x0b = cat_k norm(E_b[ids[:, k]])           (T, D)   every byte row normalised over byte_dim BEFORE the cat; D = bpt * byte_dim
    x   = x0t * s_t + x0b * s_b                (T, D)   s_t = scalars[-1], s_b = scalars[-2]; no outer norm

in any floating dtype, one sequence (row of the batch) at a time as the run's forward takes them, the byte ids in per-token order (slot
k of every token).  The two scalars stay float32 beside bfloat16 tables, as the run's `scalars` parameter does beside its bfloat16
embeddings: a bfloat16 tensor times a 0-dim float32 tensor is bfloat16, so run in bfloat16 this rounds x0t, x0b, each of the two
products and their sum -- the rounding points of the reference's eager bfloat16 run, because it is made of the same torch operations.
Nothing here comes from the reference; the restatement is checked against the reference's own outputs and gradients in
tests/golden/split_x0.npz (tools/gen_golden_split_x0.py wrote them), and the GPU tests then use it in float64 as the exact result
for shapes the fixture does not hold.

Float inputs are regenerated from seeds (numpy's legacy RandomState) and rounded to bfloat16 values, so that the float64, float32 and
bfloat16 runs of a case see the same numbers and differ in their arithmetic only; the integer inputs (tokens, byte ids after the pull)
are stored in the fixture, since producing them needs the oracle's pull.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

import golden_inputs as gi
from byte_fc_ref import bf16_values, rel_err  # noqa: F401  (bf16-valued float64; largest difference over largest element)

GOLDEN = Path(__file__).resolve().parent / "golden" / "split_x0.npz"
F32_EPS = float(np.finfo(np.float32).eps)   # the kernels' epsilon for both dtypes (MotSplitX0Desc.eps <= 0)
S_TOK, S_BYTE = float(np.float32(0.7)), float(np.float32(-0.3))   # scalars[-1], scalars[-2]: not the initial 0.5, and not equal

# name: (model_dim, byte_dim, bpt, B, T, token vocab, standard deviation of the tables, seed, the output whose gradient is absent)
CASES = {
    "d64_b4_bpt16": (64, 4, 16, 2, 24, 40, 1.0, 8101, None),       # EOT at a row start, mid-row and twice in a row
    "d128_b8_bpt16": (128, 8, 16, 2, 24, 40, 1.0, 8102, "x0b"),    # the smallest shape bf16 takes at bpt 16; no gradient into x0b
    "d96_b24_bpt4": (96, 24, 4, 3, 20, 40, 1.0, 8103, None),       # a byte row of 6 fp32 / 3 bf16 chunks: no power-of-two group of lanes
    "d64_b8_bpt8_small": (64, 8, 8, 2, 24, 40, 0.02, 8104, None),  # rows of magnitude 0.02: the epsilon matters
    "d64_b4_bpt16_one": (64, 4, 16, 1, 1, 40, 1.0, 8105, None),    # one token: what .squeeze() and the cat make of T == 1
}
OUTS = ("x0t", "x0b", "x")
GRADS = ("d_tok", "d_byte", "d_scale_tok", "d_scale_byte")
QUANTITIES = OUTS + GRADS


def case_tokens(name: str) -> np.ndarray:
    """Token ids with the EOT token (vocab - 1) at a row start, in the middle of a row and twice in a row (as byte_fc_ref.case_tokens)."""
    D, Db, bpt, B, T, Vt, std, seed, absent = CASES[name]
    rs = np.random.RandomState(seed)
    toks = rs.randint(0, Vt - 1, size=(B, T)).astype(np.int32)
    toks[rs.random_sample((B, T)) < 0.1] = 0      # tokens without a valid byte (row 0 of the synthetic table)
    e = Vt - 1
    if T >= 8:
        toks[0, 0] = e
        toks[0, T // 2] = e
        toks[B - 1, 3] = e
        toks[B - 1, 4] = e
    return toks


def case_ttb(name: str) -> np.ndarray:
    D, Db, bpt, B, T, Vt, std, seed, absent = CASES[name]
    return gi.synth_ttb(seed + 1, Vt, bpt, "left")


def make_inputs(seed: int, Vt: int, D: int, Db: int, B: int, T: int, std: float = 1.0, byte_rows: int = gi.BYTE_VOCAB, absent=None) -> dict:
    """The two tables and the three upstream gradients (None where absent): float64 arrays of bfloat16 values."""
    g = {w: (None if w == absent else bf16_values(np.random.RandomState(seed + 4 + j).standard_normal((B, T, D)))) for j, w in enumerate(OUTS)}
    return {"tok_table": bf16_values(std * gi.normal_table(seed + 2, Vt, D)), "byte_table": bf16_values(std * gi.normal_table(seed + 3, byte_rows, Db)),
            "g": g}


def case_inputs(name: str) -> dict:
    D, Db, bpt, B, T, Vt, std, seed, absent = CASES[name]
    return make_inputs(seed, Vt, D, Db, B, T, std, absent=absent)


def key(name: str, what: str) -> str:
    return f"{name}/{what}"


def load_golden():
    return np.load(GOLDEN)


def forward(tokens, ids, Et, Eb, s_t, s_b, *, bpt: int, eps: float | None = None):
    """tokens (B, T) int, ids (B, T*bpt) int in per-token byte order; Et / Eb torch tensors of one floating dtype, s_t / s_b 0-dim
    tensors.  eps None = what F.rms_norm(eps=None) takes for that dtype.  Row by row; returns (x0t, x0b, x), each (B, T, D)."""
    tokens, ids = torch.as_tensor(tokens).long(), torch.as_tensor(ids).long()
    B, T = tokens.shape
    Db = Eb.shape[1]
    r0t, r0b, rx = [], [], []
    for b in range(B):
        a = Et[tokens[b]][None]                                        # (1, T, D)
        x0t = F.rms_norm(a, (a.size(-1),), eps=eps)
        u = Eb[ids[b].reshape(T, bpt)]                                 # (T, bpt, Db)
        x0b = F.rms_norm(u, (Db,), eps=eps).reshape(1, T, bpt * Db)    # each byte row on its own, then side by side
        r0t.append(x0t); r0b.append(x0b); rx.append(x0t * s_t + x0b * s_b)
    return torch.cat(r0t, dim=0), torch.cat(r0b, dim=0), torch.cat(rx, dim=0)


def run(tokens, ids, inputs: dict, *, bpt: int, dtype=torch.float64, s_tok: float = S_TOK, s_byte: float = S_BYTE, **kw) -> dict:
    """Forward and autograd; numpy in, a dict of float64 numpy out: the three outputs and the four gradients.  The scalars are
    float64 in the float64 run and float32 otherwise."""
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64).to(dtype)
    n = lambda a: a.detach().double().numpy()
    Et, Eb = t(inputs["tok_table"]).requires_grad_(True), t(inputs["byte_table"]).requires_grad_(True)
    sdt = torch.float64 if dtype == torch.float64 else torch.float32
    s_t, s_b = torch.tensor(s_tok, dtype=sdt, requires_grad=True), torch.tensor(s_byte, dtype=sdt, requires_grad=True)
    outs = dict(zip(OUTS, forward(tokens, ids, Et, Eb, s_t, s_b, bpt=bpt, **kw)))
    pairs = [(outs[w], t(g).reshape(outs[w].shape)) for w, g in inputs["g"].items() if g is not None]
    torch.autograd.backward([o for o, _ in pairs], [g for _, g in pairs])
    res = {w: n(outs[w]) for w in OUTS}
    zero = lambda p: p.grad if p.grad is not None else torch.zeros_like(p)
    res.update(d_tok=n(zero(Et)), d_byte=n(zero(Eb)), d_scale_tok=n(zero(s_t)), d_scale_byte=n(zero(s_b)))   # what no gradient reaches: zero
    return res
