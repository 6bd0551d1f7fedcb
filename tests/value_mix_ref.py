"""Plain-torch restatement of the mixture-of-tokenizers value embeddings (modded-nanogpt/runs/9_mot-in_mot-valemb.py: mixin_bytes
225-235, parameters 252-254, call site 310-313; runs 3 and 6 alike).  For every slot j:

    u_j[n] = cat(Vt_j[tok_n], Vb_j[ids[n, 0]], ..., Vb_j[ids[n, bpt-1]])      K = token_dim + bpt * byte_dim, per-token byte order
    ve_j[n] = norm(F.linear(u_j[n], W_j))                                    W_j (out_dim, K), no bias; norm(x) = F.rms_norm(x, (x.size(-1),))

in any floating dtype, one sequence (row of the batch) at a time as the run's forward takes them.  Run in bfloat16 it rounds where the
reference's bfloat16 run rounds, because it is made of the same torch operations: the linear's result (sums in fp32) and the normalised
row (rms factor in fp32).  Nothing here comes from the reference; the restatement is checked against the reference's own outputs and
gradients in tests/golden/value_mix.npz (tools/gen_golden_value_mix.py wrote them), and the GPU tests then use it in float64 as the
exact result for shapes the fixture does not hold.

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
from byte_fc_ref import bf16_values, init_byte_fc, rel_err  # noqa: F401  (the same helpers: bf16-valued float64, init_linear, largest difference over largest element)

GOLDEN = Path(__file__).resolve().parent / "golden" / "value_mix.npz"
F32_EPS = float(np.finfo(np.float32).eps)   # the kernels' epsilon for both dtypes (MotValueMixDesc.eps <= 0)

# name: (token_dim, byte_dim, bpt, out_dim, B, T, slots, token vocab, standard deviation of the tables, seed)
CASES = {
    "t32_b8_bpt8": (32, 8, 8, 32, 2, 24, 3, 40, 1.0, 9001),          # V1: EOT at a row start, mid-row and twice in a row
    "t64_b24_bpt4": (64, 24, 4, 64, 2, 24, 2, 40, 1.0, 9002),        # V2: K = 160, widths that are multiples of neither 64 nor 128
    "t32_b8_bpt16": (32, 8, 16, 32, 2, 24, 1, 40, 1.0, 9003),        # the runs' bpt: mixin_bytes as it stands in the run
    "t32_b8_bpt8_small": (32, 8, 8, 32, 2, 24, 1, 40, 0.02, 9004),   # rows of magnitude 0.01: where the float32 and bfloat16 epsilons differ
}
QUANTITIES = ("out", "d_tok", "d_byte", "d_weight")


def case_tokens(name: str) -> np.ndarray:
    """Token ids with the EOT token (vocab - 1) at a row start, in the middle of a row and twice in a row (as byte_fc_ref.case_tokens)."""
    Dt, Db, bpt, Do, B, T, S, Vt, std, seed = CASES[name]
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
    Dt, Db, bpt, Do, B, T, S, Vt, std, seed = CASES[name]
    return gi.synth_ttb(seed + 1, Vt, bpt, "left")


def make_inputs(seed: int, Vt: int, Dt: int, Db: int, bpt: int, Do: int, B: int, T: int, slots: int, std: float = 1.0, byte_rows: int = gi.BYTE_VOCAB):
    """Per slot (token value table, byte value table, mixin weight, upstream gradient): float64 arrays of bfloat16 values; the
    weight as the runs' init_linear draws it (uniform in +-sqrt(3) * 0.5 / sqrt(K))."""
    out = []
    for j in range(slots):
        s = seed + 10 * j
        g = np.random.RandomState(s + 4).standard_normal((B, T, Do))
        out.append((bf16_values(std * gi.normal_table(s + 2, Vt, Dt)), bf16_values(std * gi.normal_table(s + 3, byte_rows, Db)),
                    bf16_values(init_byte_fc(s + 5, Do, Dt + bpt * Db)), bf16_values(g)))
    return out


def case_tables(name: str):
    Dt, Db, bpt, Do, B, T, S, Vt, std, seed = CASES[name]
    return make_inputs(seed, Vt, Dt, Db, bpt, Do, B, T, S, std)


def key(name: str, what: str) -> str:
    return f"{name}/{what}"


def load_golden():
    return np.load(GOLDEN)


def forward(tokens, ids, Vt, Vb, W, *, bpt: int, norm_out: bool = True, eps: float | None = None) -> torch.Tensor:
    """One slot.  tokens (B, T) int, ids (B, T*bpt) int in per-token byte order; Vt / Vb / W torch tensors of one floating dtype.
    eps None = what F.rms_norm(eps=None) takes for that dtype.  Row by row, each as a (1, T, K) batch: the shapes of the run's forward."""
    tokens, ids = torch.as_tensor(tokens).long(), torch.as_tensor(ids).long()
    B, T = tokens.shape
    rows = []
    for b in range(B):
        u = torch.cat([Vt[tokens[b]][None], Vb[ids[b].reshape(T, bpt)].reshape(1, T, bpt * Vb.shape[1])], dim=-1)
        y = F.linear(u, W)
        rows.append(F.rms_norm(y, (y.size(-1),), eps=eps) if norm_out else y)
    return torch.cat(rows, dim=0)


def run(tokens, ids, slots, *, bpt: int, dtype=torch.float64, **kw) -> list:
    """Forward and autograd for every slot (Vt, Vb, W, g) of `slots`; numpy in, a list of dicts of float64 numpy out: "out", "d_tok",
    "d_byte", "d_weight"."""
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64).to(dtype)
    n = lambda a: a.detach().double().numpy()
    res = []
    for Vt, Vb, W, g in slots:
        Vt_, Vb_, W_ = t(Vt).requires_grad_(True), t(Vb).requires_grad_(True), t(W).requires_grad_(True)
        x = forward(tokens, ids, Vt_, Vb_, W_, bpt=bpt, **kw)
        x.backward(t(g).reshape(x.shape))
        res.append({"out": n(x), "d_tok": n(Vt_.grad), "d_byte": n(Vb_.grad), "d_weight": n(W_.grad)})
    return res
