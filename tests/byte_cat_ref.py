"""Plain-torch restatement of the bytes-only front-end and the byte value embeddings (modded-nanogpt/runs/5_bytes-in_bytes-valemb.py:
reshape_bytes 225-232, value embeddings 248 and 305, x0 at 314):

    out_j[n] = norm_j?(cat_k T_j[ids[n, k]])      model_dim = bpt * byte_dim columns, no token row;  norm(x) = F.rms_norm(x, (x.size(-1),))

for 1..4 tables T_j over one id stream, in any floating dtype.  Run in bfloat16 it rounds where the reference's bfloat16 run rounds:
once, at the normalised row (rms factor in fp32); rows without a norm are copies.  Nothing here comes from the reference; the
restatement is checked against the reference's own outputs and gradients in tests/golden/byte_cat.npz (tools/gen_golden_byte_cat.py
wrote them), and the GPU tests then use it in float64 as the exact result for shapes the fixture does not hold.

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

GOLDEN = Path(__file__).resolve().parent / "golden" / "byte_cat.npz"
F32_EPS = float(np.finfo(np.float32).eps)   # the kernels' epsilon for both dtypes (MotByteCatDesc.eps <= 0)
BF16_EPS = 2.0 ** -7

# name: (byte_dim, bpt, B, T, token vocab, norm flag per table, standard deviation of the tables, seed)
CASES = {
    "b4_bpt16_n4": (4, 16, 2, 12, 40, (True, False, False, False), 1.0, 5001),   # run 5's four outputs; byte_dim 4: float32 only on the device
    "b8_bpt16_n4": (8, 16, 2, 8, 40, (True, False, False, False), 1.0, 5002),    # the same in a width bfloat16 takes
    "b48_bpt8_n1": (48, 8, 1, 12, 40, (True,), 1.0, 5003),                       # one table (runs 4, 6); slots that are no power of two wide
    "b64_bpt4_n1": (64, 4, 1, 12, 40, (True,), 1.0, 5004),                       # run 5's byte_dim
    "b8_bpt8_n2_small": (8, 8, 1, 12, 40, (True, True), 0.02, 5005),             # rows of magnitude 0.02: where the float32 and bfloat16 epsilons differ
}


def bf16_values(a: np.ndarray) -> np.ndarray:
    """float64 array of the bfloat16 roundings (nearest-even) of `a`."""
    return torch.tensor(np.asarray(a, dtype=np.float32)).bfloat16().double().numpy()


def case_tokens(name: str) -> np.ndarray:
    """Token ids with the EOT token (vocab - 1) at a row start, in the middle of a row and twice in a row."""
    Db, bpt, B, T, Vt, norm, std, seed = CASES[name]
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
    Db, bpt, B, T, Vt, norm, std, seed = CASES[name]
    return gi.synth_ttb(seed + 1, Vt, bpt, "left")


def make_inputs(seed: int, rows, Db: int, bpt: int, B: int, T: int, std: float = 1.0):
    """(tables, upstream gradients): one (rows_j, Db) table and one (B, T, bpt * Db) gradient per entry of `rows`, float64 arrays
    of bfloat16 values"""
    tables = [bf16_values(std * gi.normal_table(seed + 10 + j, r, Db)) for j, r in enumerate(rows)]
    gs = [bf16_values(np.random.RandomState(seed + 20 + j).standard_normal((B, T, bpt * Db))) for j in range(len(rows))]
    return tables, gs


def case_tables(name: str):
    Db, bpt, B, T, Vt, norm, std, seed = CASES[name]
    return make_inputs(seed, [gi.BYTE_VOCAB] * len(norm), Db, bpt, B, T, std)


def key(name: str, what: str) -> str:
    return f"{name}/{what}"


def load_golden():
    return np.load(GOLDEN)


def forward(ids, tables, norm, *, bpt: int, eps: float | None = None) -> list:
    """ids (B, T*bpt) int; tables torch tensors (rows_j, Db) of one floating dtype; a bool per table.  eps None = what
    F.rms_norm(eps=None) takes for that dtype; the kernels use the float32 epsilon for both dtypes: pass F32_EPS."""
    ids = torch.as_tensor(ids).long()
    B, T = ids.shape[0], ids.shape[1] // bpt
    outs = []
    for tab, nm in zip(tables, norm):
        x = tab[ids.to(tab.device).reshape(B, T, bpt)].reshape(B, T, bpt * tab.shape[1])
        outs.append(F.rms_norm(x, (x.size(-1),), eps=eps) if nm else x)
    return outs


def run(ids, tables, norm, gs, *, bpt: int, dtype=torch.float64, device="cpu", **kw) -> dict:
    """Forward and autograd with the upstream gradients gs (None: that output takes no part in the backward); numpy in, float64
    numpy out: "out" and "d_table", a list each (d_table[j] None where gs[j] is None)."""
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64).to(dtype).to(device)
    tabs = [t(a).requires_grad_(True) for a in tables]
    outs = forward(ids, tabs, norm, bpt=bpt, **kw)
    live = [(o, t(g).reshape(o.shape)) for o, g in zip(outs, gs) if g is not None]
    if live:
        torch.autograd.backward([o for o, _ in live], [g for _, g in live])
    n = lambda a: None if a is None else a.detach().double().cpu().numpy()
    return {"out": [n(o) for o in outs], "d_table": [n(tb.grad) for tb in tabs]}


def rel_err(got, ref) -> float:
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))
