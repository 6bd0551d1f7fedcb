"""Plain-torch restatement of the token value embeddings (scaled-pre-train/train_gpt.py:566 and :600; modded-nanogpt/runs/
71_*_toks-valemb.py:247 and :303):

    ve_j = T_j[tokens]                                  j = 0 .. n-1, every T_j of shape (vocab, dim), one token tensor
    dT_j[r] = sum of g_j[n] over the positions n with tokens[n] == r

in any floating dtype.  Nothing here comes from the reference; the restatement is checked against the reference's own float64
gradients in tests/golden/value_embeds.npz (tools/gen_golden_value_embeds.py wrote them), and the GPU tests then use it in float64
as the exact result for shapes the fixture does not hold.

Float inputs are regenerated from seeds (numpy's legacy RandomState) and rounded to bfloat16 values, so that the float64, float32
and bfloat16 runs of a case see the same numbers and differ in their arithmetic only; the tokens are stored in the fixture.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

import golden_inputs as gi

GOLDEN = Path(__file__).resolve().parent / "golden" / "value_embeds.npz"

# name: (vocab, dim, token shape, tables, kind of ids, seed)
CASES = {
    "v50_d4_one": (50, 4, (1,), 1, "uniform", 6001),            # one position, one table
    "v97_d8_n65": (97, 8, (65,), 3, "uniform", 6002),           # one more position than a wave's slice of the sorted stream
    "v40_d16_skewed": (40, 16, (2, 96), 3, "skewed", 6003),     # FineWeb-shaped: a few ids take most positions
    "v10_d8_hot": (10, 8, (300,), 2, "hot", 6004),              # one hot group: every id 3 except ten
    "v100_d32_ends": (100, 32, (3, 50), 2, "ends", 6005),       # a (B, T) token tensor whose ids are only 0 and vocab - 1
}


def bf16_values(a: np.ndarray) -> np.ndarray:
    """float64 array of the bfloat16 roundings (nearest-even) of `a`."""
    return torch.tensor(np.asarray(a, dtype=np.float32)).bfloat16().double().numpy()


def make_tokens(seed: int, vocab: int, shape, kind: str) -> np.ndarray:
    """int32 ids of the given shape: "uniform", "skewed" (golden_inputs.fineweb_like_tokens: the most frequent id takes
    vocab^(-1/3) of the positions), "hot" (every id 3 except ten positions), "perm" (a permutation of 0 .. n-1: every group of
    size one; needs n == vocab), "ends" (only 0 and vocab - 1)."""
    n = int(np.prod(shape))
    rs = np.random.RandomState(seed)
    if kind == "uniform":
        t = rs.randint(0, vocab, size=n)
    elif kind == "skewed":
        t = gi.fineweb_like_tokens(seed, 1, n, vocab=vocab).reshape(-1)
    elif kind == "hot":
        t = np.full(n, 3 % vocab)
        at = rs.choice(n, size=min(10, n), replace=False)
        t[at] = rs.randint(0, vocab, size=at.size)
    elif kind == "perm":
        assert n == vocab
        t = rs.permutation(n)
    elif kind == "ends":
        t = np.where(rs.random_sample(n) < 0.5, 0, vocab - 1)
    else:
        raise ValueError(kind)
    return t.astype(np.int32).reshape(shape)


def make_inputs(seed: int, vocab: int, dim: int, shape, n_tables: int):
    """(tables, upstream gradients): n_tables (vocab, dim) tables and shape + (dim,) gradients, float64 arrays of bfloat16 values"""
    tables = [bf16_values(gi.normal_table(seed + 10 + j, vocab, dim)) for j in range(n_tables)]
    gs = [bf16_values(np.random.RandomState(seed + 20 + j).standard_normal(tuple(shape) + (dim,))) for j in range(n_tables)]
    return tables, gs


def case_tokens(name: str) -> np.ndarray:
    vocab, dim, shape, n, kind, seed = CASES[name]
    return make_tokens(seed, vocab, shape, kind)


def case_inputs(name: str):
    vocab, dim, shape, n, kind, seed = CASES[name]
    return make_inputs(seed, vocab, dim, shape, n)


def key(name: str, what: str) -> str:
    return f"{name}/{what}"


def load_golden():
    return np.load(GOLDEN)


def run(tokens, tables, gs, *, dtype=torch.float64, device="cpu") -> dict:
    """Forward and autograd with the upstream gradients gs (None: that output takes no part in the backward); numpy in, float64
    numpy out: "out" and "d_table", a list each (d_table[j] None where gs[j] is None)."""
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64).to(dtype).to(device)
    tok = torch.as_tensor(np.asarray(tokens)).long().to(device)
    tabs = [t(a).requires_grad_(True) for a in tables]
    outs = [tab[tok] for tab in tabs]
    live = [(o, t(g).reshape(o.shape)) for o, g in zip(outs, gs) if g is not None]
    if live:
        torch.autograd.backward([o for o, _ in live], [g for _, g in live])
    n = lambda a: None if a is None else a.detach().double().cpu().numpy()
    return {"out": [n(o) for o in outs], "d_table": [n(tb.grad) for tb in tabs]}


def rel_err(got, ref) -> float:
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))
