"""A torch restatement of the token-level output head, the last five lines of the reference's training scripts, run eagerly with
autograd in any dtype on any device:
    scaled-pre-train/train_gpt.py:619-623 with byte_mixout_method "noop": norm, lm_head (CastedLinear), 30 sigmoid(l.float() / 7.5),
                                                                          cross_entropy over the flattened rows
    modded-nanogpt/runs/71_mot-in_toks-valemb.py:331-334 (and the other runs): norm, F.linear with the weight in bf16, .float(),
                                                                          15 l rsqrt(l^2 + 225), cross_entropy
The GPU tests use it in float64 as the reference and in bfloat16 as the eager path whose own error sets the bf16 bar.
tests/golden/token_head.npz (tools/gen_golden_token_head.py) holds the reference's own outputs for the small cases below;
test_token_head_capi.py checks this file against them."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

SOFTCAPS = ("sigmoid30", "rsqrt15")
VOCAB, DIM, ROWS = 384, 64, 40   # the fixture's shape: next_multiple_of_n(300, n=128) classes


def softcap(l: torch.Tensor, kind: str) -> torch.Tensor:
    if kind == "sigmoid30":
        return 30 * torch.sigmoid(l / 7.5)              # train_gpt.py:622
    if kind == "rsqrt15":
        return 15 * l * torch.rsqrt(l.square() + 225)   # runs/71_*.py:334
    raise ValueError(kind)


def head(x, w, targets, kind, norm_in=True, dtype=torch.float64, drop=None):
    """Eager forward + backward in `dtype` (the weight cast to it, as CastedLinear and lm_head_w.bfloat16() do; the logits
    softcapped in fp32, or in float64 when dtype is float64).  Returns dict(loss, dx, dW) in float64.
    `drop`: flat indices of rows whose terms leave the sum (the denominator stays the row count)."""
    xd = x.detach().to(dtype).clone().requires_grad_(True)
    wd = w.detach().to(torch.float64 if dtype == torch.float64 else torch.float32).clone().requires_grad_(True)
    h = F.rms_norm(xd, (xd.size(-1),)) if norm_in else xd
    logits = F.linear(h, wd.type_as(h))
    z = softcap(logits.double() if dtype == torch.float64 else logits.float(), kind)
    z = z.reshape(-1, z.size(-1))
    t = targets.reshape(-1).long()
    if drop is None:
        loss = F.cross_entropy(z, t)
    else:
        keep = torch.ones_like(t, dtype=torch.bool)
        keep[drop] = False
        loss = F.cross_entropy(z[keep], t[keep], reduction="sum") / t.numel()
    loss.backward()
    f = lambda a: a.detach().double()
    return {"loss": f(loss), "dx": f(xd.grad), "dW": f(wd.grad)}


def case_inputs(kind: str, norm_in: bool):
    """Seeded inputs of one fixture case: x [ROWS, DIM] fp32, W [VOCAB, DIM] fp32 filled (the reference zeroes lm_head at init;
    a zero weight tests nothing), targets int64 [ROWS] with the first, the last real and the last padded class among them."""
    rng = np.random.default_rng(2000 + 10 * SOFTCAPS.index(kind) + int(norm_in))
    x = rng.standard_normal((ROWS, DIM)).astype(np.float32) * (1.0 if norm_in else 0.8)
    w = (rng.standard_normal((VOCAB, DIM)) * 1.5).astype(np.float32)   # std(l) ~ 12 with norm_in: well into the curved part of both caps
    t = rng.integers(0, VOCAB, ROWS).astype(np.int64)
    t[:4] = (0, 299, VOCAB - 1, 0)
    return torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(t)


def case_key(kind: str, norm_in: bool, dtype: str, what: str) -> str:
    return f"{kind}_n{int(norm_in)}_{dtype}_{what}"
