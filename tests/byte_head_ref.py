"""A torch restatement of the byte output head of a mixout run (scaled-pre-train/train_gpt.py:483-527, 618-623 with identity
ByteSelfAttn layers), run eagerly with autograd in any dtype on any device.  The GPU tests use it in float64 as the reference and
in float32 / bfloat16 as the eager path whose own error sets the bf16 bar.  tests/golden/byte_head.npz (tools/gen_golden_byte_head.py)
holds the reference's own outputs for small cases; test_byte_head_capi.py checks this file against them."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

VOCAB = 512            # next_multiple_of_n(458, n=128)
N_TOKENS, BPT = 16, 8  # the fixture's cases
DIMS = {"copy": 16, "split": 128}
LAYERS = (0, 1, 2)
HEAD_EPS = 2.0 ** -23  # the head's epsilon in every dtype (kHeadEps): what F.rms_norm(eps=None) takes in fp32, not in float64


def byte_states(x: torch.Tensor, method: str, bpt: int, n_layer_out: int, eps=None) -> torch.Tensor:
    """ByteMixoutCopy / ByteMixoutSplit.forward with identity layers: x (..., T, D) -> (..., T*bpt, D or D/bpt).  `eps` goes to every
    F.rms_norm: None is the dtype's own (2.2e-16 in float64), HEAD_EPS the head's, which rows near zero need."""
    if method == "copy":
        h = x.repeat_interleave(bpt, dim=-2)
    else:
        h = x.reshape(*x.shape[:-2], x.shape[-2] * bpt, x.shape[-1] // bpt)
    for _ in range(n_layer_out):
        h = h + F.rms_norm(h, (h.size(-1),), eps=eps)
    return h


def head(x, w, targets, method, bpt, n_layer_out, dtype=torch.float64, drop=None, eps=None):
    """Eager forward + backward in `dtype` (the weight cast to it, as CastedLinear does; logits softcapped in fp32 or float64).
    Returns dict(states, loss, dx, dW) in float64.  `drop`: flat indices of targets whose terms leave the sum (denominator M);
    `eps` as in byte_states."""
    xd = x.detach().to(dtype).clone().requires_grad_(True)
    wd = w.detach().to(torch.float64 if dtype == torch.float64 else torch.float32).clone().requires_grad_(True)
    h = byte_states(xd, method, bpt, n_layer_out, eps)
    logits = F.linear(F.rms_norm(h, (h.size(-1),), eps=eps), wd.type_as(h))
    z = 30 * torch.sigmoid((logits.double() if dtype == torch.float64 else logits.float()) / 7.5)
    z = z.reshape(-1, z.size(-1))
    t = targets.reshape(-1).long()
    if drop is None:
        loss = F.cross_entropy(z, t)
    else:
        keep = torch.ones_like(t, dtype=torch.bool)
        keep[drop] = False
        per = F.cross_entropy(z[keep], t[keep], reduction="sum")
        loss = per / t.numel()
    loss.backward()
    f = lambda a: a.detach().double()
    return {"states": f(h), "loss": f(loss), "dx": f(xd.grad), "dW": f(wd.grad)}


def case_inputs(method: str, n_layer_out: int):
    """Seeded inputs of one fixture case: x [N_TOKENS, D] fp32, W [512, K] fp32 (CastedLinear's init), targets int64 [N_TOKENS*BPT]."""
    D = DIMS[method]
    K = D if method == "copy" else D // BPT
    rng = np.random.default_rng(1000 + 10 * (method == "split") + n_layer_out)
    x = rng.standard_normal((N_TOKENS, D)).astype(np.float32)
    bound = (3 ** 0.5) * 0.5 * K ** -0.5
    w = rng.uniform(-bound, bound, (VOCAB, K)).astype(np.float32)
    t = rng.integers(0, 458, N_TOKENS * BPT).astype(np.int64)
    t[rng.random(t.shape) < 0.3] = 456   # pad-heavy, like real targets
    return torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(t)


def case_key(method: str, n_layer_out: int, dtype: str, what: str) -> str:
    return f"{method}_L{n_layer_out}_{dtype}_{what}"
