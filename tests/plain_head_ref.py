"""A torch restatement of the plain cross-entropy head, the loss of the reference's two loops without a softcap, run eagerly with
autograd in any dtype on any device:
    mathblations/model.py:337-338 + main.py:294-303 (evaluation :164-187): F.rms_norm(x); lm_head(x).float(); the scored window of
                                                      each sequence (slice_logits_and_targets); F.cross_entropy; argmax accuracies
    inference/inference.py:349-359:                   lm_head(hidden_states); shift; CrossEntropyLoss()  (ignore_index -100)
Both are F.cross_entropy(F.linear(norm(x), W).float(), y, ignore_index=...) with the mean over the kept targets: a window is the
same loss as marking every other position ignored.  The GPU tests use head() in float64 as the reference, in float32 as the eager
path whose own error sets the bar of the large-logit cases, and in bfloat16 (lm_head's output rounded to bf16, then .float(), as
the reference rounds) as the eager path whose own error sets the bf16 bar.  tests/golden/plain_head.npz
(tools/gen_golden_plain_head.py) holds the reference's own outputs for the small cases below; test_plain_head_capi.py checks this
file against them."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

IGNORE = -100
FLT_EPS = float(torch.finfo(torch.float32).eps)   # the fused call's epsilon in every dtype: F.rms_norm(eps=None) on fp32 and bf16 inputs
B, T, DIM = 4, 16, 32          # the fixture's shape
VOCABS = (128, 256)
KINDS = ("math", "infer")      # mathblations (norm, windows) and inference (no norm, shifted labels with -100)


def kept_mask(t: torch.Tensor, vocab: int, ignore_index: int = IGNORE) -> torch.Tensor:
    return (t >= 0) & (t < vocab) & (t != ignore_index)


def head(x, w, targets, norm_in=True, dtype=torch.float64, ignore_index=IGNORE, eps=FLT_EPS):
    """Eager forward + backward in `dtype` (the weight cast to it, as lm_head in bf16 is; the logits then .float(), or kept in float64).
    eps: the norm's; None is F.rms_norm's own choice, which in float64 is 2.2e-16 (the fixture's float64 run) and matters on rows
    whose mean square is tiny.
    A target outside [0, vocab) is dropped like an ignored one.  Returns dict(loss, dx, dW) in float64; with no kept row the loss is
    NaN, as F.cross_entropy's, and the gradients are returned as zeros."""
    f64 = dtype == torch.float64
    xd = x.detach().to(dtype).clone().requires_grad_(True)
    wd = w.detach().to(torch.float64 if f64 else torch.float32).clone().requires_grad_(True)
    h = F.rms_norm(xd, (xd.size(-1),), eps=eps) if norm_in else xd
    logits = F.linear(h, wd.type_as(h))
    logits = (logits if f64 else logits.float()).reshape(-1, wd.shape[0])
    t = targets.reshape(-1).long()
    t = torch.where(kept_mask(t, wd.shape[0], ignore_index), t, torch.full_like(t, IGNORE))
    loss = F.cross_entropy(logits, t, ignore_index=IGNORE)
    f = lambda a: a.detach().double()
    if not bool((t != IGNORE).any()):
        return {"loss": f(loss), "dx": torch.zeros_like(xd).double(), "dW": torch.zeros_like(wd).double()}
    loss.backward()
    return {"loss": f(loss), "dx": f(xd.grad), "dW": f(wd.grad)}


def rows(s: torch.Tensor, c: torch.Tensor, targets: torch.Tensor, ignore_index: int = IGNORE):
    """The evaluation's rows from stored products s [N, V] (as the call stored them, any float dtype) and row factors c [N]:
    row_loss = lse(c s) - (c s)[y] in float64 (0 for a dropped row), pred = the lowest class of the largest stored product,
    rank = the number of stored products above the target's (-1 for a dropped row)."""
    s64 = s.double()
    t = targets.reshape(-1).long()
    keep = kept_mask(t, s.shape[1], ignore_index)
    tc = torch.where(keep, t, torch.zeros_like(t))
    l = s64 * c.double()[:, None]
    row_loss = torch.where(keep, torch.logsumexp(l, -1) - l.gather(1, tc[:, None])[:, 0], torch.zeros_like(l[:, 0]))
    top = s64.max(-1, keepdim=True).values
    cls = torch.arange(s.shape[1], device=s.device)
    pred = torch.where(s64 == top, cls, torch.full_like(cls, s.shape[1])).min(-1).values
    rank = torch.where(keep, (s64 > s64.gather(1, tc[:, None])).sum(-1), torch.full_like(t, -1))
    return row_loss, pred.int(), rank.int()


def counts(pred: torch.Tensor, targets: torch.Tensor, vocab: int, group_rows: int = 0, ignore_index: int = IGNORE):
    """[kept rows, kept rows with pred == target] and, with group_rows, the groups with a kept row whose kept rows are all right."""
    t = targets.reshape(-1).long()
    keep = kept_mask(t, vocab, ignore_index)
    hit = keep & (pred.reshape(-1).long() == t)
    out = [int(keep.sum()), int(hit.sum())]
    if group_rows:
        k, h = keep.reshape(-1, group_rows), hit.reshape(-1, group_rows)
        out.append(int((k.any(-1) & (h | ~k).all(-1)).sum()))
    return out


def case_inputs(kind: str, vocab: int):
    """Seeded inputs of one fixture case.
    "math":  x [B, T, DIM] fp32, W [vocab, DIM] fp32, y_tokens [B, T] int64, y_indices [B, 2] int64 (the scored window of each
             sequence).  Sequence 0's window holds the float64 argmax everywhere (a fully right sequence), about half of the other
             windows' targets are the argmax, the rest random; targets outside the windows are random tokens, as in the reference.
    "infer": hidden [B, T, DIM] fp32 (taken as already normed), W, labels [B, T] int64 with -100 entries (the prompt of each
             sequence and some scattered positions), None."""
    rng = np.random.default_rng(4100 + 10 * KINDS.index(kind) + vocab)
    x = rng.standard_normal((B, T, DIM)).astype(np.float32)
    w = (rng.standard_normal((vocab, DIM)) * 0.7).astype(np.float32)
    y = rng.integers(0, vocab, (B, T)).astype(np.int64)
    if kind == "math":
        h = x.astype(np.float64)
        h = h / np.sqrt((h * h).mean(-1, keepdims=True) + np.finfo(np.float32).eps)
        best = (h @ w.astype(np.float64).T).argmax(-1)
        start = rng.integers(1, T - 5, B)
        idx = np.stack([start, start + rng.integers(2, 5, B)], 1).astype(np.int64)
        take = rng.random((B, T)) < 0.5
        take[0] = True
        y = np.where(take, best, y)
        return tuple(torch.from_numpy(a) for a in (x, w, y, idx))
    x *= 0.8
    for b in range(B):
        y[b, : 2 + b] = IGNORE
    y[rng.random((B, T)) < 0.15] = IGNORE
    y[1, T - 1] = IGNORE
    return torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(y), None


def case_key(kind: str, vocab: int, dtype: str, what: str) -> str:
    return f"{kind}_v{vocab}_{dtype}_{what}"
