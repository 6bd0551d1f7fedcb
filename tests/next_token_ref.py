"""Plain-torch float64 restatement of mot_next_token's rules on given logits (include/mot.h, MotNextTokenDesc), for the tests.

Per row: masses exp((l - max) / temperature); top-k keeps l >= the k-th largest value (ties stay); top-p keeps, among the survivors, a
class when the mass of the STRICTLY larger logits is <= top_p of the survivors' mass, so a tie group stays whole (the one place where
the call pins what torch.sort leaves open); greedy takes the largest logit, the lowest class on ties; the draw takes the first kept
class, in ascending class order, whose running mass exceeds u * Z, else the last kept class.  -0 counts as +0."""
from typing import NamedTuple

import torch

U_MAX = 1.0 - 2.0 ** -24


class RefStep(NamedTuple):
    token: torch.Tensor      # int64 [n], -1 for a row with a NaN or +inf logit (or no finite logit)
    prob: torch.Tensor       # float64 [n]
    kept: torch.Tensor       # int64 [n]
    probs: torch.Tensor      # float64 [n, V]: the filtered distribution
    keep: torch.Tensor       # bool [n, V]
    top_cls: torch.Tensor    # int64 [n, n_top], -1 past the kept count
    top_prob: torch.Tensor   # float64 [n, n_top], 0 past the kept count


def strictly_larger_mass(l, mass):
    """G[r, v] = the sum of mass[r, w] over the classes w with l[r, w] > l[r, v]."""
    sl, order = torch.sort(l, dim=1, descending=True, stable=True)
    sm = mass.gather(1, order)
    before = torch.cumsum(sm, dim=1) - sm                                      # mass in front of each sorted position
    first = torch.searchsorted((-sl).contiguous(), (-sl).contiguous(), right=False)   # where the position's tie group starts
    g_sorted = before.gather(1, first)
    return torch.empty_like(g_sorted).scatter_(1, order, g_sorted)


def next_token_ref(logits, *, temperature=1.0, top_k=0, top_p=1.0, greedy=False, u=None, n_top=0) -> RefStep:
    l = logits.detach().double() + 0.0
    n, V = l.shape
    bad = torch.isnan(l).any(1) | (l == float("inf")).any(1) | (l == float("-inf")).all(1)
    l = torch.where(bad[:, None], torch.zeros_like(l), l)   # a bad row is computed on zeros and overwritten below
    m = l.max(dim=1, keepdim=True).values
    e = torch.exp((l - m) / float(temperature))
    keep = torch.ones_like(l, dtype=torch.bool)
    if 0 < top_k < V:
        keep = l >= torch.topk(l, int(top_k), dim=1).values[:, -1:]
    if top_p < 1.0:
        mass = e * keep
        lk = torch.where(keep, l, torch.full_like(l, float("-inf")))
        keep = keep & (strictly_larger_mass(lk, mass) <= float(top_p) * mass.sum(1, keepdim=True))
    mass = e * keep
    Z = mass.sum(1, keepdim=True)
    probs = mass / Z
    kept = keep.sum(1)
    cls = torch.arange(V, device=l.device)
    lk = torch.where(keep, l, torch.full_like(l, float("-inf")))
    if greedy:
        token = torch.argmax((lk == lk.max(1, keepdim=True).values).to(torch.int8), dim=1)   # the lowest class of the maximum
    else:
        uu = torch.nan_to_num(u.detach().double().reshape(n, 1), nan=0.0).clamp(0.0, U_MAX)
        cross = (torch.cumsum(mass, dim=1) > uu * Z) & keep
        last = torch.where(keep, cls, torch.full_like(cls, -1)).max(1).values
        token = torch.where(cross.any(1), torch.argmax(cross.to(torch.int8), dim=1), last)
    prob = probs.gather(1, token[:, None])[:, 0]
    # the largest filtered probabilities: descending logit, the lowest class first on ties (a stable sort of ascending classes)
    order = torch.sort(lk, dim=1, descending=True, stable=True).indices[:, :n_top]
    valid = torch.arange(n_top, device=l.device)[None, :] < kept[:, None]
    top_cls = torch.where(valid, order, torch.full_like(order, -1))
    top_prob = torch.where(valid, probs.gather(1, order), torch.zeros_like(order, dtype=torch.float64))
    token = torch.where(bad, torch.full_like(token, -1), token)
    prob = torch.where(bad, torch.full_like(prob, float("nan")), prob)
    kept = torch.where(bad, torch.zeros_like(kept), kept)
    top_cls = torch.where(bad[:, None], torch.full_like(top_cls, -1), top_cls)
    top_prob = torch.where(bad[:, None], torch.zeros_like(top_prob), top_prob)
    return RefStep(token, prob, kept, probs, keep, top_cls, top_prob)


def eager_logits(x, weight, norm_in, dtype):
    """lm_head on the rows of x in `dtype`, as the reference's modules would run it (F.rms_norm with eps=None, then F.linear)."""
    import torch.nn.functional as F
    h = x.to(dtype)
    if norm_in:
        h = F.rms_norm(h, (h.shape[-1],))
    return F.linear(h, weight.to(dtype))
