"""GPU tests of the generation step (mot_next_token / functional.next_token / PlainLMHead.next_token).

Decisions are judged on the call's OWN logits output: the float64 restatement of tests/next_token_ref.py runs on the returned logits,
so the product's rounding cannot move a boundary, and token, kept and top_cls must then be exactly equal.  Inputs are built to have
margin, and the tests assert the margins on their inputs:
  W = randn * 3 / sqrt(D): every size has classes holding at least 1e-3 of the mass;
  top_p sits in a gap between two consecutive boundaries (the masses of the strictly larger logits) that is at least 1e-3 wide in
  EVERY row of the call, at least 1e-4 from both ends; the kernel's masses differ from float64 by about 1e-6 relative (fp32 exp) and
  by their rounding up to multiples of 2^-44;
  each u is the middle of the CDF interval of a kept class holding at least 1e-3, or 0 (the first kept class), or 1 (clamped: the last).
Logits: the error relative to the largest float64 logit is at most twice that of the eager restatement in the same dtype on the same
inputs, floor 1e-6 (DESIGN section 8's rule); prob and top_prob: the same rule against float64 on the returned logits, relative to the
row's largest probability, the eager side being an fp32 softmax of the filtered logits.
In fp32 the row pass keeps rows up to 32 768 classes in registers (bf16: 65 536), so 32 896 and 65 664 are the first re-read sizes."""
import math

import pytest
import torch

import mixture_of_tokenizers_amd as mot
import next_token_ref as nr
from mixture_of_tokenizers_amd import _capi as capi
from mixture_of_tokenizers_amd.modules import PlainLMHead

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BOTH = [torch.float32, torch.bfloat16]
MASS, GAP, EDGE = 1e-3, 1e-3, 1e-4


def clear_status():
    capi.status_word(DEV).zero_()


def status():
    return int(capi.status_word(DEV).item())


def make(V, D, n, dtype, seed=0):
    """W (V, D) = randn * 3 / sqrt(D), and x (n, D) as the last position of a (n, 3, D) tensor: a strided view."""
    g = torch.Generator().manual_seed(1000 * seed + V + 7 * D + n)
    w = (torch.randn(V, D, generator=g) * 3.0 / math.sqrt(D)).to(dtype).to(DEV)
    hidden = torch.randn(n, 3, D, generator=g).to(dtype).to(DEV)
    x = hidden[:, -1, :]
    assert n == 1 or not x.is_contiguous()
    return x, w


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def filtered(L, T, top_k):
    """float64 on the logits L: the survivors of top-k, their normalised masses and the mass of the strictly larger logits."""
    l = L.double() + 0.0
    V = l.shape[1]
    keep = torch.ones_like(l, dtype=torch.bool)
    if 0 < top_k < V:
        keep = l >= torch.topk(l, top_k, dim=1).values[:, -1:]
    mass = torch.exp((l - l.max(1, keepdim=True).values) / T) * keep
    mass = mass / mass.sum(1, keepdim=True)
    G = nr.strictly_larger_mass(torch.where(keep, l, torch.full_like(l, float("-inf"))), mass)
    return keep, mass, G


def pick_top_p(L, T, top_k, nominal):
    """The float32 top_p nearest `nominal` that has margin in every row, and asserts that one exists."""
    keep, mass, G = filtered(L, T, top_k)
    n, V = G.shape
    Gs = torch.sort(torch.where(keep, G, torch.full_like(G, 2.0)), dim=1).values        # the boundaries of each row, ascending
    ends = torch.cat([Gs[:, 1:], torch.full((n, 1), 2.0, device=G.device, dtype=G.dtype)], dim=1).clamp(max=1.0)
    wide = (ends - Gs >= GAP) & (Gs <= 1.0)
    mids = ((Gs + ends) / 2)[wide]
    cand = torch.cat([mids.flatten()[:8192], torch.tensor([nominal], device=G.device, dtype=G.dtype)]).float().double()
    cand = cand[(cand > 0) & (cand < 1)]
    idx = torch.searchsorted(Gs, cand[None, :].expand(n, -1).contiguous(), right=True)   # boundaries <= p: at least the maximum's 0
    below = Gs.gather(1, idx - 1)
    above = torch.where(idx < V, Gs.gather(1, idx.clamp(max=V - 1)), torch.ones_like(below)).clamp(max=1.0)
    ok = (above - below >= GAP) & ((cand[None, :] - below >= EDGE) | (below == 0)) & (above - cand[None, :] >= EDGE)
    ok = ok.all(0)
    assert bool(ok.any()), f"no top_p with margin near {nominal}"
    best = cand[ok][torch.argmin((cand[ok] - nominal).abs())]
    return float(best)


def pick_u(probs, keep):
    """One u per row, cycling through: the middle of the CDF interval of a kept class holding >= 1e-3, 0, and 1."""
    n, V = probs.shape
    cdf = torch.cumsum(probs, dim=1)
    u = torch.zeros(n, dtype=torch.float64)
    for r in range(n):
        kind = r % 3 if n > 1 else 0
        if kind == 0:
            big = torch.nonzero((probs[r] >= MASS) & keep[r])[:, 0]
            assert big.numel() > 0, f"row {r}: no kept class holds {MASS}"
            c = int(big[(7 * r + 3) % big.numel()])
            u[r] = float(cdf[r, c] - probs[r, c] / 2)
            assert float(probs[r, c]) >= MASS
        elif kind == 2:
            u[r] = 1.0
    return u.float().to(probs.device)


def tolerance(err_eager):
    return max(2.0 * err_eager, 1e-6)


def check_logits(L, x, w, norm_in, dtype):
    ref = nr.eager_logits(x.double(), w.double(), norm_in, torch.float64)
    eager = nr.eager_logits(x, w, norm_in, dtype).double()
    scale = float(ref.abs().max())
    err_eager, err = float((eager - ref).abs().max()) / scale, float((L.double() - ref).abs().max()) / scale
    print(f"logits: error {err:.3e}, eager {err_eager:.3e}")
    assert err <= tolerance(err_eager), (err, err_eager)


def check_probs(out, ref, L, T):
    """prob and top_prob against float64 on the returned logits, relative to the row's largest probability."""
    eager = torch.softmax(torch.where(ref.keep, L.float() / T, torch.full_like(L, float("-inf")).float()), dim=1).double()
    top = ref.probs.max(1).values
    err_eager = float(((eager - ref.probs).abs().max(1).values / top).max())
    good = ref.token >= 0
    err = float(((out.prob.double() - ref.prob).abs() / top)[good].max())
    assert torch.isfinite(out.prob[good]).all()
    if out.top_prob is not None:
        err = max(err, float(((out.top_prob.double() - ref.top_prob).abs().max(1).values / top)[good].max()))
    print(f"probs: error {err:.3e}, eager {err_eager:.3e}")
    assert err <= tolerance(err_eager), (err, err_eager)


def compare(out, ref, L, T):
    assert torch.equal(out.logits, L)   # the same stored logits on every call
    assert torch.equal(out.token, ref.token), (out.token, ref.token)
    assert torch.equal(out.kept.long(), ref.kept)
    if out.top_cls is not None:
        assert torch.equal(out.top_cls.long(), ref.top_cls)
    check_probs(out, ref, L, T)


def run_case(V, D, n, dtype, norm_in, T, top_k, p_nominal, seed=0, x=None, w=None, logits_rule=True):
    if x is None:
        x, w = make(V, D, n, dtype, seed)
    clear_status()
    kw = dict(norm_in=norm_in, temperature=T, top_k=top_k)
    first = mot.next_token(x, w, greedy=True, return_logits=True, n_top=3, **kw)   # no top-p yet: its value is picked on these logits
    L = first.logits
    assert L.shape == (n, V) and L.dtype == torch.float32
    if logits_rule:
        check_logits(L, x, w, norm_in, dtype)
    compare(first, nr.next_token_ref(L, temperature=T, top_k=top_k, greedy=True, n_top=3), L, T)
    top_p = 1.0 if p_nominal >= 1 else pick_top_p(L, T, top_k, p_nominal)
    base = nr.next_token_ref(L, temperature=T, top_k=top_k, top_p=top_p, greedy=True)
    u = pick_u(base.probs, base.keep)
    out = mot.next_token(x, w, top_p=top_p, u=u, n_top=5, return_logits=True, **kw)
    ref = nr.next_token_ref(L, temperature=T, top_k=top_k, top_p=top_p, u=u, n_top=5)
    compare(out, ref, L, T)
    greedy = mot.next_token(x, w, top_p=top_p, greedy=True, n_top=8, return_logits=True, **kw)
    compare(greedy, nr.next_token_ref(L, temperature=T, top_k=top_k, top_p=top_p, greedy=True, n_top=8), L, T)
    assert status() == 0
    return out, ref, top_p


# (V, D, n, norm_in, T, top_k, nominal top_p); top_k: 1, 50, V - 1, >= V; top_p: very small, 0.5, 0.9, 1; every n and V in both dtypes
CASES = [
    (128, 16, 1, False, 1.0, 0, 1.0),
    (128, 16, 3, True, 0.7, 50, 0.5),
    (128, 64, 17, False, 1.5, 127, 0.9),
    (128, 64, 70, True, 1.0, 128, 1e-6),
    (4224, 16, 16, False, 0.7, 1, 0.5),
    (4224, 64, 17, True, 1.0, 50, 0.9),
    (4224, 64, 70, False, 1.5, 4223, 0.5),
    (4224, 2048, 1, True, 1.0, 50, 0.5),
    (4224, 2048, 16, False, 0.7, 0, 0.9),
    (4224, 2048, 17, True, 1.5, 5000, 1e-6),
    (32768, 64, 3, False, 1.0, 50, 0.9),
    (32768, 16, 16, True, 0.7, 32767, 0.5),
    (32896, 64, 1, True, 1.0, 50, 0.5),
    (32896, 16, 17, False, 1.5, 0, 1.0),
    (65536, 64, 1, False, 0.7, 50, 0.9),
    (65536, 16, 70, True, 1.0, 65535, 1e-6),
    (65664, 64, 3, True, 1.5, 50, 0.5),
    (65664, 16, 16, False, 1.0, 1, 1.0),
    (262144, 64, 1, False, 1.0, 50, 0.9),
    (262144, 16, 3, True, 0.7, 262143, 0.5),
    (262144, 64, 16, True, 1.5, 0, 1e-6),
    (262144, 16, 17, False, 1.0, 50, 0.5),
    (262144, 64, 70, False, 0.7, 300000, 0.9),
]


@pytest.mark.parametrize("dtype", BOTH, ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=[f"V{c[0]}-D{c[1]}-n{c[2]}-k{c[5]}-p{c[6]}" for c in CASES])
def test_decisions_logits_and_probabilities(case, dtype):
    V, D, n, norm_in, T, top_k, p = case
    run_case(V, D, n, dtype, norm_in, T, top_k, p)


def integer_inputs(V, D, n, dtype, seed):
    """x in {-1, 0, 1}^D and W in {-1, 0, 1}: exact integer logits with many equal ones, in both dtypes."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-1, 2, (n, D), generator=g).to(dtype).to(DEV)
    w = torch.randint(-1, 2, (V, D), generator=g).to(dtype).to(DEV)
    return x, w


@pytest.mark.parametrize("dtype", BOTH, ids=["fp32", "bf16"])
@pytest.mark.parametrize("V,D,n", [(4224, 16, 6), (65664, 64, 17)])
def test_ties_on_every_boundary(V, D, n, dtype):
    x, w = integer_inputs(V, D, n, dtype, V + n)
    x[1] = 0   # a row of equal logits; its u is 0
    rest = torch.arange(n, device=x.device) != 1
    out, ref, top_p = run_case(V, D, n, dtype, False, 1.0, 40, 0.5, x=x, w=w, logits_rule=False)
    L = out.logits
    assert torch.equal(L, nr.eager_logits(x.double(), w.double(), False, torch.float64).float())   # exact integers
    assert torch.equal(L, L.round()) and float(L[1].abs().max()) == 0.0
    # the row of equal logits: everything stays under both cuts, the draw at u = 0 and greedy return class 0
    g = mot.next_token(x, w, top_k=40, top_p=top_p, greedy=True, n_top=2)
    assert int(g.token[1]) == 0 and int(g.kept[1]) == V and g.top_cls[1].tolist() == [0, 1]
    assert int(out.token[1]) == 0 and int(out.kept[1]) == V
    # a tie group at the maximum (greedy took its lowest class) and one on the top-k boundary, in some row
    at_max = (L == L.max(1, keepdim=True).values).sum(1)
    assert int(at_max[rest].max()) >= 2
    assert torch.equal(g.token, torch.argmax((L == L.max(1, keepdim=True).values).to(torch.int8), dim=1))
    only_k = nr.next_token_ref(L, top_k=40, greedy=True)
    assert int((only_k.kept[rest] > 40).sum()) >= 1
    # and one on the top-p boundary: the last kept value of a row is shared by several classes, of which the call kept every one
    lk = torch.where(ref.keep, L.double(), torch.full_like(L, float("inf")).double())
    lowest = lk.min(1, keepdim=True).values
    members = (L.double() == lowest).sum(1)
    assert int((members[rest] >= 2).sum()) >= 1
    assert torch.equal(((L.double() == lowest) & ref.keep).sum(1), members)


def test_bf16_random_logits_tie_on_the_top_k_boundary():
    V, k = 4224, 300   # logits around 4.5, where bf16 values lie 2^-5 apart and some six classes share each
    x, w = make(V, 64, 3, torch.bfloat16, seed=5)
    out, ref, _ = run_case(V, 64, 3, torch.bfloat16, True, 1.0, k, 1.0, x=x, w=w)
    assert int((ref.kept > k).sum()) >= 1   # bf16 logits repeat: the k-th value is shared


@pytest.mark.parametrize("dtype", BOTH, ids=["fp32", "bf16"])
def test_nan_and_inf_rows_leave_their_neighbours_alone(dtype):
    V, D, n = 4224, 64, 5
    x, w = make(V, D, n, dtype, seed=9)
    x = x.contiguous()
    clear_status()
    good = mot.next_token(x, w, top_k=50, greedy=True, n_top=3, return_logits=True)
    assert status() == 0
    xb = x.clone()
    xb[1] = float("nan")
    xb[3] = 3.0e38 * torch.sign(w[7]).masked_fill(w[7] == 0, 1.0)   # the product with class 7 overflows to +inf
    u = torch.full((n,), 0.25, device=DEV)
    for greedy in (True, False):
        clear_status()
        out = mot.next_token(xb, w, top_k=50, greedy=greedy, u=None if greedy else u, n_top=3, return_logits=True)
        torch.cuda.synchronize()
        assert status() == capi.STATUS_LOGIT_NONFINITE
        with pytest.raises(IndexError, match="NaN or \\+inf"):
            mot.check_status()
        assert status() == 0
        assert torch.isnan(out.logits[1]).all() and bool((out.logits[3] == float("inf")).any())
        assert out.token[[1, 3]].tolist() == [-1, -1] and torch.isnan(out.prob[[1, 3]]).all() and out.kept[[1, 3]].tolist() == [0, 0]
        assert out.top_cls[[1, 3]].eq(-1).all() and out.top_prob[[1, 3]].eq(0).all()
        ok = [0, 2, 4]
        ref = nr.next_token_ref(out.logits, top_k=50, greedy=greedy, u=u, n_top=3)
        assert ref.token[[1, 3]].tolist() == [-1, -1]
        assert torch.equal(out.token, ref.token) and torch.equal(out.kept.long(), ref.kept) and torch.equal(out.top_cls.long(), ref.top_cls)
        if greedy:   # bit-equal to the call without the bad rows
            for name in ("token", "prob", "kept", "top_cls", "top_prob", "logits"):
                assert torch.equal(getattr(out, name)[ok], getattr(good, name)[ok]), name


@pytest.mark.parametrize("dtype", BOTH, ids=["fp32", "bf16"])
def test_logits_of_plus_and_minus_300(dtype):
    V, D, n = 4224, 64, 3
    x, w = integer_inputs(V, D, n, dtype, 77)
    x = torch.where(x == 0, torch.ones_like(x), x) * 5      # entries +-5: |l| <= 320
    w[11] = torch.sign(x[0])                                 # row 0 reaches +320 at class 11 and -320 at class 12
    w[12] = -torch.sign(x[0])
    out, ref, _ = run_case(V, D, n, dtype, False, 1.0, 0, 0.5, x=x, w=w, logits_rule=False)
    assert float(out.logits[0, 11]) == 320.0 and float(out.logits[0, 12]) == -320.0
    assert torch.isfinite(out.prob).all() and torch.isfinite(out.top_prob).all()
    assert int(out.kept[0]) == 1 and int(out.token[0]) == 11


@pytest.mark.parametrize("dtype", BOTH, ids=["fp32", "bf16"])
@pytest.mark.parametrize("V,n", [(4224, 16), (65664, 17)])
def test_two_runs_give_the_same_bits(V, n, dtype):
    x, w = make(V, 64, n, dtype, seed=3)
    u = torch.rand(n, generator=torch.Generator().manual_seed(4)).to(DEV)
    runs = [mot.next_token(x, w, norm_in=True, temperature=0.8, top_k=100, top_p=0.7, u=u, n_top=8, return_logits=True) for _ in range(3)]
    for other in runs[1:]:
        for name in mot.NextToken._fields:
            assert torch.equal(getattr(runs[0], name), getattr(other, name)), name
    # the module on (B, T, D) is the functional call on the sliced rows; without u it draws its own numbers on the device
    head = PlainLMHead(torch.nn.Linear(64, V, bias=False), norm_in=True).to(DEV)
    with torch.no_grad():
        head.lm_head.weight.copy_(w)
    hidden = torch.randn(n, 3, 64, generator=torch.Generator().manual_seed(6)).to(dtype).to(DEV)
    a = head.next_token(hidden, temperature=0.8, top_k=100, top_p=0.7, u=u, n_top=4)
    b = mot.next_token(hidden[:, -1, :].contiguous(), w, norm_in=True, temperature=0.8, top_k=100, top_p=0.7, u=u, n_top=4)
    for name in ("token", "prob", "kept", "top_cls", "top_prob"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(head.next_token(hidden[:, -1, :], greedy=True).token, mot.next_token(hidden[:, -1, :], w, norm_in=True, greedy=True).token)
    own = head.next_token(hidden, top_k=5)
    assert own.token.shape == (n,) and bool(((own.token >= 0) & (own.token < V)).all()) and bool((own.kept >= 5).all())
    assert mot.next_token(hidden[:0, -1, :], w, greedy=True).token.shape == (0,)


@pytest.mark.parametrize("dtype", BOTH, ids=["fp32", "bf16"])
@pytest.mark.parametrize("V,n", [(4224, 3), (65664, 17)])
def test_capture_and_replay_on_inputs_changed_in_place(V, n, dtype):
    D = 64
    gen = torch.Generator().manual_seed(V + n)
    w = (torch.randn(V, D, generator=gen) * 3.0 / math.sqrt(D)).to(dtype).to(DEV)
    hidden = torch.randn(n, 2, D, generator=gen).to(dtype).to(DEV)
    u = torch.rand(n, generator=gen).to(DEV)
    kw = dict(norm_in=True, temperature=0.9, top_k=64, top_p=0.8, n_top=4, return_logits=True)

    def step():
        return mot.next_token(hidden[:, -1, :], w, u=u, **kw)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    clear_status()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for i in range(3):
        with torch.no_grad():
            hidden.copy_(torch.randn(n, 2, D, generator=gen).to(dtype))
            u.copy_(torch.rand(n, generator=gen))
            if i == 2:
                w.mul_(0.5)
        graph.replay()
        torch.cuda.synchronize()
        eager = step()
        for name in mot.NextToken._fields:
            assert torch.equal(getattr(out, name), getattr(eager, name)), (i, name)
        ref = nr.next_token_ref(out.logits, temperature=0.9, top_k=64, top_p=0.8, u=u, n_top=4)
        assert torch.equal(out.kept.long() >= 1, ref.kept >= 1) and bool(((out.token >= 0) & (out.token < V)).all())
    assert status() == 0
