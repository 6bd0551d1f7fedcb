"""-m gpu: the token value embeddings (functional.value_embeds, modules.ValueEmbeds, mot_value_embeds_fwd / _bwd;
scaled-pre-train/train_gpt.py:566, 600 and modded-nanogpt/runs/71_*_toks-valemb.py:247, 303), forward and backward, against the
float64 restatement of tests/value_embeds_ref.py evaluated on the device (which tests/test_value_embeds_capi.py holds to the
reference's own float64 gradients).

Bars:
  * forward: the bits of table[ids], fp32 and bf16;
  * fp32 gradients: max|hip - ref64| <= 2e-5 max|ref64| per tensor, the project's bar (TOL in tests/test_gpu_backward.py).  A
    sequential fp32 sum of a 5 990-term group of N(0, 1) rows is off by 1.7e-6 of the largest element and an eight-way split by
    5.9e-7 (measured on the CPU), so the reference's own arithmetic stays a factor of ten inside the bar;
  * bf16 gradients: the same bar plus one bf16 step of the element, |hip - ref64| <= 2e-5 max|ref64| + 2^-7 |ref64| elementwise,
    since the fp32 sum is rounded once to the table's dtype;
  * rows of ids that do not occur: exactly zero; no NaN left of a NaN pre-fill; two runs, and a run with a caller's token order,
    give the same bits.
"""
import functools

import numpy as np
import pytest
import torch
from torch import nn

import value_embeds_ref as vr
from util_gpu import DEV, dev, host, rel

pytestmark = pytest.mark.gpu
TOL = 2e-5
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}

# name: (vocab, dim, token shape, tables, kind of ids, seed, dtypes)
SHAPES = {
    "v50_d4_n1": (50, 4, (1,), 1, "uniform", 7001, ("fp32",)),                  # 4 columns are 16 bytes in fp32 only
    "v97_d8_n63": (97, 8, (63,), 3, "uniform", 7002, ("fp32", "bf16")),         # one short of a slice of the sorted stream,
    "v97_d8_n64": (97, 8, (64,), 3, "uniform", 7003, ("fp32", "bf16")),         # a slice,
    "v97_d8_n65": (97, 8, (65,), 3, "uniform", 7004, ("fp32", "bf16")),         # one more
    "v1000_d768_n257": (1000, 768, (257,), 3, "uniform", 7005, ("fp32",)),      # three column blocks of 64 lanes x 4
    "v300_d1024_n4096": (300, 1024, (4096,), 3, "skewed", 7006, ("bf16",)),     # the training scripts' width, skewed ids
    "v64_d2048_n513": (64, 2048, (513,), 4, "uniform", 7007, ("fp32", "bf16")),  # the widest row, four tables
    "v10_d64_n6000_hot": (10, 64, (6000,), 2, "hot", 7008, ("fp32", "bf16")),   # one hot group: every id 3 except ten
    "v10_d8_n40000_hot": (10, 8, (40000,), 1, "hot", 7012, ("fp32", "bf16")),    # a group of more than 32 768 positions: past the LDS sort
    "v4096_d16_perm": (4096, 16, (4096,), 1, "perm", 7009, ("fp32", "bf16")),   # every group of size one
    "v50257_d16_n300": (50257, 16, (300,), 2, "uniform", 7010, ("fp32", "bf16")),  # almost every row absent
    "v100_d32_3x50_ends": (100, 32, (3, 50), 2, "ends", 7011, ("fp32", "bf16")),   # (B, T) tokens, ids only 0 and vocab - 1
}
CASES = [(n, dt) for n, c in SHAPES.items() for dt in c[6]]


@pytest.fixture(scope="module")
def mot():
    import mixture_of_tokenizers_amd as m
    return m


@functools.lru_cache(maxsize=None)
def case(name):
    """(tokens, tables, gradients, float64 table gradients) of a shape: computed once, shared by the tests, never written to"""
    vocab, dim, shape, n, kind, seed, _ = SHAPES[name]
    toks = vr.make_tokens(seed, vocab, shape, kind)
    tables, gs = vr.make_inputs(seed, vocab, dim, shape, n)
    ref = vr.run(toks, tables, gs, dtype=torch.float64, device=DEV)["d_table"]
    return toks, tables, gs, ref


def check_grad(got, ref, dt, what=""):
    """got: a device tensor in the table's dtype; ref: the float64 gradient"""
    assert got.dtype == DTYPES[dt] and tuple(got.shape) == ref.shape
    g = host(got.float()).astype(np.float64)
    assert np.isfinite(g).all(), f"{what}: {int((~np.isfinite(g)).sum())} non-finite elements"
    print(f"{what}: max|hip - float64| / max|float64| = {float(rel(g, ref)):.3e}")
    if dt == "fp32":
        assert rel(g, ref) < TOL
    else:
        excess = np.abs(g - ref) - (TOL * np.abs(ref).max() + 2.0 ** -7 * np.abs(ref))
        assert (excess <= 0).all(), f"{what}: {int((excess > 0).sum())} elements over the bar, worst excess {excess.max():.3e}"


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("name,dt", CASES)
def test_forward_is_a_copy(mot, name, dt):
    toks, tables, gs, _ = case(name)
    tabs = [dev(t, DTYPES[dt]) for t in tables]
    for tok in (dev(toks), dev(toks.astype(np.int64))):
        outs = mot.value_embeds(tok, tabs)
        assert isinstance(outs, tuple) and len(outs) == len(tabs)
        for o, t in zip(outs, tabs):
            assert o.dtype == DTYPES[dt] and tuple(o.shape) == toks.shape + (t.shape[1],)
            assert torch.equal(o, t[tok.long()])
    mot.check_status()


# ------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("name,dt", CASES)
def test_backward_writes_every_element_once_with_the_same_bits(mot, name, dt):
    Fm = mot.functional
    vocab, dim, shape, n, kind, seed, _ = SHAPES[name]
    toks, tables, gs, ref = case(name)
    tok = dev(toks)
    tabs = [dev(t, DTYPES[dt]) for t in tables]
    ups = [dev(g, DTYPES[dt]) for g in gs]
    bufs = [torch.full((vocab, dim), float("nan"), dtype=DTYPES[dt], device=DEV) for _ in range(n)]
    got = Fm.value_embeds_backward(ups, tok, tabs, out=bufs)
    mot.check_status()
    absent = np.setdiff1d(np.arange(vocab), toks)
    for j in range(n):
        assert got[j] is bufs[j]
        assert not torch.isnan(got[j]).any(), f"d_table{j}: {int(torch.isnan(got[j]).sum())} elements were never written"
        check_grad(got[j], ref[j], dt, f"{name} {dt} d_table{j}")
        rows = got[j][dev(absent)].float()
        assert not rows.any() and not torch.signbit(rows).any()                    # +0, not a small number and not -0
    again = Fm.value_embeds_backward(ups, tok, tabs)                               # fresh (uninitialised) buffers, a second run
    order = Fm.token_order(tok, vocab)
    given = Fm.value_embeds_backward(ups, tok, tabs, token_order=order)
    for j in range(n):
        assert torch.equal(again[j], got[j]), f"d_table{j}: two runs differ"
        assert torch.equal(given[j], got[j]), f"d_table{j}: the caller's token order changes the bits"


def test_a_none_gradient_skips_its_table(mot):
    Fm = mot.functional
    name = "v97_d8_n65"
    toks, tables, gs, ref = case(name)
    tok = dev(toks.astype(np.int64))
    for dt in DTYPES:
        tabs = [dev(t, DTYPES[dt]) for t in tables]
        ups = [dev(gs[0], DTYPES[dt]), None, dev(gs[2], DTYPES[dt])]
        bufs = [torch.full((97, 8), 7.0, dtype=DTYPES[dt], device=DEV) for _ in range(3)]
        got = Fm.value_embeds_backward(ups, tok, tabs, out=bufs)
        assert got[1] is None and (bufs[1] == 7.0).all()                            # untouched
        check_grad(got[0], ref[0], dt, f"{dt} d_table0")
        check_grad(got[2], ref[2], dt, f"{dt} d_table2")
        assert Fm.value_embeds_backward([None] * 3, tok, tabs) == [None] * 3


# ------------------------------------------------------------------------------------------------ autograd
@pytest.mark.parametrize("dt", list(DTYPES))
def test_autograd_through_the_module(mot, dt):
    """ve[0] feeds two consumers, as train_gpt.py:602 does; .grad is in the parameter's dtype; a second backward accumulates."""
    vocab, dim, B, T, seed = 211, 64, 2, 96, 7100
    toks = vr.make_tokens(seed, vocab, (B, T), "skewed")
    tables, gs = vr.make_inputs(seed, vocab, dim, (B, T), 3)
    extra = vr.bf16_values(np.random.RandomState(seed + 30).standard_normal((B, T, dim)))
    m = mot.modules.ValueEmbeds(vocab, dim).to(DEV)
    for sub in m.modules():
        if isinstance(sub, nn.Embedding) and dt == "bf16":
            sub.bfloat16()                                                           # the training scripts' cast
    with torch.no_grad():
        for e, t in zip(m, tables):
            e.weight.copy_(dev(t, DTYPES[dt]))
    tok = dev(toks)
    ups = [dev(g, DTYPES[dt]) for g in gs]
    up_extra = dev(extra, DTYPES[dt])

    def step():
        ve = m(tok)
        assert isinstance(ve, list) and len(ve) == 3
        torch.autograd.backward([ve[0], ve[1], ve[2], ve[0]], ups + [up_extra])
        return ve

    ve = step()
    mot.check_status()
    for o, e in zip(ve, m):
        assert torch.equal(o, e.weight.detach()[tok.long()])
    # autograd adds the two gradients of ve[0] in the outputs' dtype before the node sees them
    g0 = host((ups[0] + up_extra).double())
    ref = vr.run(toks, tables, [g0, gs[1], gs[2]], dtype=torch.float64, device=DEV)["d_table"]
    first = []
    for j, e in enumerate(m):
        assert e.weight.grad.dtype == DTYPES[dt] and e.weight.grad.shape == e.weight.shape
        check_grad(e.weight.grad, ref[j], dt, f"{dt} .grad {j}")
        first.append(e.weight.grad.clone())
    step()
    for j, e in enumerate(m):
        assert torch.equal(e.weight.grad, first[j] + first[j])                       # accumulated: twice the same bits


def test_live_weights_are_read(mot):
    """Tied or in-place-updated tables are honoured: nothing is cached between calls."""
    m = mot.modules.ValueEmbeds(50, 8, n=2).to(DEV)
    tok = dev(np.arange(50, dtype=np.int32))
    m[1].weight = m[0].weight                                                         # tied
    with torch.no_grad():
        m[0].weight.mul_(3.0)
    a, b = m(tok)
    assert torch.equal(a, m[0].weight.detach()) and torch.equal(b, a)
    (a + 2 * b).sum().backward()
    assert torch.equal(m[0].weight.grad, torch.full((50, 8), 3.0, device=DEV))


def test_one_sort_serves_the_front_end_and_the_value_embeddings(mot):
    Fm = mot.functional
    vocab, dim, seed = 97, 8, 7200
    tok = dev(vr.make_tokens(seed, vocab, (2, 40), "uniform"))
    tables, _ = vr.make_inputs(seed, vocab, dim, (2, 40), 3)
    params = [dev(t, torch.float32).requires_grad_(True) for t in tables]
    Fm._token_orders.clear()
    x = mot.embed_mix(tok, params[0], mode="noop", norm_tok=False)
    entries = list(Fm._token_orders.entries)
    assert len(entries) == 1
    ve = mot.value_embeds(tok, params)
    assert len(Fm._token_orders.entries) == 1 and Fm._token_orders.entries[0][3] is entries[0][3]
    (x.sum() + sum(v.sum() for v in ve)).backward()
    torch.cuda.synchronize()
    counts = np.bincount(host(tok).reshape(-1), minlength=vocab).astype(np.float32)
    assert np.array_equal(host(params[1].grad), np.repeat(counts[:, None], dim, axis=1))
    assert np.array_equal(host(params[0].grad), 2 * np.repeat(counts[:, None], dim, axis=1))


# ------------------------------------------------------------------------------------------------ bad ids
@pytest.mark.parametrize("bad", [97 + 7, -1])
def test_an_id_out_of_range_is_flagged_and_read_as_row_zero(mot, bad):
    Fm = mot.functional
    vocab, dim, seed = 97, 8, 7300
    toks = vr.make_tokens(seed, vocab, (130,), "uniform")
    toks[[5, 77]] = bad
    tables, gs = vr.make_inputs(seed, vocab, dim, (130,), 2)
    tabs = [dev(t, torch.float32) for t in tables]
    mot.check_status()
    outs = mot.value_embeds(dev(toks), tabs)
    with pytest.raises(IndexError):
        mot.check_status()
    clamped = np.where((toks >= 0) & (toks < vocab), toks, 0)
    for o, t in zip(outs, tabs):
        assert torch.isfinite(o).all() and torch.equal(o, t[dev(clamped).long()])
    got = Fm.value_embeds_backward([dev(g, torch.float32) for g in gs], dev(toks), tabs)
    with pytest.raises(IndexError):
        mot.check_status()
    ref = vr.run(clamped, tables, gs, dtype=torch.float64, device=DEV)["d_table"]
    for j in range(2):
        check_grad(got[j], ref[j], "fp32", f"bad id {bad} d_table{j}")
    mot.check_status()


# ------------------------------------------------------------------------------------------------ hipGraph
def _graph_step(step, params):
    """warm up eagerly on the capture stream, then capture one step; returns (graph, what the captured step returned)"""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                                      # allocates the workspace, fills the token-order cache
        for p in params:
            p.grad = None
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        outs = step()
    return graph, outs


@pytest.mark.parametrize("dt", list(DTYPES))
def test_forward_and_backward_replay_from_a_hip_graph(mot, dt):
    """No memset node, no allocation by the library, no sync, and no token order from outside the capture: capture forward +
    backward through the autograd node, copy a new batch into the token buffer, replay, compare with an eager run on it."""
    vocab, dim, B, T, seed = 300, 64, 2, 160, 7400
    tables, gs = vr.make_inputs(seed, vocab, dim, (B, T), 3)
    toks = dev(vr.make_tokens(seed + 1, vocab, (B, T), "skewed"))
    params = [dev(t, DTYPES[dt]).requires_grad_(True) for t in tables]
    ups = [dev(g, DTYPES[dt]) for g in gs]

    def step():
        outs = mot.value_embeds(toks, params)
        torch.autograd.backward(list(outs), ups)
        return outs

    graph, outs = _graph_step(step, params)
    toks.copy_(dev(vr.make_tokens(seed + 2, vocab, (B, T), "skewed")))       # a new batch, the same buffer
    graph.replay()
    torch.cuda.synchronize()
    fresh = [p.detach().clone().requires_grad_(True) for p in params]
    want = mot.value_embeds(toks, fresh)
    torch.autograd.backward(list(want), ups)
    mot.check_status()
    for a, b in zip(outs, want):
        assert torch.equal(a, b)
    for p, q in zip(params, fresh):
        assert q.grad.abs().max() > 0
        assert torch.equal(p.grad, q.grad)                                     # the same bits, replayed or eager


def test_the_fused_front_end_sorts_inside_the_capture(mot):
    """The same sequence through embed_mix(mode="noop"): the token order of the eager warm-up must not be replayed for the new batch."""
    vocab, dim, B, T, seed = 300, 64, 2, 160, 7500
    tables, gs = vr.make_inputs(seed, vocab, dim, (B, T), 1)
    toks = dev(vr.make_tokens(seed + 1, vocab, (B, T), "skewed"))
    param = dev(tables[0], torch.float32).requires_grad_(True)
    up = dev(gs[0], torch.float32)

    def step():
        x = mot.embed_mix(toks, param, mode="noop", norm_tok=False)
        x.backward(up)
        return x

    graph, x = _graph_step(step, [param])
    new = vr.make_tokens(seed + 2, vocab, (B, T), "skewed")
    toks.copy_(dev(new))
    graph.replay()
    torch.cuda.synchronize()
    mot.check_status()
    assert torch.equal(x, param.detach()[toks.long()])
    ref = vr.run(new, tables, gs, dtype=torch.float64, device=DEV)["d_table"][0]
    assert rel(host(param.grad), ref) < TOL


# ------------------------------------------------------------------------------------------------ refusals
def test_functional_refusals(mot):
    Fm = mot.functional
    z = lambda r, c, dt=torch.float32: torch.zeros(r, c, device=DEV, dtype=dt)
    tok = torch.zeros((2, 8), dtype=torch.int64, device=DEV)
    with pytest.raises(NotImplementedError, match="dim 6"):
        mot.value_embeds(tok, [z(50, 6)])
    with pytest.raises(NotImplementedError, match="multiple of 8"):
        mot.value_embeds(tok, [z(50, 12, torch.bfloat16)])
    with pytest.raises(NotImplementedError, match="dim 2052"):
        mot.value_embeds(tok, [z(50, 2052)])
    with pytest.raises(ValueError, match="5 tables"):
        mot.value_embeds(tok, [z(50, 8)] * 5)
    with pytest.raises(TypeError, match="share one dtype"):
        mot.value_embeds(tok, [z(50, 8), z(50, 8, torch.bfloat16)])
    with pytest.raises(ValueError, match="table 1 must be"):
        mot.value_embeds(tok, [z(50, 8), z(51, 8)])
    with pytest.raises(TypeError, match="int32 or int64"):
        mot.value_embeds(tok.float(), [z(50, 8)])
    with pytest.raises(ValueError, match="2 gradients for 1 tables"):
        Fm.value_embeds_backward([z(16, 8), z(16, 8)], tok, [z(50, 8)])
    with pytest.raises(ValueError, match="token_order must be"):
        Fm.value_embeds_backward([torch.zeros(2, 8, 8, device=DEV)], tok, [z(50, 8)], token_order=torch.zeros(3, dtype=torch.int32, device=DEV))
    (x,) = mot.value_embeds(tok[:, :0], [z(50, 8)])                                # an empty batch
    assert x.shape == (2, 0, 8)
    (g,) = Fm.value_embeds_backward([x], tok[:, :0], [z(50, 8)])
    assert g.shape == (50, 8) and not g.any()
