"""-m gpu: the mixture-of-tokenizers value embeddings ve_j = norm(W_j . cat(Vt_j[tok], Vb_j[id_0], ..., Vb_j[id_{bpt-1}])) (mot.value_mix,
MotValueMixDesc; modded-nanogpt/runs/9_mot-in_mot-valemb.py:310-313), forward and backward, float32 and bfloat16, against the
reference's own runs (tests/golden/value_mix.npz) and the float64 restatement of tests/value_mix_ref.py evaluated with the kernels'
epsilon on the same (bfloat16-valued) operands.

Shapes: the smallest at which a route can go wrong (token_dim / byte_dim / bpt -> out_dim, B x T, slots):
  V1  32 /  8 /  8 ->   32, 2 x 24, 3   fixture case; the composed route in both dtypes; EOT at a row start, mid-row and doubled
  V2  64 / 24 /  4 ->   64, 2 x 24, 2   fixture case; K = 160
  V3 256 / 16 / 16 ->  256, 3 x 200, 3  600 rows: a tail tile; bf16 takes the one-launch gather-GEMM
  V4 1024 / 64 / 16 -> 1024, 1 x 520, 3 the runs' dims: four whole 128-token tiles plus 8 (bf16: two column passes)
  V5 128 / 16 /  8 ->  512, 2 x 130     once with 1 slot and once with 4; out_dim != token_dim
  V6 = V3's dims, 1 x 256, every token and every byte id equal: one row of each table receives everything

Bars (the project's own, as tests/test_gpu_byte_fc.py):
  * fp32 forward: max|hip - f64| <= 2 max(max|ref_fp32 - f64|, 1e-6), ref_fp32 the reference's own float32 run (fixture cases) or the
    restatement in float32;
  * bf16 forward: max|hip - f64| <= 2 max|ref_bf16 - f64|, ref_bf16 the reference's own bfloat16 run or the restatement in bfloat16;
  * fp32 gradients: max|hip - ref64| <= 2e-5 max|ref64| per tensor;
  * bf16 gradients (every one passes through a bf16 MFMA product): elementwise err <= 2^-8 |ref| + 4e-3 max|ref|;
  * two GPU results whose atomic order may differ, or two routes: twice the gradient bar between them.
"""
import functools

import numpy as np
import pytest
import torch

import golden_inputs as gi
import value_mix_ref as vm
from oracle import oracle as orc
from util_gpu import DEV, dev, host, rel

pytestmark = pytest.mark.gpu
TOL = 2e-5
SHAPES = {   # name: (token_dim, byte_dim, bpt, out_dim, B, T, slots, token vocab, seed, fixture case)
    "V1": (32, 8, 8, 32, 2, 24, 3, 40, 9001, "t32_b8_bpt8"),
    "V2": (64, 24, 4, 64, 2, 24, 2, 40, 9002, "t64_b24_bpt4"),
    "V3": (256, 16, 16, 256, 3, 200, 3, 300, 9103, None),
    "V4": (1024, 64, 16, 1024, 1, 520, 3, 300, 9104, None),
    "V5a": (128, 16, 8, 512, 2, 130, 1, 150, 9105, None),
    "V5b": (128, 16, 8, 512, 2, 130, 4, 150, 9105, None),
}
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
KEYS = {"tok_table": "d_tok", "byte_table": "d_byte", "weight": "d_weight"}


@pytest.fixture(scope="module")
def mot():
    import mixture_of_tokenizers_amd as m
    return m


@functools.lru_cache(maxsize=None)
def golden():
    return vm.load_golden()


def eot_tokens(seed, B, T, Vt):
    """Token ids with the EOT token (vocab - 1) at a row start, in the middle of a row and twice in a row (as value_mix_ref.case_tokens)."""
    rs = np.random.RandomState(seed)
    toks = rs.randint(0, Vt - 1, size=(B, T)).astype(np.int32)
    toks[rs.random_sample((B, T)) < 0.1] = 0
    e = Vt - 1
    toks[0, 0] = toks[0, T // 2] = toks[B - 1, 3] = toks[B - 1, 4] = e
    return toks


def ids_of(toks, tab, bpt, pull):
    padded = orc.tokens_to_bytes(toks, tab.astype(np.float32))
    if pull == "left":
        return padded, orc.pull_from_left(padded, bpt, gi.PAD, gi.EOT)
    if pull == "right":
        return padded, orc.pull_from_right(padded, bpt, gi.PAD, gi.EOT)
    return padded, padded


@functools.lru_cache(maxsize=None)
def problem(name):
    """Inputs of a shape as numpy arrays (float64 arrays of bfloat16 values): computed once and shared; no test writes to them."""
    Dt, Db, bpt, Do, B, T, S, Vt, seed, case = SHAPES[name]
    if case:
        toks, tab, slots = vm.case_tokens(case), vm.case_ttb(case), vm.case_tables(case)
        ids = golden()[vm.key(case, "ids_pulled")].astype(np.int64)
    else:
        toks, tab = eot_tokens(seed, B, T, Vt), gi.synth_ttb(seed + 1, Vt, bpt, "left")
        slots = vm.make_inputs(seed, Vt, Dt, Db, bpt, Do, B, T, S)
        ids = ids_of(toks, tab, bpt, "left")[1].astype(np.int64)
    return toks, tab, ids, slots


def restate(toks, ids, slots, bpt, norm_out=True):
    """float64 restatement with the kernels' epsilon plus the restatement's float32 / bfloat16 forward, per slot"""
    r = vm.run(toks, ids, slots, bpt=bpt, norm_out=norm_out, eps=vm.F32_EPS)
    t = lambda a, dt: torch.tensor(a, dtype=torch.float64).to(dt)
    with torch.no_grad():
        for j, (Vt_, Vb_, W_, g_) in enumerate(slots):
            for k, dt in DTYPES.items():
                r[j]["out_" + k] = vm.forward(toks, ids, t(Vt_, dt), t(Vb_, dt), t(W_, dt), bpt=bpt, norm_out=norm_out, eps=vm.F32_EPS).double().numpy()
    return r


@functools.lru_cache(maxsize=None)
def reference(name, norm_out=True):
    """Per slot: the float64 restatement with the kernels' epsilon, and the float32 / bfloat16 forward it is compared with (the
    reference's own runs for the fixture cases with the norm, else the restatement in that dtype)."""
    Dt, Db, bpt, Do, B, T, S, Vt, seed, case = SHAPES[name]
    toks, tab, ids, slots = problem(name)
    r = restate(toks, ids, slots, bpt, norm_out)
    if case and norm_out:
        for j in range(S):
            r[j]["out_fp32"] = golden()[vm.key(case, f"{j}/f32/out")].astype(np.float64)
            r[j]["out_bf16"] = golden()[vm.key(case, f"{j}/bf16/out")].astype(np.float64)
    return r


def params(name, dtype, leaf=True):
    toks, tab, ids, slots = problem(name)
    P = (lambda a: torch.nn.Parameter(dev(a, dtype))) if leaf else (lambda a: dev(a, dtype))
    return (dev(toks), dev(ids), [P(s[0]) for s in slots], [P(s[1]) for s in slots], [P(s[2]) for s in slots], [dev(s[3], dtype) for s in slots])


def forward_bar(ref, dt):
    f64 = ref["out"]
    if dt == "fp32":
        return 2 * max(float(np.abs(ref["out_fp32"] - f64).max()), 1e-6)
    return 2 * float(np.abs(ref["out_bf16"] - f64).max())


def check_forward(x, ref, dt, what):
    err, bar = float(np.abs(host(x.float()).astype(np.float64) - ref["out"]).max()), forward_bar(ref, dt)
    print(f"{what} forward {dt}: max|hip - f64| {err:.3e}, bar {bar:.3e}, error over bar {err / bar:.3f}")
    assert np.isfinite(host(x.float())).all() and err <= bar, (what, dt, err, bar)


def grad_bar(r, dt):
    """elementwise bar of a gradient tensor against its float64 reference r"""
    return 2.0 ** -8 * np.abs(r) + 4e-3 * np.abs(r).max() if dt == "bf16" else np.full(r.shape, TOL * np.abs(r).max())


def check_grads(got, ref, dt, what):
    """got: {tok_table, byte_table, weight} of one slot"""
    for k, rk in KEYS.items():
        r, a = ref[rk], host(got[k].float()).astype(np.float64).reshape(ref[rk].shape)
        err, bar = np.abs(a - r), grad_bar(r, dt)
        print(f"{what} {rk} {dt}: worst error over bar {float((err / bar).max()):.3f} (max error {float(err.max() / np.abs(r).max()):.3e} of max|ref|)")
        assert np.isfinite(a).all() and (err <= bar).all(), (what, rk, float((err / bar).max()))


def close_grads(a, b, dt, what, factor=2):
    """two device results of one slot within `factor` times the gradient bar of each other"""
    for k in KEYS:
        x, y = host(a[k].float()).astype(np.float64), host(b[k].float()).astype(np.float64)
        err, bar = np.abs(x - y), factor * grad_bar(y, dt)
        print(f"{what} {k} {dt}: worst difference over {factor} x bar {float((err / bar).max()):.3f}")
        assert (err <= bar).all(), (what, k)


def fwd_saved(mot, toks, Vt, Vb, W, **kw):
    """the forward with what the backward wants: (outs, ids, row_rnorms)"""
    return mot.functional._value_mix_fwd(toks, Vt, Vb, W, save=True, **kw)


# ------------------------------------------------------------------------------------------------ forward and gradients
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_and_gradients_ids_given(mot, name, dt):
    Dt, Db, bpt, Do, B, T, S, Vt, seed, case = SHAPES[name]
    toks, ids, pVt, pVb, pW, gs = params(name, DTYPES[dt])
    ref = reference(name)
    ve = mot.value_mix(toks, pVt, pVb, pW, bpt=bpt, ids=ids)
    assert isinstance(ve, tuple) and len(ve) == S
    for j, x in enumerate(ve):
        assert x.shape == (B, T, Do) and x.dtype == DTYPES[dt] and x.requires_grad
        check_forward(x, ref[j], dt, f"{name} slot {j}")
    assert len({x.grad_fn for x in ve}) == 1                       # ONE autograd node
    torch.autograd.backward(list(ve), gs)
    mot.check_status()
    for j in range(S):
        for p in (pVt[j], pVb[j], pW[j]):
            assert p.grad.dtype == DTYPES[dt] and p.grad.shape == p.shape
        check_grads({"tok_table": pVt[j].grad, "byte_table": pVb[j].grad, "weight": pW[j].grad}, ref[j], dt, f"{name} slot {j} .grad")
    # the direct call: the token-table gradients come back in the tables' dtype, the others as fp32 sums
    outs, _, rns = fwd_saved(mot, toks, [p.detach() for p in pVt], [p.detach() for p in pVb], [p.detach() for p in pW], bpt=bpt, ids=ids)
    res = mot.functional.value_mix_backward(gs, toks, [p.detach() for p in pVt], [p.detach() for p in pVb], [p.detach() for p in pW], bpt=bpt, ids=ids,
                                            outs=outs, row_rnorms=rns)
    for j in range(S):
        assert res[j]["tok_table"].dtype == DTYPES[dt] and res[j]["byte_table"].dtype == res[j]["weight"].dtype == torch.float32
        assert torch.equal(outs[j], ve[j].detach())
        check_grads(res[j], ref[j], dt, f"{name} slot {j} direct")
        assert torch.equal(res[j]["tok_table"], pVt[j].grad)       # written once, the same bits on every run


@pytest.mark.parametrize("dt", list(DTYPES))
def test_a_slot_without_a_gradient_is_skipped(mot, dt):
    Dt, Db, bpt, Do, B, T, S, Vt, seed, case = SHAPES["V1"]
    toks, ids, pVt, pVb, pW, gs = params("V1", DTYPES[dt])
    ve = mot.value_mix(toks, pVt, pVb, pW, bpt=bpt, ids=ids)
    ve[1].backward(gs[1])
    mot.check_status()
    assert pVt[0].grad is None and pW[2].grad is None and pVb[0].grad is None
    check_grads({"tok_table": pVt[1].grad, "byte_table": pVb[1].grad, "weight": pW[1].grad}, reference("V1")[1], dt, "V1 slot 1 alone")


@pytest.mark.parametrize("dt", list(DTYPES))
def test_without_the_output_norm(mot, dt):
    Dt, Db, bpt, Do, B, T, S, Vt, seed, case = SHAPES["V1"]
    toks, ids, Vt_, Vb_, W_, gs = params("V1", DTYPES[dt], leaf=False)
    ref = reference("V1", norm_out=False)
    ve = mot.value_mix(toks, Vt_, Vb_, W_, bpt=bpt, ids=ids, norm_out=False)
    res = mot.functional.value_mix_backward(gs, toks, Vt_, Vb_, W_, bpt=bpt, ids=ids, norm_out=False)
    mot.check_status()
    for j in range(S):
        check_forward(ve[j], ref[j], dt, f"V1 slot {j} no norm")
        check_grads(res[j], ref[j], dt, f"V1 slot {j} no norm")


@pytest.mark.parametrize("dt", list(DTYPES))
def test_supplied_token_order_gives_the_same_token_table_bits(mot, dt):
    Dt, Db, bpt, Do, B, T, S, Vt, seed, case = SHAPES["V3"]
    toks, ids, Vt_, Vb_, W_, gs = params("V3", DTYPES[dt], leaf=False)
    outs, _, rns = fwd_saved(mot, toks, Vt_, Vb_, W_, bpt=bpt, ids=ids)
    order = mot.functional.token_order(toks, Vt)
    kw = dict(bpt=bpt, ids=ids, outs=outs, row_rnorms=rns)
    a = mot.functional.value_mix_backward(gs, toks, Vt_, Vb_, W_, token_order=order, **kw)
    b = mot.functional.value_mix_backward(gs, toks, Vt_, Vb_, W_, **kw)
    mot.check_status()
    for j in range(S):
        assert torch.equal(a[j]["tok_table"], b[j]["tok_table"])
        check_grads(a[j], reference("V3")[j], dt, f"V3 slot {j} token order")
    with pytest.raises(ValueError, match="token_order"):
        mot.functional.value_mix_backward(gs, toks, Vt_, Vb_, W_, token_order=order[:-1].contiguous(), **kw)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_one_row_of_each_table_receives_everything(mot, dt):
    """V6: 256 equal tokens with equal byte ids."""
    Dt, Db, bpt, Do, B, T, S, Vt, seed = 256, 16, 16, 256, 1, 256, 3, 300, 9106
    slots = vm.make_inputs(seed, Vt, Dt, Db, bpt, Do, B, T, S)
    toks, ids = np.full((B, T), 17, dtype=np.int32), np.full((B, T * bpt), 101, dtype=np.int64)
    ref = vm.run(toks, ids, slots, bpt=bpt, eps=vm.F32_EPS)
    t = lambda a: dev(a, DTYPES[dt])
    Vt_, Vb_, W_, gs = [t(s[0]) for s in slots], [t(s[1]) for s in slots], [t(s[2]) for s in slots], [t(s[3]) for s in slots]
    outs, _, rns = fwd_saved(mot, dev(toks), Vt_, Vb_, W_, bpt=bpt, ids=dev(ids))
    res = mot.functional.value_mix_backward(gs, dev(toks), Vt_, Vb_, W_, bpt=bpt, ids=dev(ids), outs=outs, row_rnorms=rns)
    mot.check_status()
    for j in range(S):
        assert torch.equal(outs[j][0, 0], outs[j][0, T - 1])
        check_grads(res[j], ref[j], dt, f"V6 slot {j}")
        assert int((res[j]["tok_table"].float().abs().sum(1) > 0).sum()) == 1 and int((res[j]["byte_table"].abs().sum(1) > 0).sum()) == 1
        assert not torch.signbit(res[j]["tok_table"][[0, 16, 18, Vt - 1]].float()).any()      # rows of absent ids are +0


# ------------------------------------------------------------------------------------------------ ids from the token->byte table
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("pull", ["left", "right", None])
@pytest.mark.parametrize("name", ["V1", "V3"])
def test_ids_from_the_token_to_byte_table(mot, name, pull, dt):
    Dt, Db, bpt, Do, B, T, S, Vt, seed, case = SHAPES[name]
    toks, tab, _, slots = problem(name)
    padded, ids = ids_of(toks, tab, bpt, pull)
    _, _, Vt_, Vb_, W_, gs = params(name, DTYPES[dt], leaf=False)
    o_t, ids_t, rn_t = fwd_saved(mot, dev(toks), Vt_, Vb_, W_, bpt=bpt, ttb=dev(tab), pull=pull)
    o_g, ids_g, rn_g = fwd_saved(mot, dev(toks), Vt_, Vb_, W_, bpt=bpt, ids=dev(ids.astype(np.int64)))
    mot.check_status()
    np.testing.assert_array_equal(host(ids_t), ids)                 # made once, for all slots
    for j in range(S):
        assert torch.equal(o_t[j], o_g[j]) and torch.equal(rn_t[j], rn_g[j])
    ve = mot.value_mix(dev(toks), Vt_, Vb_, W_, bpt=bpt, ttb=dev(tab), pull=pull)      # the public call
    assert all(torch.equal(a, b) for a, b in zip(ve, o_g))
    if pull == "left":
        ref = reference(name)
        for j in range(S):
            check_forward(ve[j], ref[j], dt, f"{name} slot {j} ttb")
    # and through autograd: the node saves the ids the forward made
    pW = [torch.nn.Parameter(w.clone()) for w in W_]
    ve = mot.value_mix(dev(toks), Vt_, Vb_, pW, bpt=bpt, ttb=dev(tab), pull=pull)
    torch.autograd.backward(list(ve), gs)
    mot.check_status()
    res = mot.functional.value_mix_backward(gs, dev(toks), Vt_, Vb_, W_, bpt=bpt, ids=ids_t, outs=o_t, row_rnorms=rn_t)
    for j in range(S):
        close_grads({"weight": pW[j].grad, "tok_table": res[j]["tok_table"], "byte_table": res[j]["byte_table"]}, res[j], dt, f"{name} slot {j} ttb")


# ------------------------------------------------------------------------------------------------ against what exists
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", ["V3", "V5b"])
def test_agrees_with_separate_concat_linear_calls(mot, name, dt):
    """One embed_mix(mode="concat_linear", norm_out=True) call per slot computes the same thing, with its own autograd node."""
    Dt, Db, bpt, Do, B, T, S, Vt, seed, case = SHAPES[name]
    toks, ids, pVt, pVb, pW, gs = params(name, DTYPES[dt])
    qVt, qVb, qW = ([torch.nn.Parameter(p.detach().clone()) for p in ps] for ps in (pVt, pVb, pW))
    ve = mot.value_mix(toks, pVt, pVb, pW, bpt=bpt, ids=ids)
    torch.autograd.backward(list(ve), gs)
    ref = reference(name)
    for j in range(S):
        y = mot.embed_mix(toks, qVt[j], qVb[j], mode="concat_linear", bpt=bpt, ids_a=ids, weight=qW[j], norm_out=True, eps=vm.F32_EPS)
        y.backward(gs[j])
        mot.check_status()
        diff, bar = float((ve[j].detach().float() - y.detach().float()).abs().max()), forward_bar(ref[j], dt)
        print(f"{name} slot {j} {dt}: max|value_mix - concat_linear| {diff:.3e}, bar {bar:.3e}")
        assert diff <= bar
        close_grads({"tok_table": pVt[j].grad, "byte_table": pVb[j].grad, "weight": pW[j].grad},
                    {"tok_table": qVt[j].grad, "byte_table": qVb[j].grad, "weight": qW[j].grad}, dt, f"{name} slot {j} vs concat_linear")


# ------------------------------------------------------------------------------------------------ determinism, graphs, bad ids, empty
@pytest.mark.parametrize("dt", list(DTYPES))
def test_forward_bits_repeat_and_backward_repeats_within_the_bar(mot, dt):
    Dt, Db, bpt, Do, B, T, S, Vt, seed, case = SHAPES["V3"]
    toks, ids, Vt_, Vb_, W_, gs = params("V3", DTYPES[dt], leaf=False)
    o1, _, rn1 = fwd_saved(mot, toks, Vt_, Vb_, W_, bpt=bpt, ids=ids)
    o2, _, rn2 = fwd_saved(mot, toks, Vt_, Vb_, W_, bpt=bpt, ids=ids)
    a = mot.functional.value_mix_backward(gs, toks, Vt_, Vb_, W_, bpt=bpt, ids=ids, outs=o1, row_rnorms=rn1)
    b = mot.functional.value_mix_backward(gs, toks, Vt_, Vb_, W_, bpt=bpt, ids=ids, outs=o1, row_rnorms=rn1)
    for j in range(S):
        assert torch.equal(o1[j], o2[j]) and torch.equal(rn1[j], rn2[j])
        assert torch.equal(a[j]["tok_table"], b[j]["tok_table"])
        close_grads(a[j], b[j], dt, f"V3 slot {j} repeat")


@pytest.mark.parametrize("dt", list(DTYPES))
def test_forward_and_backward_replay_from_a_hip_graph(mot, dt):
    """No memset or memcpy node, no allocation by the library, no sync: capture forward + backward, change the batch in place,
    replay, compare with the uncaptured calls."""
    Dt, Db, bpt, Do, B, T, S, Vt, seed, case = SHAPES["V3"]
    toks, ids, Vt_, Vb_, W_, gs = params("V3", DTYPES[dt], leaf=False)
    toks, ids, gs = toks.clone(), ids.clone(), [g.clone() for g in gs]
    F = mot.functional
    held = {}

    def step():
        outs, _, rns = fwd_saved(mot, toks, Vt_, Vb_, W_, bpt=bpt, ids=ids)
        held["outs"], held["rns"] = outs, rns
        held["res"] = F.value_mix_backward(gs, toks, Vt_, Vb_, W_, bpt=bpt, ids=ids, outs=outs, row_rnorms=rns)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                      # warm-up on the capture stream: allocates the workspaces
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        step()
    rs = np.random.RandomState(9150)
    toks.copy_(dev(rs.randint(0, Vt, (B, T)).astype(np.int32)))
    ids.copy_(dev(rs.randint(0, gi.BYTE_VOCAB, (B, T * bpt)).astype(np.int64)))
    for g in gs:
        g.copy_(dev(vm.bf16_values(rs.standard_normal((B, T, Do))), DTYPES[dt]))
    graph.replay()
    torch.cuda.synchronize()
    outs, _, rns = fwd_saved(mot, toks, Vt_, Vb_, W_, bpt=bpt, ids=ids)
    ref = F.value_mix_backward(gs, toks, Vt_, Vb_, W_, bpt=bpt, ids=ids, outs=outs, row_rnorms=rns)
    mot.check_status()
    for j in range(S):
        assert torch.equal(outs[j], held["outs"][j]) and torch.equal(rns[j], held["rns"][j])
        assert torch.equal(ref[j]["tok_table"], held["res"][j]["tok_table"])
        close_grads(held["res"][j], ref[j], dt, f"V3 slot {j} graph")


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", ["V1", "V3"])
def test_out_of_range_byte_id_is_flagged_and_the_call_completes(mot, name, dt):
    Dt, Db, bpt, Do, B, T, S, Vt, seed, case = SHAPES[name]
    toks, ids, Vt_, Vb_, W_, gs = params(name, DTYPES[dt], leaf=False)
    mot.check_status()
    bad = ids.clone()
    bad[1, 5] = gi.BYTE_VOCAB + 3
    ve = mot.value_mix(toks, Vt_, Vb_, W_, bpt=bpt, ids=bad)
    torch.cuda.synchronize()
    assert all(torch.isfinite(x.float()).all() for x in ve)
    with pytest.raises(IndexError, match="byte id"):
        mot.check_status()
    mot.check_status()                                 # the word is cleared
    clamped = bad.clone()
    clamped[1, 5] = 0                                   # a bad id reads row 0
    want = mot.value_mix(toks, Vt_, Vb_, W_, bpt=bpt, ids=clamped)
    assert all(torch.equal(a, b) for a, b in zip(ve, want))
    mot.check_status()
    # the backward too: flagged, and the bad slot's gradient lands on row 0
    outs, _, rns = fwd_saved(mot, toks, Vt_, Vb_, W_, bpt=bpt, ids=clamped)
    a = mot.functional.value_mix_backward(gs, toks, Vt_, Vb_, W_, bpt=bpt, ids=bad, outs=outs, row_rnorms=rns)
    torch.cuda.synchronize()
    with pytest.raises(IndexError, match="byte id"):
        mot.check_status()
    assert all(torch.isfinite(r["byte_table"]).all() and torch.isfinite(r["weight"]).all() for r in a)


def test_empty_batch(mot):
    Vt_, Vb_, W_ = torch.zeros(10, 32, device=DEV), torch.zeros(gi.BYTE_VOCAB, 8, device=DEV), torch.zeros(32, 96, device=DEV)
    for shape, idshape in (((0, 4), (0, 32)), ((2, 0), (2, 0))):
        toks, ids = torch.zeros(shape, dtype=torch.int32, device=DEV), torch.zeros(idshape, dtype=torch.int64, device=DEV)
        ve = mot.value_mix(toks, [Vt_, Vt_], [Vb_, Vb_], [W_, W_], bpt=8, ids=ids)
        assert len(ve) == 2 and all(x.shape == shape + (32,) and x.dtype == torch.float32 for x in ve)
        res = mot.functional.value_mix_backward([torch.zeros(shape + (32,), device=DEV)] * 2, toks, [Vt_, Vt_], [Vb_, Vb_], [W_, W_], bpt=8, ids=ids,
                                                norm_out=False)
        assert all(not r[k].any() for r in res for k in KEYS)
    mot.check_status()


@pytest.mark.parametrize("dt", list(DTYPES))
def test_gradients_accumulate_into_an_existing_grad(mot, dt):
    Dt, Db, bpt, Do, B, T, S, Vt, seed, case = SHAPES["V1"]
    toks, ids, pVt, pVb, pW, gs = params("V1", DTYPES[dt])
    torch.autograd.backward(list(mot.value_mix(toks, pVt, pVb, pW, bpt=bpt, ids=ids)), gs)
    first = [[p.grad.clone() for p in ps] for ps in (pVt, pVb, pW)]
    torch.autograd.backward(list(mot.value_mix(toks, pVt, pVb, pW, bpt=bpt, ids=ids)), gs)
    mot.check_status()
    ref = reference("V1")
    for j in range(S):
        assert torch.equal(pVt[j].grad, first[0][j] + first[0][j])                     # the token-table gradient is the same bits every run
        twice = {k: 2 * ref[j][rk] for k, rk in KEYS.items()}
        got = {"tok_table": pVt[j].grad, "byte_table": pVb[j].grad, "weight": pW[j].grad}
        for k in KEYS:
            a, r = host(got[k].float()).astype(np.float64), twice[k]
            assert (np.abs(a - r) <= 2 * grad_bar(r, dt)).all(), (j, k)


# ------------------------------------------------------------------------------------------------ module
@pytest.mark.parametrize("dt", list(DTYPES))
def test_module_end_to_end_with_the_runs_byte_value_tables(mot, dt):
    """The runs allocate 50 257 rows for the byte value tables: the library sees the leading 458, rows from 458 on get zero gradient."""
    Dt, Db, bpt, Do, B, T, S, Vt, seed, case = SHAPES["V1"]
    toks, tab, ids, slots = problem("V1")
    V = 50257
    torch.manual_seed(0)
    m = mot.MotValueEmbeds(V, Dt, Db, bytes_per_token=bpt, n=S, ttb=torch.from_numpy(tab)).to(DEV)
    with torch.no_grad():
        for j, (Vt_, Vb_, W_, g_) in enumerate(slots):
            m.value_embeds_toks[j].weight[:Vt].copy_(dev(Vt_)); m.value_embeds_bytes[j].weight[:gi.BYTE_VOCAB].copy_(dev(Vb_))
            m.value_byte_mixin_weights[j].copy_(dev(W_))
    m = m.to(DTYPES[dt])
    assert sorted(m.state_dict()) == sorted([f"value_byte_mixin_weights.{j}" for j in range(S)] + [f"value_embeds_bytes.{j}.weight" for j in range(S)] +
                                            [f"value_embeds_toks.{j}.weight" for j in range(S)])
    ve_ids = m(dev(toks), dev(ids))
    ve_ttb = m(dev(toks))
    mot.check_status()
    ref = reference("V1")
    assert isinstance(ve_ids, list) and len(ve_ids) == S
    for j in range(S):
        assert torch.equal(ve_ids[j].detach(), ve_ttb[j].detach())
        check_forward(ve_ids[j].detach(), ref[j], dt, f"module slot {j}")
    ve1d = m(dev(toks[0]), dev(ids[0]))                     # a single sequence, as the run feeds it
    assert ve1d[0].shape == (T, Do) and torch.equal(ve1d[0].detach(), ve_ids[0].detach()[0])
    torch.autograd.backward(ve_ttb, [dev(s[3], DTYPES[dt]) for s in slots])
    torch.cuda.synchronize()
    mot.check_status()
    for j in range(S):
        gt, gb, gw = m.value_embeds_toks[j].weight.grad, m.value_embeds_bytes[j].weight.grad, m.value_byte_mixin_weights[j].grad
        assert gt.dtype == gb.dtype == gw.dtype == DTYPES[dt] and gt.shape == (V, Dt) and gb.shape == (V, Db)
        assert not gb[gi.BYTE_VOCAB:].any() and not gt[Vt:].any()
        check_grads({"tok_table": gt[:Vt], "byte_table": gb[:gi.BYTE_VOCAB], "weight": gw}, ref[j], dt, f"module slot {j}")
    opt = torch.optim.SGD(m.parameters(), lr=0.01)
    before = m.value_byte_mixin_weights[0].detach().clone()
    opt.step()
    assert not torch.equal(before, m.value_byte_mixin_weights[0].detach())
