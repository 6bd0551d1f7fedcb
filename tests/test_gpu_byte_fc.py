"""-m gpu: the linear-on-bytes mixin x = norm(E_tok[tok] + byte_fc . cat_k E_byte[id_k]) (mot.byte_fc_mix, MotByteFcMixDesc;
modded-nanogpt/runs/71051_*.py:225-229), forward and backward, float32 and bfloat16, against the reference's own runs
(tests/golden/byte_fc.npz) and the float64 restatement of tests/byte_fc_ref.py evaluated with the kernels' epsilon on the same
(bfloat16-valued) operands.

Shapes: the smallest at which a route can go wrong (model_dim, byte_dim, bpt, B x T):
  S1  64 /  8 /  8, 2 x 24    fixture case; the general scatter kernel
  S2  96 / 24 /  4, 2 x 24    fixture case; widths that are multiples of neither 64 nor 128
  S3 256 / 16 / 16, 3 x 200   600 rows: the 256-row product route with a tail tile; bf16: the residual gather-GEMM; the lane-contiguous scatter
  S4 768 / 48 / 16, 1 x 300   the headline dims (bf16: the gather-GEMM's NT = 6 form)
  S5 1024 / 64 / 16, 1 x 520  run 71051's dims: gradient rows of 2048 columns; bf16: the gather-GEMM's two column passes, four whole tiles + 8
  S6 512 / 16 /  8, 2 x 130   K = 128 != model_dim
  S7 = S3's dims, 1 x 256, every token and every byte id the same: one token row and one byte row receive everything

Bars (the project's own, DESIGN sections 4 and 10):
  * fp32 forward: max|hip - f64| <= 2 max(max|ref_fp32 - f64|, 1e-6), ref_fp32 the reference's own float32 run (fixture cases) or the
    restatement in float32;
  * gradients, fp32, and the bf16 token-table gradient (a sum of fp32 rows): max|hip - ref64| <= 2e-5 max|ref64| per tensor;
  * bf16 forward: max|hip - f64| <= 2 max|ref_bf16 - f64|, ref_bf16 the reference's own bfloat16 run or the restatement in bfloat16;
  * bf16 gradients whose products run on the bf16 MFMA (byte_fc, and through du the byte table): elementwise
    err <= 2^-8 |ref| + 4e-3 max|ref|, the bar of the bf16 concat + linear backward (tests/test_gpu_bf16.py);
  * two GPU results whose atomic order may differ: twice the gradient bar between them.
"""
import functools

import numpy as np
import pytest
import torch

import byte_fc_ref as bf
import golden_inputs as gi
from oracle import oracle as orc
from util_gpu import DEV, dev, host, rel

pytestmark = pytest.mark.gpu
TOL = 2e-5
SHAPES = {   # name: (model_dim, byte_dim, bpt, B, T, token vocab, seed, fixture case)
    "S1": (64, 8, 8, 2, 24, 40, 71051, "m64_b8_bpt8"),
    "S2": (96, 24, 4, 2, 24, 40, 71053, "m96_b24_bpt4"),
    "S3": (256, 16, 16, 3, 200, 300, 8103, None),
    "S4": (768, 48, 16, 1, 300, 200, 8104, None),
    "S5": (1024, 64, 16, 1, 520, 300, 8105, None),
    "S6": (512, 16, 8, 2, 130, 150, 8106, None),
}
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def mot():
    import mixture_of_tokenizers_amd as m
    return m


@functools.lru_cache(maxsize=None)
def golden():
    return bf.load_golden()


def eot_tokens(seed, B, T, Vt):
    """Token ids with the EOT token (vocab - 1) at a row start, in the middle of a row and twice in a row (as byte_fc_ref.case_tokens)."""
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
    Dm, Db, bpt, B, T, Vt, seed, case = SHAPES[name]
    if case:
        toks, tab = bf.case_tokens(case), bf.case_ttb(case)
        Et, Eb, W, g = bf.case_tables(case)
        ids = golden()[bf.key(case, "ids_pulled")].astype(np.int64)
    else:
        toks, tab = eot_tokens(seed, B, T, Vt), gi.synth_ttb(seed + 1, Vt, bpt, "left")
        Et, Eb, W, g = bf.make_inputs(seed, Vt, Dm, Db, bpt, B, T)
        ids = ids_of(toks, tab, bpt, "left")[1].astype(np.int64)
    return toks, tab, ids, Et, Eb, W, g


@functools.lru_cache(maxsize=None)
def reference(name, norm_out=True):
    """float64 restatement with the kernels' epsilon, and the float32 / bfloat16 forward it is compared with (the reference's own
    runs for the fixture cases with the norm, else the restatement in that dtype)."""
    Dm, Db, bpt, B, T, Vt, seed, case = SHAPES[name]
    toks, tab, ids, Et, Eb, W, g = problem(name)
    r = bf.run(toks, ids, Et, Eb, W, g, bpt=bpt, norm_out=norm_out, eps=bf.F32_EPS)
    if case and norm_out:
        r["out_fp32"], r["out_bf16"] = golden()[bf.key(case, "f32/out")].astype(np.float64), golden()[bf.key(case, "bf16/out")].astype(np.float64)
    else:
        t = lambda a, dt: torch.tensor(a, dtype=torch.float64).to(dt)
        with torch.no_grad():
            for k, dt in DTYPES.items():
                r["out_" + k] = bf.forward(toks, ids, t(Et, dt), t(Eb, dt), t(W, dt), bpt=bpt, norm_out=norm_out, eps=bf.F32_EPS).double().numpy()
    return r


def params(name, dtype):
    toks, tab, ids, Et, Eb, W, g = problem(name)
    P = lambda a: torch.nn.Parameter(dev(a, dtype))
    return dev(toks), dev(ids), P(Et), P(Eb), P(W), dev(g, dtype)


def forward_bar(ref, dt):
    """(what to compare, absolute bar) of the forward for a dtype"""
    f64 = ref["out"]
    if dt == "fp32":
        return 2 * max(float(np.abs(ref["out_fp32"] - f64).max()), 1e-6)
    return 2 * float(np.abs(ref["out_bf16"] - f64).max())


def check_forward(x, ref, dt, what):
    err, bar = float(np.abs(host(x.float()).astype(np.float64) - ref["out"]).max()), forward_bar(ref, dt)
    print(f"{what} forward {dt}: max|hip - f64| {err:.3e}, bar {bar:.3e}, error over bar {err / bar:.3f}")
    assert np.isfinite(host(x.float())).all() and err <= bar, (what, dt, err, bar)


def check_grads(got, ref, dt, what, mfma_keys=("byte_table", "byte_fc")):
    """got: fp32 sums {tok_table, byte_table, byte_fc} (or bf16 .grad tensors for the MFMA group)"""
    names = {"tok_table": "d_tok", "byte_table": "d_byte", "byte_fc": "d_byte_fc"}
    for k, rk in names.items():
        if k not in got:
            continue
        r, a = ref[rk], host(got[k].float()).astype(np.float64)
        if dt == "bf16" and k in mfma_keys:
            err, bar = np.abs(a - r), 2.0 ** -8 * np.abs(r) + 4e-3 * np.abs(r).max()
            print(f"{what} {rk} {dt}: worst error over bar {float((err / bar).max()):.3f} (max error {float(err.max() / np.abs(r).max()):.3e} of max|ref|)")
            assert (err <= bar).all(), (what, rk, float((err / bar).max()))
        else:
            e = rel(a, r)
            print(f"{what} {rk} {dt}: max|hip - ref64| / max|ref64| {float(e):.3e}, error over bar {float(e) / TOL:.3f}")
            assert e < TOL


# ------------------------------------------------------------------------------------------------ forward and gradients
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_and_gradients_ids_given(mot, name, dt):
    Dm, Db, bpt, B, T, Vt, seed, case = SHAPES[name]
    toks, ids, pEt, pEb, pW, g = params(name, DTYPES[dt])
    ref = reference(name)
    x = mot.byte_fc_mix(toks, pEt, pEb, pW, bpt=bpt, ids=ids)
    assert x.shape == (B, T, Dm) and x.dtype == DTYPES[dt] and x.requires_grad
    check_forward(x, ref, dt, name)
    x.backward(g)
    mot.check_status()
    for p in (pEt, pEb, pW):
        assert p.grad.dtype == DTYPES[dt] and p.grad.shape == p.shape
    if dt == "fp32":
        check_grads({"tok_table": pEt.grad, "byte_table": pEb.grad, "byte_fc": pW.grad}, ref, dt, name)
    else:
        # through autograd the .grad of a bf16 parameter is rounded once more: the bar of the bf16 concat + linear backward, every tensor
        check_grads({"tok_table": pEt.grad, "byte_table": pEb.grad, "byte_fc": pW.grad}, ref, dt, name + " .grad", mfma_keys=("tok_table", "byte_table", "byte_fc"))
        # and the fp32 sums the node rounds: the token-table gradient at the fp32 bar, the MFMA group at its own
        sums = mot.functional.byte_fc_mix_backward(g, toks, pEt.detach(), pEb.detach(), pW.detach(), bpt=bpt, ids=ids)
        assert all(v.dtype == torch.float32 for v in sums.values())
        check_grads(sums, ref, dt, name + " fp32 sums")
        # .grad is those sums rounded once (a second run's atomic order may move a sum across a rounding boundary: one bf16 step)
        assert ((pEt.grad.float() - sums["tok_table"]).abs() <= 2.0 ** -8 * sums["tok_table"].abs() + 1e-30).all()


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", ["S1", "S3"])
def test_without_the_output_norm(mot, name, dt):
    Dm, Db, bpt, B, T, Vt, seed, case = SHAPES[name]
    toks, ids, pEt, pEb, pW, g = params(name, DTYPES[dt])
    ref = reference(name, norm_out=False)
    x = mot.byte_fc_mix(toks, pEt, pEb, pW, bpt=bpt, ids=ids, norm_out=False)
    check_forward(x, ref, dt, name + " no norm")
    sums = mot.functional.byte_fc_mix_backward(g, toks, pEt.detach(), pEb.detach(), pW.detach(), bpt=bpt, ids=ids, norm_out=False)
    mot.check_status()
    check_grads(sums, ref, dt, name + " no norm")


@pytest.mark.parametrize("dt", list(DTYPES))
def test_supplied_token_order(mot, dt):
    Dm, Db, bpt, B, T, Vt, seed, case = SHAPES["S3"]
    toks, ids, pEt, pEb, pW, g = params("S3", DTYPES[dt])
    order = mot.functional.token_order(toks, Vt)
    kw = dict(bpt=bpt, ids=ids)
    if dt == "fp32":
        rn = torch.empty((B, T), dtype=torch.float32, device=DEV)
        kw.update(out=mot.functional._byte_fc_mix_fwd(toks, pEt.detach(), pEb.detach(), pW.detach(), bpt=bpt, ids=ids, row_rnorm=rn), row_rnorm=rn)
    sums = mot.functional.byte_fc_mix_backward(g, toks, pEt.detach(), pEb.detach(), pW.detach(), token_order=order, **kw)
    mot.check_status()
    check_grads(sums, reference("S3"), dt, "S3 token order")
    with pytest.raises(ValueError, match="token_order"):
        mot.functional.byte_fc_mix_backward(g, toks, pEt.detach(), pEb.detach(), pW.detach(), token_order=order[:-1].contiguous(), **kw)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_one_token_row_and_one_byte_row_receive_everything(mot, dt):
    """S7: 256 equal tokens with equal byte ids: every ds row lands on one token row, every du slot on one byte row."""
    Dm, Db, bpt, B, T, Vt, seed = 256, 16, 16, 1, 256, 300, 8107
    Et, Eb, W, g = bf.make_inputs(seed, Vt, Dm, Db, bpt, B, T)
    toks, ids = np.full((B, T), 17, dtype=np.int32), np.full((B, T * bpt), 101, dtype=np.int64)
    ref = bf.run(toks, ids, Et, Eb, W, g, bpt=bpt, eps=bf.F32_EPS)
    P = lambda a: torch.nn.Parameter(dev(a, DTYPES[dt]))
    pEt, pEb, pW = P(Et), P(Eb), P(W)
    x = mot.byte_fc_mix(dev(toks), pEt, pEb, pW, bpt=bpt, ids=dev(ids))
    assert torch.equal(x[0, 0], x[0, T - 1])
    kw = dict(bpt=bpt, ids=dev(ids))
    if dt == "fp32":
        rn = torch.empty((B, T), dtype=torch.float32, device=DEV)
        kw.update(out=mot.functional._byte_fc_mix_fwd(dev(toks), pEt.detach(), pEb.detach(), pW.detach(), bpt=bpt, ids=dev(ids), row_rnorm=rn), row_rnorm=rn)
    sums = mot.functional.byte_fc_mix_backward(dev(g, DTYPES[dt]), dev(toks), pEt.detach(), pEb.detach(), pW.detach(), **kw)
    mot.check_status()
    check_grads(sums, ref, dt, "S7")
    assert int((sums["tok_table"].abs().sum(1) > 0).sum()) == 1 and int((sums["byte_table"].abs().sum(1) > 0).sum()) == 1


# ------------------------------------------------------------------------------------------------ ids from the token->byte table
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("pull", ["left", "right", None])
@pytest.mark.parametrize("name", ["S1", "S3"])
def test_ids_from_the_token_to_byte_table(mot, name, pull, dt):
    Dm, Db, bpt, B, T, Vt, seed, case = SHAPES[name]
    toks, tab, _, Et, Eb, W, g = problem(name)
    padded, ids = ids_of(toks, tab, bpt, pull)
    F = mot.functional
    t = lambda a: dev(a, DTYPES[dt])
    tEt, tEb, tW = t(Et), t(Eb), t(W)
    rn_t, rn_g = (torch.empty((B, T), dtype=torch.float32, device=DEV) for _ in range(2))
    c_t, c_g = (torch.zeros(4, dtype=torch.int64, device=DEV) for _ in range(2))
    r = F._byte_fc_mix_fwd(dev(toks), tEt, tEb, tW, bpt=bpt, ttb=dev(tab), pull=pull, return_ids=True, counters=c_t, row_rnorm=rn_t)
    x = F._byte_fc_mix_fwd(dev(toks), tEt, tEb, tW, bpt=bpt, ids=dev(ids.astype(np.int64)), counters=c_g, row_rnorm=rn_g)
    mot.check_status()
    np.testing.assert_array_equal(host(r.ids_padded), padded)
    np.testing.assert_array_equal(host(r.ids_pulled), ids)
    assert torch.equal(r.x, x) and torch.equal(rn_t, rn_g)
    # counters: tokens and byte slots as the ids-given call counts them; pads before and after the pull from the oracle's ids
    assert host(c_g).tolist() == [B * T, B * T * bpt, 0, 0]
    assert host(c_t).tolist() == [B * T, B * T * bpt, int((padded == gi.PAD).sum()), int((ids == gi.PAD).sum())]
    # the public call, without the id outputs
    assert torch.equal(mot.byte_fc_mix(dev(toks), tEt, tEb, tW, bpt=bpt, ttb=dev(tab), pull=pull), x)


@pytest.mark.parametrize("name", ["S3", "S4", "S5", "S6"])
def test_bf16_composed_route(mot, name):
    """bf16 at model_dim 256 / 512 / 768 / 1024 runs as one gather-GEMM in its residual form (S5: two column passes); composed=True
    keeps the separate gather, product and row-pass kernels, the route of every other width.  Both meet the bar, with both id sources."""
    Dm, Db, bpt, B, T, Vt, seed, case = SHAPES[name]
    toks, tab, ids, Et, Eb, W, g = problem(name)
    t = lambda a: dev(a, torch.bfloat16)
    tEt, tEb, tW = t(Et), t(Eb), t(W)
    ref = reference(name)
    x_one = mot.byte_fc_mix(dev(toks), tEt, tEb, tW, bpt=bpt, ids=dev(ids))
    x_cmp = mot.byte_fc_mix(dev(toks), tEt, tEb, tW, bpt=bpt, ids=dev(ids), composed=True)
    check_forward(x_cmp, ref, "bf16", name + " composed")
    diff = float((x_one.float() - x_cmp.float()).abs().max())
    print(f"{name}: max|gather-GEMM - composed| {diff:.3e}")
    assert diff <= forward_bar(ref, "bf16")
    r = mot.byte_fc_mix(dev(toks), tEt, tEb, tW, bpt=bpt, ttb=dev(tab), pull="left", composed=True, return_ids=True)
    mot.check_status()
    np.testing.assert_array_equal(host(r.ids_pulled), ids)
    assert torch.equal(r.x, x_cmp)


# ------------------------------------------------------------------------------------------------ determinism, graphs, bad ids, empty
@pytest.mark.parametrize("dt", list(DTYPES))
def test_forward_bits_repeat_and_backward_repeats_within_the_bar(mot, dt):
    Dm, Db, bpt, B, T, Vt, seed, case = SHAPES["S3"]
    toks, ids, pEt, pEb, pW, g = params("S3", DTYPES[dt])
    F = mot.functional
    Et, Eb, W = pEt.detach(), pEb.detach(), pW.detach()
    rn1, rn2 = (torch.empty((B, T), dtype=torch.float32, device=DEV) for _ in range(2))
    x1 = F._byte_fc_mix_fwd(toks, Et, Eb, W, bpt=bpt, ids=ids, row_rnorm=rn1)
    x2 = F._byte_fc_mix_fwd(toks, Et, Eb, W, bpt=bpt, ids=ids, row_rnorm=rn2)
    assert torch.equal(x1, x2) and torch.equal(rn1, rn2)
    a = F.byte_fc_mix_backward(g, toks, Et, Eb, W, bpt=bpt, ids=ids, out=x1, row_rnorm=rn1)
    b = F.byte_fc_mix_backward(g, toks, Et, Eb, W, bpt=bpt, ids=ids, out=x1, row_rnorm=rn1)
    for k in a:
        if dt == "bf16" and k != "tok_table":
            err, r = np.abs(host(a[k] - b[k]).astype(np.float64)), np.abs(host(b[k]).astype(np.float64))
            assert (err <= 2 * (2.0 ** -8 * r + 4e-3 * r.max())).all(), k
        else:
            assert rel(host(a[k]), host(b[k])) < 2 * TOL


@pytest.mark.parametrize("dt", list(DTYPES))
def test_forward_and_backward_replay_from_a_hip_graph(mot, dt):
    """No memset or memcpy node, no allocation by the library, no sync: capture forward + backward, change the batch in place,
    replay, compare with the uncaptured calls."""
    Dm, Db, bpt, B, T, Vt, seed, case = SHAPES["S3"]
    toks, ids, pEt, pEb, pW, g = params("S3", DTYPES[dt])
    toks, ids, g = toks.clone(), ids.clone(), g.clone()
    F = mot.functional
    Et, Eb, W = pEt.detach(), pEb.detach(), pW.detach()
    rn = torch.empty((B, T), dtype=torch.float32, device=DEV)
    into = {"tok_table": torch.zeros_like(Et, dtype=torch.float32), "byte_table": torch.zeros_like(Eb, dtype=torch.float32),
            "byte_fc": torch.zeros_like(W, dtype=torch.float32)}
    x_static = torch.empty((B, T, Dm), dtype=DTYPES[dt], device=DEV)

    def step():
        x = F._byte_fc_mix_fwd(toks, Et, Eb, W, bpt=bpt, ids=ids, row_rnorm=rn)
        x_static.copy_(x)
        for v in into.values():
            v.zero_()
        F.byte_fc_mix_backward(g, toks, Et, Eb, W, bpt=bpt, ids=ids, out=x_static, row_rnorm=rn, into=into)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                      # warm-up on the capture stream: allocates the workspaces
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        step()
    rs = np.random.RandomState(8150)
    toks.copy_(dev(rs.randint(0, Vt, (B, T)).astype(np.int32)))
    ids.copy_(dev(rs.randint(0, gi.BYTE_VOCAB, (B, T * bpt)).astype(np.int64)))
    g.copy_(dev(bf.bf16_values(rs.standard_normal((B, T, Dm))), DTYPES[dt]))
    graph.replay()
    torch.cuda.synchronize()
    rn2 = torch.empty_like(rn)
    x = F._byte_fc_mix_fwd(toks, Et, Eb, W, bpt=bpt, ids=ids, row_rnorm=rn2)
    ref = F.byte_fc_mix_backward(g, toks, Et, Eb, W, bpt=bpt, ids=ids, out=x, row_rnorm=rn2)
    mot.check_status()
    assert torch.equal(x, x_static) and torch.equal(rn, rn2)
    for k in ref:
        if dt == "bf16" and k != "tok_table":
            err, r = np.abs(host(into[k] - ref[k]).astype(np.float64)), np.abs(host(ref[k]).astype(np.float64))
            assert (err <= 2 * (2.0 ** -8 * r + 4e-3 * r.max())).all(), k
        else:
            assert rel(host(into[k]), host(ref[k])) < 2 * TOL


@pytest.mark.parametrize("dt", list(DTYPES))
def test_out_of_range_byte_id_is_flagged_and_the_call_completes(mot, dt):
    Dm, Db, bpt, B, T, Vt, seed, case = SHAPES["S1"]
    toks, ids, pEt, pEb, pW, g = params("S1", DTYPES[dt])
    mot.check_status()
    bad = ids.clone()
    bad[1, 5] = gi.BYTE_VOCAB + 3
    x = mot.byte_fc_mix(toks, pEt.detach(), pEb.detach(), pW.detach(), bpt=bpt, ids=bad)
    torch.cuda.synchronize()
    assert torch.isfinite(x.float()).all()
    with pytest.raises(IndexError, match="byte id"):
        mot.check_status()
    mot.check_status()                                 # the word is cleared
    clamped = bad.clone()
    clamped[1, 5] = 0                                   # a bad id reads row 0
    assert torch.equal(x, mot.byte_fc_mix(toks, pEt.detach(), pEb.detach(), pW.detach(), bpt=bpt, ids=clamped))
    mot.check_status()


def test_empty_batch(mot):
    Et, Eb, W = torch.zeros(10, 64, device=DEV), torch.zeros(gi.BYTE_VOCAB, 8, device=DEV), torch.zeros(64, 64, device=DEV)
    x = mot.byte_fc_mix(torch.zeros((0, 4), dtype=torch.int32, device=DEV), Et, Eb, W, bpt=8, ids=torch.zeros((0, 32), dtype=torch.int64, device=DEV))
    assert x.shape == (0, 4, 64) and x.dtype == torch.float32
    x = mot.byte_fc_mix(torch.zeros((2, 0), dtype=torch.int32, device=DEV), Et, Eb, W, bpt=8, ids=torch.zeros((2, 0), dtype=torch.int64, device=DEV))
    assert x.shape == (2, 0, 64)


# ------------------------------------------------------------------------------------------------ module
@pytest.mark.parametrize("dt", list(DTYPES))
def test_front_end_module_end_to_end(mot, dt):
    Dm, Db, bpt, B, T, Vt, seed, case = SHAPES["S4"]
    toks, tab, ids, Et, Eb, W, g = problem("S4")
    fe = mot.ByteFcFrontEnd(Vt, gi.BYTE_VOCAB, Dm, Db, bytes_per_token=bpt, ttb=torch.from_numpy(tab)).to(DEV)
    with torch.no_grad():
        fe.embed_tokens.weight.copy_(dev(Et)); fe.embed_bytes.weight.copy_(dev(Eb)); fe.byte_fc.copy_(dev(W))
    fe = fe.to(DTYPES[dt])
    x_ids = fe(dev(toks), dev(ids))
    x_ttb = fe(dev(toks))
    mot.check_status()
    want = mot.byte_fc_mix(dev(toks), fe.embed_tokens.weight.detach(), fe.embed_bytes.weight.detach(), fe.byte_fc.detach(), bpt=bpt, ids=dev(ids))
    assert torch.equal(x_ids.detach(), want) and torch.equal(x_ttb.detach(), want)
    check_forward(want, reference("S4"), dt, "module S4")
    x1d = fe(dev(toks[0]), dev(ids[0]))                     # a single sequence, as the run feeds it
    assert torch.equal(x1d.detach()[0], want[0])
    # one SGD step
    opt = torch.optim.SGD(fe.parameters(), lr=0.01)
    before = fe.byte_fc.detach().clone()
    (x_ttb.float() * dev(g, torch.float32)).sum().backward()
    assert fe.byte_fc.grad.dtype == DTYPES[dt] == fe.embed_tokens.weight.grad.dtype == fe.embed_bytes.weight.grad.dtype
    opt.step()
    torch.cuda.synchronize()
    mot.check_status()
    assert not torch.equal(before, fe.byte_fc.detach()) and torch.isfinite(fe.byte_fc.detach().float()).all()


# ------------------------------------------------------------------------------------------------ against what exists
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", ["S3", "S5"])
def test_agrees_with_the_concat_linear_emulation(mot, name, dt):
    """embed_mix(mode="concat_linear") with the weight [I | byte_fc] computes the same mixin (twice the contraction)."""
    Dm, Db, bpt, B, T, Vt, seed, case = SHAPES[name]
    toks, tab, ids, Et, Eb, W, g = problem(name)
    t = lambda a: dev(a, DTYPES[dt])
    x = mot.byte_fc_mix(dev(toks), t(Et), t(Eb), t(W), bpt=bpt, ids=dev(ids))
    y = mot.embed_mix(dev(toks), t(Et), t(Eb), mode="concat_linear", bpt=bpt, ids_a=dev(ids), weight=t(bf.as_concat_linear_weight(W)), norm_out=True,
                      eps=bf.F32_EPS)
    mot.check_status()
    ref = reference(name)
    diff, bar = float((x.float() - y.float()).abs().max()), forward_bar(ref, dt)
    print(f"{name} {dt}: max|byte_fc_mix - concat_linear emulation| {diff:.3e}, bar {bar:.3e}")
    check_forward(y, ref, dt, name + " emulation")
    assert diff <= bar
