"""-m gpu: the write-once backward of the fused front-end (mot_embed_mix_bwd_once; functional.embed_mix_backward_once,
embed_mix(write_once=True), SumFrontEnd / ConcatFrontEnd(write_once_grads=True)) in float32 and bfloat16, against the float64
restatement of tests/embed_mix_once_ref.py evaluated with the kernels' epsilon on the same (bfloat16-valued) operands.  For "sum" and
"noop" that restatement is itself held to oracle.embed_mix_bwd(dtype=np.float64) to 1e-12.  Nothing here reads a reference checkout.

Cases: the smallest shapes at which the kernels can go wrong (token vocab; mode and flags; tok_dim / byte_dim / bpt; tokens):
  one     50   sum, run 71 (norm_out)                               32 / 8 / 4         (1,)                       one position, 49 absent rows
  n65     97   sum, run 71041 (norms, scales 0.7 / 1.3, norm_out)   64 / 16 / 4        (65,) uniform              a slice boundary
  hot     10   sum, run 71081 (norms, scales, no norm_out)          768 / 48 / 16      (300,) id 3 but ten        a group over 5 slices; 3 column blocks
  ends   100   concat, norm_out                                     32 / 8 / 4 (64)    (3, 50) ids 0 and 99       first and last row, token columns only
  noop    40   noop, norm_tok                                       16 / - / 0         (2, 96) FineWeb-shaped     no byte part
  wide    33   sum, run 71                                          2048 / 128 / 16    (130,)                     the widest row
  sorted  20   sum, run 71                                          64 / 16 / 4        (6200,), 6000 of one id    the LDS-sort canon; ~94 pieces in four quarters

Bars (the project's own: test_gpu_backward.py, test_gpu_value_embeds.py, test_gpu_split_x0.py):
  * fp32 table gradients: max|hip - ref64| <= 2e-5 max|ref64|;
  * a table gradient delivered in bf16 (the token table's; the bf16 .grad tensors autograd hands out): the same plus one bf16 step of
    the element, 2^-7 |ref64| elementwise;
  * scalar gradients (sums that can cancel): max(2 |ref_fp32 - ref64|, 2e-5 sum_n |contribution of position n|), ref_fp32 the
    restatement's float32 run;
  * the new path against today's embed_mix_backward on the same inputs: the same bars, with today's result in the reference's place.
"""
import functools

import numpy as np
import pytest
import torch

import embed_mix_once_ref as er
import golden_inputs as gi
from oracle import oracle as orc
from util_gpu import DEV, dev, host

pytestmark = pytest.mark.gpu
TOL = 2e-5
BYTE_ROWS = 458
RUN71 = dict(norm_out=True)
RUN71041 = dict(norm_tok=True, norm_byte=True, norm_out=True)
RUN71081 = dict(norm_tok=True, norm_byte=True, norm_out=False)
CASES = {   # name: (token vocab, mode, flags, scales, tok_dim, byte_dim, bpt, tokens' shape, seed)
    "one": (50, "sum", RUN71, None, 32, 8, 4, (1,), 9101),
    "n65": (97, "sum", RUN71041, (0.7, 1.3), 64, 16, 4, (65,), 9102),
    "hot": (10, "sum", RUN71081, (0.7, 1.3), 768, 48, 16, (300,), 9103),
    "ends": (100, "concat", RUN71, None, 32, 8, 4, (3, 50), 9104),
    "noop": (40, "noop", dict(norm_tok=True), None, 16, 0, 0, (2, 96), 9105),
    "wide": (33, "sum", RUN71, None, 2048, 128, 16, (130,), 9106),
    "sorted": (20, "sum", RUN71, None, 64, 16, 4, (6200,), 9107),
}
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
EPS = {"fp32": er.F32_EPS, "bf16": er.BF16_EPS}     # what the kernels take when no eps is given (F.rms_norm(eps=None) per dtype)
RUNS = [(n, dt) for n in CASES for dt in DTYPES]


@pytest.fixture(scope="module")
def mot():
    import mixture_of_tokenizers_amd as m
    return m


def make_tokens(name):
    Vt, mode, flags, scales, Dt, Db, bpt, shape, seed = CASES[name]
    rs = np.random.RandomState(seed)
    n = int(np.prod(shape))
    if name == "hot":
        toks = np.full(n, 3, dtype=np.int32)
        toks[rs.choice(n, 10, replace=False)] = rs.randint(4, Vt, 10)
    elif name == "ends":
        toks = np.where(rs.random_sample(n) < 0.5, 0, Vt - 1).astype(np.int32)
    elif name == "noop":
        toks = gi.fineweb_like_tokens(seed, shape[0], shape[1], vocab=Vt)
    elif name == "sorted":
        toks = rs.randint(0, Vt, n).astype(np.int32)
        toks[rs.choice(n, 6000, replace=False)] = 7
    else:
        toks = rs.randint(0, Vt, n).astype(np.int32)
    return toks.reshape(shape)


@functools.lru_cache(maxsize=None)
def problem(name):
    """Tokens, byte ids and the bfloat16-valued operands of a case: computed once and shared; no test writes to them."""
    Vt, mode, flags, scales, Dt, Db, bpt, shape, seed = CASES[name]
    toks = make_tokens(name)
    n = toks.size
    ids = np.random.RandomState(seed + 1).randint(0, BYTE_ROWS, (n, bpt)).astype(np.int64) if bpt else None
    Dm = Dt + bpt * Db if mode == "concat" else Dt
    return toks, ids, er.make_inputs(seed + 2, Vt, Dt, BYTE_ROWS, Db, n, Dm)


@functools.lru_cache(maxsize=None)
def reference(name, dt):
    """The float64 restatement with the epsilon the kernels take for `dt`, and its float32 run (for the scalar bars)."""
    Vt, mode, flags, scales, Dt, Db, bpt, shape, seed = CASES[name]
    toks, ids, inp = problem(name)
    kw = dict(mode=mode, bpt=bpt, scales=scales, eps=EPS[dt], **flags)
    return er.run(toks, ids, inp, dtype=torch.float64, **kw), er.run(toks, ids, inp, dtype=torch.float32, **kw)


def operands(name, dt, toks=None, ids=None):
    """The device tensors of a case and the keywords of the two backward calls."""
    Vt, mode, flags, scales, Dt, Db, bpt, shape, seed = CASES[name]
    ptoks, pids, inp = problem(name)
    toks = ptoks if toks is None else toks
    ids = pids if ids is None else ids
    t = DTYPES[dt]
    Dm = inp["g"].shape[1]
    kw = dict(mode=mode, bpt=bpt, **flags)
    if bpt:
        kw["ids_a"] = dev(ids.reshape(toks.reshape(-1, toks.shape[-1]).shape[0], -1))
    if scales:
        kw["scale_tok"], kw["scale_byte"] = dev(np.float32([scales[0]])), dev(np.float32([scales[1]]))
    g = dev(inp["g"], t).reshape(toks.shape + (Dm,))
    return g, dev(toks), dev(inp["Et"], t), (dev(inp["Eb"], t) if bpt else None), kw


def table_bar(ref, in_bf16):
    ref = np.asarray(ref, dtype=np.float64)
    return TOL * np.abs(ref).max() + (2.0 ** -7 * np.abs(ref) if in_bf16 else 0.0)


def check_table(got, ref, in_bf16, what):
    got, ref = host(got.double()).reshape(np.shape(ref)), np.asarray(ref, dtype=np.float64)
    assert np.isfinite(got).all(), what
    err, bar = np.abs(got - ref), table_bar(ref, in_bf16)
    print(f"{what}: max|hip - ref| {err.max():.3e}, max|ref| {np.abs(ref).max():.3e}, worst err / bar {np.max(err / np.maximum(bar, 1e-300)):.3f}")
    assert (err <= bar).all(), f"{what}: {int((err > bar).sum())} elements over the bar, worst err / bar {np.max(err / np.maximum(bar, 1e-300)):.3f}"


def scalar_bar(r64, r32, k):
    return max(2 * abs(r32["d_scale_" + k] - r64["d_scale_" + k]), TOL * r64["abs_scale_" + k])


def check_scalar(got, want, bar, what):
    got = float(got.double().reshape(-1)[0])
    print(f"{what}: hip {got!r}, ref {want!r}, |difference| {abs(got - want):.3e}, bar {bar:.3e}")
    assert abs(got - want) <= bar, f"{what}: |{got!r} - {want!r}| = {abs(got - want):.3e} over the bar {bar:.3e}"


def check_all(got, name, dt, what, byte_in_bf16=False):
    r64, r32 = reference(name, dt)
    check_table(got["tok_table"], r64["d_tok"], dt == "bf16", f"{what} d_tok")
    if r64["d_byte"] is not None:
        check_table(got["byte_table"], r64["d_byte"], byte_in_bf16, f"{what} d_byte")
    if CASES[name][3]:
        for k in ("tok", "byte"):
            check_scalar(got["scale_" + k], r64["d_scale_" + k], scalar_bar(r64, r32, k), f"{what} d_scale_{k}")


def same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("name", [n for n in CASES if CASES[n][1] in ("sum", "noop")])
def test_the_restatement_agrees_with_the_oracle_in_float64(name):
    Vt, mode, flags, scales, Dt, Db, bpt, shape, seed = CASES[name]
    toks, ids, inp = problem(name)
    r64, _ = reference(name, "fp32")
    s = scales or (1.0, 1.0)
    orc.set_eps(er.F32_EPS)
    try:
        o = orc.embed_mix_bwd(toks.reshape(-1), ids, None, inp["Et"], inp["Eb"], inp["g"], mode=mode, bpt=bpt, scale_tok=s[0], scale_byte=s[1],
                              dtype=np.float64, **flags)
    finally:
        orc.set_eps(0.0)
    assert np.abs(o["tok_table"] - r64["d_tok"]).max() <= 1e-12 * np.abs(r64["d_tok"]).max()
    if mode == "sum":
        assert np.abs(o["byte_table"] - r64["d_byte"]).max() <= 1e-12 * np.abs(r64["d_byte"]).max()
        assert abs(o["scales"][1] - r64["d_scale_byte"]) <= 1e-12 * r64["abs_scale_byte"]
    assert abs(o["scales"][0] - r64["d_scale_tok"]) <= 1e-12 * r64["abs_scale_tok"]


# ------------------------------------------------------------------------------------------------ the direct call
@pytest.mark.parametrize("name,dt", RUNS)
def test_backward_writes_every_element_once_with_the_same_bits(mot, name, dt):
    Fm = mot.functional
    Vt, mode, flags, scales, Dt, Db, bpt, shape, seed = CASES[name]
    g, tok, Et, Eb, kw = operands(name, dt)
    nan = lambda shape, t: torch.full(shape, float("nan"), dtype=t, device=DEV)
    bufs = {"tok_table": nan((Vt, Dt), DTYPES[dt])}
    if bpt:
        bufs["byte_table"] = nan((BYTE_ROWS, Db), torch.float32)
    if scales:
        bufs["scale_tok"], bufs["scale_byte"] = nan((1,), torch.float32), nan((1,), torch.float32)
    got = Fm.embed_mix_backward_once(g, tok, Et, Eb, out=bufs, **kw)
    mot.check_status()
    assert got.keys() == bufs.keys()
    for k in bufs:
        assert got[k] is bufs[k] and not torch.isnan(got[k]).any(), f"{k}: {int(torch.isnan(got[k]).sum())} elements were never written"
    assert got["tok_table"].dtype == DTYPES[dt]
    check_all(got, name, dt, f"{name} {dt}")
    absent = np.setdiff1d(np.arange(Vt), problem(name)[0])
    rows = got["tok_table"][dev(absent)].float()
    assert not rows.any() and not torch.signbit(rows).any()                        # +0, not a small number and not -0
    again = Fm.embed_mix_backward_once(g, tok, Et, Eb, **kw)                        # fresh (uninitialised) buffers, a second run
    same_bits(got, again)
    order = Fm.token_order(tok, Vt)
    same_bits(got, Fm.embed_mix_backward_once(g, tok, Et, Eb, token_order=order, **kw))   # the caller's order, or one made in the call
    only = Fm.embed_mix_backward_once(g, tok, Et, Eb, want_grads=["tok_table"], **kw)
    assert list(only) == ["tok_table"] and torch.equal(only["tok_table"], got["tok_table"])
    mot.check_status()


@pytest.mark.parametrize("name,dt", RUNS)
def test_the_new_path_agrees_with_todays_backward(mot, name, dt):
    Fm = mot.functional
    g, tok, Et, Eb, kw = operands(name, dt)
    new = Fm.embed_mix_backward_once(g, tok, Et, Eb, **kw)
    old = Fm.embed_mix_backward(g, tok, Et, Eb, **kw)
    check_table(new["tok_table"], host(old["tok_table"].double()), dt == "bf16", f"{name} {dt} d_tok against today's")
    if Eb is not None:
        check_table(new["byte_table"], host(old["byte_table"].double()), False, f"{name} {dt} d_byte against today's")
    if CASES[name][3]:
        r64, r32 = reference(name, dt)
        for k in ("tok", "byte"):
            check_scalar(new["scale_" + k], float(old["scale_" + k].double()[0]), scalar_bar(r64, r32, k), f"{name} {dt} d_scale_{k} against today's")
    mot.check_status()


# ------------------------------------------------------------------------------------------------ hipGraph
@pytest.mark.parametrize("name,dt", [("n65", "fp32"), ("n65", "bf16"), ("ends", "bf16"), ("sorted", "fp32")])
def test_a_hip_graph_replay_gives_the_eager_bits(mot, name, dt):
    """No memset or memcpy node, no allocation by the library, no sync, the token order made inside the capture: capture the call,
    replay, compare with the eager call; copy a second batch into the token and id buffers, replay, compare with an eager run on it."""
    Fm = mot.functional
    Vt, mode, flags, scales, Dt, Db, bpt, shape, seed = CASES[name]
    g, tok, Et, Eb, kw = operands(name, dt)
    tok, kw["ids_a"] = tok.clone(), kw["ids_a"].clone()
    eager = Fm.embed_mix_backward_once(g, tok, Et, Eb, **kw)
    bufs = {k: torch.empty_like(v) for k, v in eager.items()}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        Fm.embed_mix_backward_once(g, tok, Et, Eb, out=bufs, **kw)             # allocates this stream's workspace
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        Fm.embed_mix_backward_once(g, tok, Et, Eb, out=bufs, **kw)
    for b in bufs.values():
        b.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    same_bits(bufs, eager)
    rs = np.random.RandomState(seed + 7)
    toks2 = rs.randint(0, Vt, shape).astype(np.int32)
    toks2.reshape(-1)[: toks2.size // 2] = 5                                      # another hot id, other absent rows
    ids2 = rs.randint(0, BYTE_ROWS, tuple(kw["ids_a"].shape)).astype(np.int64)
    tok.copy_(dev(toks2))
    kw["ids_a"].copy_(dev(ids2))
    graph.replay()
    torch.cuda.synchronize()
    same_bits(bufs, Fm.embed_mix_backward_once(g, tok, Et, Eb, **kw))
    mot.check_status()


# ------------------------------------------------------------------------------------------------ autograd
def front_end(mot, name, dt):
    Vt, mode, flags, scales, Dt, Db, bpt, shape, seed = CASES[name]
    M = mot.modules
    if mode == "concat":
        m = M.ConcatFrontEnd(Vt, BYTE_ROWS, Dt, Db, bpt, write_once_grads=True)
    else:
        variant = {id(RUN71): "71", id(RUN71041): "71041", id(RUN71081): "71081"}[id(flags)]
        m = M.SumFrontEnd(Vt, BYTE_ROWS, Dt, Db, bpt, variant=variant, write_once_grads=True)
    m = m.to(DEV)
    inp = problem(name)[2]
    with torch.no_grad():
        m.embed_tokens.weight.copy_(dev(inp["Et"], torch.float32))
        m.embed_bytes.weight.copy_(dev(inp["Eb"], torch.float32))
        if scales:
            m.scalars.copy_(dev(np.float32([scales[1], scales[0]])))              # [-2] bytes, [-1] tokens
    m.embed_tokens.to(DTYPES[dt])
    m.embed_bytes.to(DTYPES[dt])
    return m


@pytest.mark.parametrize("name,dt", [(n, dt) for n in ("n65", "hot", "ends", "sorted") for dt in DTYPES])
def test_autograd_through_the_front_end_modules(mot, name, dt):
    Vt, mode, flags, scales, Dt, Db, bpt, shape, seed = CASES[name]
    toks, ids, inp = problem(name)
    m = front_end(mot, name, dt)
    g = dev(inp["g"], DTYPES[dt]).reshape(toks.shape + (-1,))
    rows = 1 if toks.ndim == 1 else toks.shape[0]
    x = m(dev(toks), dev(ids.reshape(rows, -1)))
    assert type(x.grad_fn).__name__.startswith("_EmbedMixOnceFn")
    x.backward(g.reshape(x.shape), retain_graph=True)
    mot.check_status()
    params = dict(tok_table=m.embed_tokens.weight, byte_table=m.embed_bytes.weight)
    for k, p in params.items():
        assert p.grad.dtype == p.dtype == DTYPES[dt] and p.grad.shape == p.shape, k
    got = {k: p.grad for k, p in params.items()}
    if scales:
        assert m.scalars.grad.dtype == torch.float32
        got["scale_byte"], got["scale_tok"] = m.scalars.grad[0:1], m.scalars.grad[1:2]
    check_all(got, name, dt, f"{name} {dt} .grad", byte_in_bf16=dt == "bf16")
    first = {k: v.clone() for k, v in got.items()}
    x.backward(g.reshape(x.shape))                                                 # a second backward accumulates: the same bits twice
    for k, p in params.items():
        assert torch.equal(p.grad, first[k] + first[k]), k
    if scales:
        assert torch.equal(m.scalars.grad, torch.cat([first["scale_byte"], first["scale_tok"]]) * 2)
    mot.check_status()


@pytest.mark.parametrize("name,dt", [("n65", "bf16"), ("ends", "fp32")])
def test_forward_and_backward_through_a_module_replay_from_a_hip_graph(mot, name, dt):
    """The autograd node inside a capture: the token order is made in line, nothing comes from outside the capture.  Capture forward +
    backward, copy a new batch into the token and id buffers, replay, compare with an eager step of a second module on that batch."""
    Vt, mode, flags, scales, Dt, Db, bpt, shape, seed = CASES[name]
    toks, ids, inp = problem(name)
    rows = 1 if toks.ndim == 1 else toks.shape[0]
    m, fresh = front_end(mot, name, dt), front_end(mot, name, dt)
    tok, bid = dev(toks), dev(ids.reshape(rows, -1))
    g = dev(inp["g"], DTYPES[dt])

    def step(mod):
        x = mod(tok, bid)
        x.backward(g.reshape(x.shape))
        return x

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(m)                                                     # allocates the workspaces
        for p in m.parameters():
            p.grad = None
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        x = step(m)
    rs = np.random.RandomState(seed + 9)
    tok.copy_(dev(rs.randint(0, Vt, shape).astype(np.int32)))       # a new batch, the same buffers
    bid.copy_(dev(rs.randint(0, BYTE_ROWS, tuple(bid.shape)).astype(np.int64)))
    graph.replay()
    torch.cuda.synchronize()
    want = step(fresh)
    mot.check_status()
    assert torch.equal(x, want)
    for p, q in zip(m.parameters(), fresh.parameters()):
        assert q.grad.abs().max() > 0 and p.grad.dtype == q.grad.dtype
        assert torch.equal(p.grad, q.grad)                          # the same bits, replayed or eager


def test_the_noop_mode_through_embed_mix(mot):
    for dt in DTYPES:
        g, tok, Et, _, kw = operands("noop", dt)
        Et = Et.clone().requires_grad_(True)
        x = mot.embed_mix(tok, Et, mode="noop", norm_tok=True, write_once=True)
        x.backward(g)
        assert Et.grad.dtype == DTYPES[dt]
        check_table(Et.grad, reference("noop", dt)[0]["d_tok"], dt == "bf16", f"noop {dt} .grad")
    mot.check_status()


def test_the_default_leaves_todays_path_as_it_is(mot):
    g, tok, Et, Eb, kw = operands("n65", "fp32")
    Et, Eb = Et.clone().requires_grad_(True), Eb.clone().requires_grad_(True)
    a = mot.embed_mix(tok, Et, Eb, **kw)
    b = mot.embed_mix(tok, Et, Eb, write_once=False, **kw)
    c = mot.embed_mix(tok, Et, Eb, write_once=True, **kw)
    assert torch.equal(a, b) and torch.equal(a, c)
    assert type(a.grad_fn) is type(b.grad_fn) and type(a.grad_fn) is not type(c.grad_fn)
    with torch.no_grad():
        assert torch.equal(mot.embed_mix(tok, Et, Eb, write_once=False, **kw), mot.embed_mix(tok, Et, Eb, **kw))
    mot.check_status()


# ------------------------------------------------------------------------------------------------ ids out of range
@pytest.mark.parametrize("which, bad", [("token", 97 + 7), ("token", -1), ("byte", BYTE_ROWS)])
def test_an_id_out_of_range_is_flagged_and_counted_as_row_zero(mot, which, bad):
    Fm = mot.functional
    name, dt = "n65", "fp32"
    Vt, mode, flags, scales, Dt, Db, bpt, shape, seed = CASES[name]
    toks, ids, inp = problem(name)
    toks, ids = toks.copy(), ids.copy()
    if which == "token":
        toks[[5, 64]] = bad
    else:
        ids[[5, 64], [0, 3]] = bad
    g, tok, Et, Eb, kw = operands(name, dt, toks, ids)
    mot.check_status()
    got = Fm.embed_mix_backward_once(g, tok, Et, Eb, **kw)
    with pytest.raises(IndexError):
        mot.check_status()
    ctoks = np.where((toks >= 0) & (toks < Vt), toks, 0)
    cids = np.where((ids >= 0) & (ids < BYTE_ROWS), ids, 0)
    rkw = dict(mode=mode, bpt=bpt, scales=scales, eps=EPS[dt], **flags)
    r64, r32 = er.run(ctoks, cids, inp, dtype=torch.float64, **rkw), er.run(ctoks, cids, inp, dtype=torch.float32, **rkw)
    check_table(got["tok_table"], r64["d_tok"], False, f"bad {which} id {bad} d_tok")
    check_table(got["byte_table"], r64["d_byte"], False, f"bad {which} id {bad} d_byte")
    for k in ("tok", "byte"):
        check_scalar(got["scale_" + k], r64["d_scale_" + k], scalar_bar(r64, r32, k), f"bad {which} id {bad} d_scale_{k}")
    mot.check_status()
