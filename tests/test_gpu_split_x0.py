"""-m gpu: run 71081's three streams in one call -- x0t = norm(E_t[tok]), x0b = cat_k norm(E_b[id_k]), x = s_t x0t + s_b x0b
(mot.split_x0, MotSplitX0Desc; modded-nanogpt/runs/71081_mot-in_toks-valemb.py:302-304, 315) -- forward and backward, float32 and
bfloat16, against the reference's own runs (tests/golden/split_x0.npz) and the float64 restatement of tests/split_x0_ref.py evaluated
with the kernels' epsilon on the same (bfloat16-valued) operands.  Nothing here reads a reference checkout.

Shapes: the smallest at which a kernel can go wrong (D / byte_dim / bpt, B x T), and the forward instantiation <T, NCH, U> each takes
(fp32, bf16; bf16 needs byte_dim % 8 == 0, so the byte_dim 4 shapes run in fp32 only):
  S1a-e the five fixture cases                  fp32 <1,4>, bf16 <1,4>     parity against the reference itself; S1e is one token
  S2    1024 / 64 / 16, 1 x 1000                fp32 <4,1>, bf16 <2,2>     the run's dims; T no multiple of 16, 32 or 64: a ragged last unit, the halo walk
  S3     768 / 48 / 16, 4 x 333                 fp32 <4,1>, bf16 <2,2>     headline dims, several rows, a byte row of 12 / 6 chunks; idle lanes in the last chunk
  S4a   2048 / 128 / 16, 1 x 130                fp32 <8,1>, bf16 <4,1>     the largest row: most chunks per lane
  S4b     64 / 4 / 16, 1 x 130                  fp32 <1,4>                 the smallest row: 16 of 64 lanes busy
  S5     128 / 8 / 16, 1 x 2048                 every token id 3 except ten: a group of 2038 positions crosses 31 slice boundaries of the write-once sums
  S6     128 / 8 / 16, 100 token rows, 3 x 50   only ids 0 and 99: the table's ends; 98 absent rows must be +0
  S7a    256 / 16 / 16, 1 x 16 424              two slabs of the backward (16 384 + 40), 1027 scalar partials over 256 threads; unit 16
  S7b    256 / 16 / 16, 2 x 65 541              131 082 tokens: the forward's unit of 32 (forward only: the backward has no such branch)
Launcher branches: ids from the token->byte table (int16, pull left) and ids given -- every parity test runs both and wants the same
bits; one slab (all but S7a) and two; a token order supplied and made in the call; each result of the backward wanted and not.

  I1-I5  128 / 8 / 16, 3 x 150                  the index phase's other instantiations inside this kernel: pull right and no pull (int16), and an
                                                int32 table with pull left, right and none; ids, counters and outputs against the oracle's ids
  I6, I7 512 / 8 / 64, 2 x 150                  bpt 64 from a token->byte table: 50 KB (int16, left) and 84 KB (int32, right) of LDS per workgroup,
                                                the dynamic-LDS opt-in of the launcher, in <fp32,4,1> and <bf16,1,4>
Launcher branches, continued: out_ids_padded, out_ids_pulled and counters are written and compared with the oracle (I1-I7); the
autograd node with ids made in the kernel -- the forward writes them, the backward reads them -- runs for pull left / right / none
(I1, I2, I3, I6) and through SplitX0FrontEnd with its attached table (S3).

Bars (the family's own, against the float64 restatement on the same inputs; S1 also against the fixture -- its float32 and bfloat16
outputs and its float64 scalar gradients in all five cases, its float64 table gradients as FIXTURE_F64 below lists and explains):
  * fp32 forward: 1e-6 + 1e-6 |ref| elementwise, each of the three outputs;
  * bf16 x0t and x0b (one rounding): at most one bf16 step from the float64 result rounded once, more than 98 % identical;
  * bf16 x (three rounding points): max|hip - f64| <= 2 max|ref_bf16 - f64|, ref_bf16 the restatement's own bfloat16 run (the
    reference's own for S1);
  * table gradients: fp32, and the fp32 sums from bf16 operands, 2e-5 max|ref64|; a token-table gradient delivered in bf16 and the
    bf16 .grad tensors autograd hands out: elementwise 2^-8 |ref| + 4e-3 max|ref|;
  * scalar gradients (sums that can cancel): max(2 |ref_fp32 - ref64|, 2e-5 sum_n |g_x[n] . x0.[n]|), ref_fp32 the restatement's float32 run.
"""
import functools

import numpy as np
import pytest
import torch

import golden_inputs as gi
import split_x0_ref as sx
from oracle import oracle as orc
from util_gpu import DEV, assert_close, dev, host

pytestmark = pytest.mark.gpu
TOL = 2e-5
SHAPES = {   # name: (D, byte_dim, bpt, B, T, token vocab, seed, fixture case)
    "S1a": (64, 4, 16, 2, 24, 40, 8101, "d64_b4_bpt16"),
    "S1b": (128, 8, 16, 2, 24, 40, 8102, "d128_b8_bpt16"),
    "S1c": (96, 24, 4, 3, 20, 40, 8103, "d96_b24_bpt4"),
    "S1d": (64, 8, 8, 2, 24, 40, 8104, "d64_b8_bpt8_small"),
    "S1e": (64, 4, 16, 1, 1, 40, 8105, "d64_b4_bpt16_one"),
    "S2": (1024, 64, 16, 1, 1000, 300, 8202, None),
    "S3": (768, 48, 16, 4, 333, 300, 8203, None),
    "S4a": (2048, 128, 16, 1, 130, 300, 8204, None),
    "S4b": (64, 4, 16, 1, 130, 300, 8205, None),
    "S5": (128, 8, 16, 1, 2048, 40, 8206, None),
    "S6": (128, 8, 16, 3, 50, 100, 8207, None),
    "S7a": (256, 16, 16, 1, 16424, 300, 8208, None),
}
# The float64 gradients of the fixture each S1 case is held to (its outputs and scalar gradients always are).  Left out: the table
# gradients of S1d, the case built so that the epsilon matters (the float64 epsilon of the reference's float64 run moves them by
# 1.3e-4 and 9.0e-4 of their largest element, the bar is 2e-5), and the byte-table gradient of S1e (one token, a 4-column byte row of
# small norm: 1.7e-5).  Those are held to the float64 restatement with the kernels' epsilon alone.
FIXTURE_F64 = {"S1a": ("d_tok", "d_byte", "d_scale_tok", "d_scale_byte"), "S1b": ("d_tok", "d_byte", "d_scale_tok", "d_scale_byte"),
               "S1c": ("d_tok", "d_byte", "d_scale_tok", "d_scale_byte"), "S1d": ("d_scale_tok", "d_scale_byte"),
               "S1e": ("d_tok", "d_scale_tok", "d_scale_byte")}
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
RUNS = [(n, dt) for n in SHAPES for dt in DTYPES if dt == "fp32" or SHAPES[n][1] % 8 == 0]


@pytest.fixture(scope="module")
def mot():
    import mixture_of_tokenizers_amd as m
    return m


@functools.lru_cache(maxsize=None)
def golden():
    return sx.load_golden()


def shape_tokens(name):
    D, Db, bpt, B, T, Vt, seed, case = SHAPES[name]
    rs = np.random.RandomState(seed)
    e = Vt - 1
    if name == "S5":     # long runs of one token in the write-once sums
        toks = np.full((B, T), 3, dtype=np.int32)
        toks[0, rs.choice(T, 10, replace=False)] = rs.randint(4, Vt, 10)
        return toks
    if name == "S6":     # the table's ends only
        return np.where(rs.random_sample((B, T)) < 0.5, 0, e).astype(np.int32)
    toks = rs.randint(0, Vt - 1, size=(B, T)).astype(np.int32)
    toks[rs.random_sample((B, T)) < 0.1] = 0
    toks[0, 0] = toks[0, T // 2] = toks[B - 1, 3] = toks[B - 1, 4] = e     # EOT at a row start, mid-row and twice in a row
    return toks


@functools.lru_cache(maxsize=None)
def problem(name):
    """Inputs of a shape as numpy arrays (float64 arrays of bfloat16 values): computed once and shared; no test writes to them."""
    D, Db, bpt, B, T, Vt, seed, case = SHAPES[name]
    if case:
        toks, tab, inp = sx.case_tokens(case), sx.case_ttb(case), sx.case_inputs(case)
        ids = golden()[sx.key(case, "ids")].astype(np.int64)
    else:
        toks, tab = shape_tokens(name), gi.synth_ttb(seed + 1, Vt, bpt, "left")
        inp = sx.make_inputs(seed, Vt, D, Db, B, T)
        ids = orc.pull_from_left(orc.tokens_to_bytes(toks, tab.astype(np.float32)), bpt, gi.PAD, gi.EOT).astype(np.int64)
    return toks, tab, ids, inp


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 restatement with the kernels' epsilon, and the float32 / bfloat16 runs it is compared with (the reference's own
    outputs for the fixture cases)."""
    D, Db, bpt, B, T, Vt, seed, case = SHAPES[name]
    toks, tab, ids, inp = problem(name)
    r = {k: sx.run(toks, ids, inp, bpt=bpt, dtype=dt, eps=sx.F32_EPS) for k, dt in (("f64", torch.float64), ("fp32", torch.float32), ("bf16", torch.bfloat16))}
    if case:
        # The reference's own runs.  Its bfloat16 run took the float32 epsilon, the kernels' (asserted here: the restatement has its
        # bits, so the bf16 bars above ARE bars against the fixture); its float32 outputs are held to the family's 1e-6; its float64
        # run took the float64 epsilon, which moves some quantities by more than a gradient bar allows, so FIXTURE_F64 lists, case by
        # case, the float64 gradients that are compared -- and for each of them the shift between the two epsilons is asserted here
        # to be under a quarter of its bar (a property of the two float64 runs, not of the kernels).
        fx = r["fixture"] = {}
        for w in sx.OUTS:
            np.testing.assert_array_equal(r["bf16"][w], golden()[sx.key(case, f"bf16/{w}")].astype(np.float64))
            fx["fp32/" + w] = golden()[sx.key(case, f"f32/{w}")].astype(np.float64)
            fx["f64/" + w] = golden()[sx.key(case, f"f64/{w}")]
        for what in FIXTURE_F64[name]:
            fx[what] = golden()[sx.key(case, f"f64/{what}")]
            if what in ("d_tok", "d_byte"):
                assert sx.rel_err(r["f64"][what], fx[what]) < TOL / 4, (name, what)
    return r


def params(name, dtype):
    toks, tab, ids, inp = problem(name)
    s = dev(np.array([1.25, sx.S_BYTE, sx.S_TOK], dtype=np.float32))   # the two at the end of a longer tensor, as in the run
    g = {w: (None if a is None else dev(a, dtype)) for w, a in inp["g"].items()}
    return dev(toks), dev(tab), dev(ids), dev(inp["tok_table"], dtype), dev(inp["byte_table"], dtype), s, g


def bf16_steps(got, ref64):
    """distance in bf16 steps between a bf16 tensor and the float64 reference rounded once"""
    r = torch.tensor(ref64, dtype=torch.float64).to(torch.bfloat16)
    key = lambda t: (lambda v: torch.where(v < 0, -(v & 0x7fff), v))(t.cpu().view(torch.int16).int())
    return (key(got) - key(r)).abs().numpy()


def check_forward(outs, ref, dt, what):
    for w in sx.OUTS:
        if w not in outs:
            continue
        got, f64 = outs[w], ref["f64"][w]
        assert tuple(got.shape) == f64.shape and np.isfinite(host(got.float())).all(), (what, w)
        if dt == "fp32":
            err = float(np.abs(host(got).astype(np.float64) - f64).max())
            print(f"{what} {w} fp32: max|hip - f64| {err:.3e}")
            assert_close(host(got), f64)
        elif w == "x":
            err, bar = float(np.abs(host(got.float()).astype(np.float64) - f64).max()), 2 * float(np.abs(ref["bf16"][w] - f64).max())
            print(f"{what} x bf16: max|hip - f64| {err:.3e}, bar {bar:.3e}, error over bar {err / bar:.3f}")
            assert err <= bar, (what, err, bar)
        else:
            steps = bf16_steps(got, f64)
            same = float((steps == 0).mean())
            print(f"{what} {w} bf16: {100 * same:.2f} % identical to the float64 result rounded once, largest distance {int(steps.max())} step(s)")
            assert steps.max() <= 1 and same > 0.98, (what, w, int(steps.max()), same)


def table_bar(r, rounded):
    return 2.0 ** -8 * np.abs(r) + 4e-3 * np.abs(r).max() if rounded else np.full(r.shape, TOL * np.abs(r).max())


def check_table(got, r, rounded, what):
    got = host(got.float()).astype(np.float64)
    err, bar = np.abs(got - r), table_bar(r, rounded)
    print(f"{what}: max error {err.max():.3e}, max|ref| {np.abs(r).max():.3e}, worst error over bar {float((err / np.maximum(bar, 1e-300)).max()):.3f}")
    assert np.isfinite(got).all() and (err <= bar).all(), (what, float(err.max()))


def check_scalars(res, ref, inp, what):
    gx = inp["g"]["x"]
    for k, w in (("scale_tok", "x0t"), ("scale_byte", "x0b")):
        r64, r32 = float(ref["f64"]["d_" + k]), float(ref["fp32"]["d_" + k])
        mass = 0.0 if gx is None else float(np.abs(gx * ref["f64"][w]).sum())
        bar = max(2 * abs(r32 - r64), TOL * mass)
        got = float(res[k].item())
        print(f"{what} d_{k}: hip {got:.9g}, f64 {r64:.9g}, fp32 restatement {r32:.9g}, |hip - f64| {abs(got - r64):.3e}, bar {bar:.3e}")
        assert abs(got - r64) <= bar, (what, k, got, r64, bar)


def call_fwd(mot, toks, tab, ids, Et, Eb, s, bpt, src, want=sx.OUTS):
    kw = dict(ttb=tab, pull="left") if src == "ttb" else dict(ids=ids)
    return dict(zip(want, mot.split_x0(toks, Et, Eb, s[2:3], s[1:2], bpt=bpt, want=want, **kw)))


def call_bwd(mot, g, toks, ids, Et, Eb, s, bpt, **kw):
    return mot.functional.split_x0_backward(g["x0t"], g["x0b"], g["x"], toks, Et, Eb, s[2:3], s[1:2], bpt=bpt, ids=ids, **kw)


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("name, dt", RUNS)
def test_forward_and_backward_against_float64(mot, name, dt):
    D, Db, bpt, B, T, Vt, seed, case = SHAPES[name]
    toks, tab, ids, Et, Eb, s, g = params(name, DTYPES[dt])
    ref = reference(name)
    outs = call_fwd(mot, toks, tab, ids, Et, Eb, s, bpt, "given")
    outs_ttb = call_fwd(mot, toks, tab, ids, Et, Eb, s, bpt, "ttb")
    mot.check_status()
    for w in sx.OUTS:
        assert torch.equal(outs[w], outs_ttb[w]), f"{name} {w}: ids from the token->byte table and ids given differ"
    check_forward(outs, ref, dt, name)
    res = call_bwd(mot, g, toks, ids, Et, Eb, s, bpt)
    mot.check_status()
    assert res["tok_table"].dtype == DTYPES[dt] and res["byte_table"].dtype == torch.float32
    check_table(res["tok_table"], ref["f64"]["d_tok"], dt == "bf16", f"{name} {dt} d_tok")
    check_table(res["byte_table"], ref["f64"]["d_byte"], False, f"{name} {dt} d_byte (fp32 sums)")
    check_scalars(res, ref, problem(name)[3], f"{name} {dt}")
    if case:   # the reference's own runs (FIXTURE_F64 says which float64 gradients; the bf16 outputs' bars above are the fixture's)
        fx = ref["fixture"]
        if dt == "fp32":
            for w in sx.OUTS:
                assert_close(host(outs[w]), fx["fp32/" + w])
        for k, what in (("tok_table", "d_tok"), ("byte_table", "d_byte")):
            if what in fx:
                check_table(res[k], fx[what], dt == "bf16" and k == "tok_table", f"{name} {dt} {what} vs the fixture's float64 run")
        fixture_ref = {"f64": {**{w: fx["f64/" + w] for w in sx.OUTS}, "d_scale_tok": fx["d_scale_tok"], "d_scale_byte": fx["d_scale_byte"]}, "fp32": ref["fp32"]}
        check_scalars(res, fixture_ref, problem(name)[3], f"{name} {dt} vs the fixture's float64 run")
    if name == "S6":   # absent rows: +0, bit for bit
        absent = torch.ones(Vt, dtype=torch.bool)
        absent[[0, Vt - 1]] = False
        rows = res["tok_table"][absent.to(DEV)]
        assert rows.numel() == 98 * D and not rows.view(torch.int16 if dt == "bf16" else torch.int32).any()


@pytest.mark.parametrize("dt", list(DTYPES))
def test_the_unit_of_32_tokens(mot, dt):
    """S7b, forward only: 131 082 tokens take the unit of 32; the float64 restatement runs in torch on the device."""
    D, Db, bpt, B, T, Vt, seed = 256, 16, 16, 2, 65541, 300, 8209
    rs = np.random.RandomState(seed)
    toks = rs.randint(0, Vt, size=(B, T)).astype(np.int32)
    tab = gi.synth_ttb(seed + 1, Vt, bpt, "left")
    ids = orc.pull_from_left(orc.tokens_to_bytes(toks, tab.astype(np.float32)), bpt, gi.PAD, gi.EOT).astype(np.int64)
    inp = sx.make_inputs(seed, Vt, D, Db, 1, 1)
    Et, Eb = dev(inp["tok_table"], DTYPES[dt]), dev(inp["byte_table"], DTYPES[dt])
    s = dev(np.array([1.25, sx.S_BYTE, sx.S_TOK], dtype=np.float32))
    t_toks, t_tab, t_ids = dev(toks), dev(tab), dev(ids)
    outs = call_fwd(mot, t_toks, t_tab, t_ids, Et, Eb, s, bpt, "given")
    outs_ttb = call_fwd(mot, t_toks, t_tab, t_ids, Et, Eb, s, bpt, "ttb")
    mot.check_status()
    with torch.no_grad():
        f = lambda d: [o.cpu().double().numpy() for o in sx.forward(t_toks, t_ids, Et.to(d), Eb.to(d), s[2].to(torch.float64 if d == torch.float64 else torch.float32),
                                                                    s[1].to(torch.float64 if d == torch.float64 else torch.float32), bpt=bpt, eps=sx.F32_EPS)]
        ref = {"f64": dict(zip(sx.OUTS, f(torch.float64))), "bf16": dict(zip(sx.OUTS, f(torch.bfloat16)))}
    for w in sx.OUTS:
        assert torch.equal(outs[w], outs_ttb[w]), w
    check_forward(outs, ref, dt, "S7b")


# ------------------------------------------------------------------------------------------------ the contract of the call
@pytest.mark.parametrize("dt", list(DTYPES))
def test_each_output_alone_has_the_bits_of_all_three(mot, dt):
    D, Db, bpt, B, T, Vt, seed, case = SHAPES["S3"]
    toks, tab, ids, Et, Eb, s, g = params("S3", DTYPES[dt])
    both = call_fwd(mot, toks, tab, ids, Et, Eb, s, bpt, "given")
    for src in ("given", "ttb"):
        for w in sx.OUTS:
            assert torch.equal(call_fwd(mot, toks, tab, ids, Et, Eb, s, bpt, src, want=(w,))[w], both[w]), (src, w)
    pair = call_fwd(mot, toks, tab, ids, Et, Eb, s, bpt, "given", want=("x", "x0t"))
    assert list(pair) == ["x", "x0t"] and torch.equal(pair["x"], both["x"]) and torch.equal(pair["x0t"], both["x0t"])


@pytest.mark.parametrize("dt", list(DTYPES))
def test_backward_bits_and_buffers(mot, dt):
    """A NULL output gradient is a zero one; the token table's gradient is WRITTEN (a NaN-filled buffer comes back clean) with the
    same bits on every run, with and without a supplied token order; the scalars likewise; the byte table's is ADDED to what the
    buffer held and stays inside its parity bar on every run."""
    D, Db, bpt, B, T, Vt, seed, case = SHAPES["S3"]
    toks, tab, ids, Et, Eb, s, g = params("S3", DTYPES[dt])
    ref = reference("S3")["f64"]
    a = call_bwd(mot, g, toks, ids, Et, Eb, s, bpt)
    nan = torch.full_like(Et, float("nan"))
    held = torch.full((gi.BYTE_VOCAB, Db), 1.5, dtype=torch.float32, device=DEV)
    order = mot.functional.token_order(toks, Vt)
    b = call_bwd(mot, g, toks, ids, Et, Eb, s, bpt, out=nan, into=held, token_order=order)
    mot.check_status()
    assert b["tok_table"] is nan and b["byte_table"] is held
    assert torch.equal(a["tok_table"], b["tok_table"]) and torch.equal(a["scale_tok"], b["scale_tok"]) and torch.equal(a["scale_byte"], b["scale_byte"])
    check_table(a["byte_table"], ref["d_byte"], False, f"S3 {dt} d_byte, first run")
    check_table(held - 1.5, ref["d_byte"] , False, f"S3 {dt} d_byte, += into a buffer of 1.5")
    # one gradient absent against the same gradient as zeros, for each of the three
    for w in sx.OUTS:
        gn, gz = dict(g, **{w: None}), dict(g, **{w: torch.zeros_like(g[w])})
        n, z = call_bwd(mot, gn, toks, ids, Et, Eb, s, bpt), call_bwd(mot, gz, toks, ids, Et, Eb, s, bpt)
        assert torch.equal(n["tok_table"], z["tok_table"]) and torch.equal(n["scale_tok"], z["scale_tok"]) and torch.equal(n["scale_byte"], z["scale_byte"]), w
        bar = 2 * TOL * float(z["byte_table"].abs().max())
        assert float((n["byte_table"] - z["byte_table"]).abs().max()) <= bar, w
    # only some results wanted: the others are not touched, the wanted ones keep their bits
    only = call_bwd(mot, g, toks, ids, Et, Eb, s, bpt, want_grads=("tok_table", "scale_byte"))
    assert sorted(only) == ["scale_byte", "tok_table"] and torch.equal(only["tok_table"], a["tok_table"]) and torch.equal(only["scale_byte"], a["scale_byte"])
    sc = call_bwd(mot, g, toks, ids, Et, Eb, s, bpt, want_grads=("scale_tok",))
    assert list(sc) == ["scale_tok"] and torch.equal(sc["scale_tok"], a["scale_tok"])


@pytest.mark.parametrize("dt", list(DTYPES))
def test_module_autograd_with_a_callers_scalars(mot, dt):
    """SplitX0FrontEnd forward + backward with a two-element slice of the caller's longer parameter: the gradients of the restatement,
    the scalars' through the slice into that parameter; ids from the attached table give the same bits as ids given."""
    D, Db, bpt, B, T, Vt, seed, case = SHAPES["S3"]
    toks, tab, ids, inp = problem("S3")
    ref = reference("S3")
    m = mot.SplitX0FrontEnd(Vt, gi.BYTE_VOCAB, D, Db, bytes_per_token=bpt, ttb=torch.from_numpy(tab)).to(DEV)
    m.embed_tokens.to(DTYPES[dt]); m.embed_bytes.to(DTYPES[dt])
    with torch.no_grad():
        m.embed_tokens.weight.copy_(dev(inp["tok_table"], DTYPES[dt]))
        m.embed_bytes.weight.copy_(dev(inp["byte_table"], DTYPES[dt]))
    long = torch.nn.Parameter(dev(np.array([1.25, 2.5, sx.S_BYTE, sx.S_TOK], dtype=np.float32)))
    x, x0t, x0b = m(dev(toks), dev(ids), scalars=long[-2:])
    check_forward({"x0t": x0t, "x0b": x0b, "x": x}, ref, dt, f"S3 module {dt}")
    g = {w: dev(a, DTYPES[dt]) for w, a in inp["g"].items()}
    torch.autograd.backward([x0t, x0b, x], [g["x0t"], g["x0b"], g["x"]])
    mot.check_status()
    assert m.scalars.grad is None and m.embed_tokens.weight.grad.dtype == DTYPES[dt] and m.embed_bytes.weight.grad.dtype == DTYPES[dt]
    check_table(m.embed_tokens.weight.grad, ref["f64"]["d_tok"], dt == "bf16", f"S3 module {dt} embed_tokens.weight.grad")
    check_table(m.embed_bytes.weight.grad, ref["f64"]["d_byte"], dt == "bf16", f"S3 module {dt} embed_bytes.weight.grad")
    assert long.grad[0] == 0 and long.grad[1] == 0
    check_scalars({"scale_tok": long.grad[3], "scale_byte": long.grad[2]}, ref, inp, f"S3 module {dt}")
    with torch.no_grad():
        y, y0t, y0b = m(dev(toks))                     # its own scalars (0.5, 0.5) and ids from the attached table
        z, z0t, z0b = m(dev(toks), dev(ids))
    assert torch.equal(y, z) and torch.equal(y0t, x0t) and torch.equal(y0b, x0b) and torch.equal(z0t, x0t)
    # an output nothing depends on: its gradient arrives as None and goes to the library as NULL
    m.zero_grad()
    x, x0t, x0b = m(dev(toks), dev(ids))
    x0t.backward(g["x0t"])
    r = sx.run(toks, ids, dict(inp, g=dict(inp["g"], x0b=None, x=None)), bpt=bpt, eps=sx.F32_EPS, s_tok=0.5, s_byte=0.5)
    check_table(m.embed_tokens.weight.grad, r["d_tok"], dt == "bf16", f"S3 module {dt} x0t alone")
    assert not m.embed_bytes.weight.grad.any() and not m.scalars.grad.any()


def test_x_agrees_with_the_sum_front_end(mot):
    """On tensors built here: x of the new call against SumFrontEnd(variant="71081"), to the fp32 forward bar."""
    D, Db, bpt, B, T, Vt, seed, case = SHAPES["S3"]
    toks, tab, ids, inp = problem("S3")
    old = mot.modules.SumFrontEnd(Vt, gi.BYTE_VOCAB, D, Db, bytes_per_token=bpt, variant="71081").to(DEV)
    new = mot.SplitX0FrontEnd(Vt, gi.BYTE_VOCAB, D, Db, bytes_per_token=bpt).to(DEV)
    with torch.no_grad():
        for m in (old, new):
            m.embed_tokens.weight.copy_(dev(inp["tok_table"], torch.float32))
            m.embed_bytes.weight.copy_(dev(inp["byte_table"], torch.float32))
            m.scalars.copy_(dev(np.array([sx.S_BYTE, sx.S_TOK], dtype=np.float32)))
        x_old = old(dev(toks), dev(ids))
        x_new, _, _ = new(dev(toks), dev(ids))
    assert_close(host(x_new), host(x_old).astype(np.float64))
    assert_close(host(x_new), reference("S3")["f64"]["x"])


@pytest.mark.parametrize("dt", list(DTYPES))
def test_forward_and_backward_replay_from_a_hip_graph(mot, dt):
    """No memset or memcpy node, no allocation by the library, no sync: capture forward + backward, change the batch in place,
    replay, compare with the uncaptured calls."""
    D, Db, bpt, B, T, Vt, seed, case = SHAPES["S3"]
    toks, tab, ids, Et, Eb, s, g = params("S3", DTYPES[dt])
    toks, ids, s, g = toks.clone(), ids.clone(), s.clone(), {w: a.clone() for w, a in g.items()}
    held = {}

    def step():
        held["outs"] = call_fwd(mot, toks, tab, ids, Et, Eb, s, bpt, "given")
        held["res"] = call_bwd(mot, g, toks, ids, Et, Eb, s, bpt)

    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        step()                                      # warm-up on the capture stream: allocates the workspaces
    torch.cuda.current_stream().wait_stream(st)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):
        step()
    rs = np.random.RandomState(8250)
    toks.copy_(dev(rs.randint(0, Vt, (B, T)).astype(np.int32)))
    ids.copy_(dev(rs.randint(0, gi.BYTE_VOCAB, (B, T * bpt)).astype(np.int64)))
    s.copy_(dev(np.array([0.0, 0.4, -1.1], dtype=np.float32)))   # the scalars are read on the device at every replay
    for a in g.values():
        a.copy_(dev(sx.bf16_values(rs.standard_normal((B, T, D))), DTYPES[dt]))
    graph.replay()
    torch.cuda.synchronize()
    outs = call_fwd(mot, toks, tab, ids, Et, Eb, s, bpt, "given")
    ref = call_bwd(mot, g, toks, ids, Et, Eb, s, bpt)
    mot.check_status()
    for w in sx.OUTS:
        assert torch.equal(outs[w], held["outs"][w]), w
    for k in ("tok_table", "scale_tok", "scale_byte"):
        assert torch.equal(ref[k], held["res"][k]), k
    assert float((ref["byte_table"] - held["res"]["byte_table"]).abs().max()) <= 2 * TOL * float(ref["byte_table"].abs().max())
    assert float(ref["scale_tok"]) != 0.0 and float(ref["byte_table"].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ the index phase's other routes
INDEX = {   # name: (D, byte_dim, bpt, B, T, token vocab, seed, pull, table element)
    "I1": (128, 8, 16, 3, 150, 120, 8301, "right", np.int16),
    "I2": (128, 8, 16, 3, 150, 120, 8302, None, np.int16),
    "I3": (128, 8, 16, 3, 150, 120, 8303, "left", np.int32),
    "I4": (128, 8, 16, 3, 150, 120, 8304, "right", np.int32),
    "I5": (128, 8, 16, 3, 150, 120, 8305, None, np.int32),
    "I6": (512, 8, 64, 2, 150, 120, 8306, "left", np.int16),     # 4 waves x (16 x 65 x 4 + 4225 x 2) B = 50 440 B of LDS: above the 48 KB opt-in
    "I7": (512, 8, 64, 2, 150, 120, 8307, "right", np.int32),    # 84 240 B
}


@functools.lru_cache(maxsize=None)
def index_problem(name):
    D, Db, bpt, B, T, Vt, seed, pull, elem = INDEX[name]
    rs = np.random.RandomState(seed)
    toks = rs.randint(0, Vt - 1, size=(B, T)).astype(np.int32)
    toks[rs.random_sample((B, T)) < 0.1] = 0
    toks[rs.random_sample((B, T)) < 0.03] = Vt - 1
    toks[0, 0] = toks[0, T // 2] = toks[B - 1, 3] = toks[B - 1, 4] = toks[1, T - 1] = Vt - 1
    tab = gi.synth_ttb(seed + 1, Vt, bpt, "right" if pull == "right" else "left", mean_valid=4.4 if bpt == 16 else 9.0).astype(elem)
    padded = orc.tokens_to_bytes(toks, tab.astype(np.float32))
    pulled = {"left": orc.pull_from_left, "right": orc.pull_from_right}[pull](padded, bpt, gi.PAD, gi.EOT) if pull else padded
    return toks, tab, padded.astype(np.int64), pulled.astype(np.int64), sx.make_inputs(seed, Vt, D, Db, B, T)


@functools.lru_cache(maxsize=None)
def index_reference(name):
    D, Db, bpt, B, T, Vt, seed, pull, elem = INDEX[name]
    toks, tab, padded, pulled, inp = index_problem(name)
    return {k: sx.run(toks, pulled, inp, bpt=bpt, dtype=dt, eps=sx.F32_EPS) for k, dt in (("f64", torch.float64), ("fp32", torch.float32), ("bf16", torch.bfloat16))}


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", list(INDEX))
def test_ids_made_in_the_kernel_every_direction_and_table_element(mot, name, dt):
    """pull right, no pull, int32 tables and bpt 64 (the dynamic-LDS opt-in above 48 KB): the outputs have the bits of ids given, the
    ids the kernel writes are the oracle's, the counters count what the oracle's ids hold, and the forward meets its bars."""
    D, Db, bpt, B, T, Vt, seed, pull, elem = INDEX[name]
    toks, tab, padded, pulled, inp = index_problem(name)
    assert pull is None or (pulled != padded).any()
    Et, Eb = dev(inp["tok_table"], DTYPES[dt]), dev(inp["byte_table"], DTYPES[dt])
    s = dev(np.array([1.25, sx.S_BYTE, sx.S_TOK], dtype=np.float32))
    given = dict(zip(sx.OUTS, mot.split_x0(dev(toks), Et, Eb, s[2:3], s[1:2], bpt=bpt, ids=dev(pulled))))
    cnt = torch.zeros(4, dtype=torch.int64, device=DEV)
    outs, ids_padded, ids_pulled = mot.functional._split_x0_fwd(dev(toks), Et, Eb, s[2:3], s[1:2], bpt=bpt, ttb=dev(tab), pull=pull, return_ids=True,
                                                                counters=cnt)
    mot.check_status()
    for w in sx.OUTS:
        assert torch.equal(outs[w], given[w]), (name, w)
    np.testing.assert_array_equal(host(ids_padded), padded)
    np.testing.assert_array_equal(host(ids_pulled), pulled)
    assert cnt.tolist() == [B * T, B * T * bpt, int((padded == gi.PAD).sum()), int((pulled == gi.PAD).sum())]
    check_forward(outs, index_reference(name), dt, f"{name} {dt}")


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", ["I1", "I2", "I3", "I6"])
def test_autograd_with_ids_made_in_the_kernel(mot, name, dt):
    """Forward + backward through the autograd node with ids from the token->byte table: the kernel writes the ids it used and the
    backward reads them.  Against the node with ids given: the same bits (the byte table's gradient inside twice its bar), and the
    float64 restatement's gradients."""
    D, Db, bpt, B, T, Vt, seed, pull, elem = INDEX[name]
    toks, tab, padded, pulled, inp = index_problem(name)
    ref = index_reference(name)
    g = [dev(inp["g"][w], DTYPES[dt]) for w in sx.OUTS]
    grads = []
    for kw in (dict(ttb=dev(tab), pull=pull), dict(ids=dev(pulled))):
        Et, Eb = (torch.nn.Parameter(dev(inp[k], DTYPES[dt])) for k in ("tok_table", "byte_table"))
        s = torch.nn.Parameter(dev(np.array([1.25, sx.S_BYTE, sx.S_TOK], dtype=np.float32)))
        outs = mot.split_x0(dev(toks), Et, Eb, s[2:3], s[1:2], bpt=bpt, **kw)
        torch.autograd.backward(list(outs), g)
        grads.append((Et.grad, Eb.grad, s.grad, outs))
    mot.check_status()
    (ta, ba, sa, oa), (tb, bb, sb, ob) = grads
    assert all(torch.equal(p, q) for p, q in zip(oa, ob)) and torch.equal(ta, tb) and torch.equal(sa, sb) and float(sa[0]) == 0.0
    assert float((ba.float() - bb.float()).abs().max()) <= float(table_bar(ref["f64"]["d_byte"], dt == "bf16").min()) * 2
    check_table(ta, ref["f64"]["d_tok"], dt == "bf16", f"{name} {dt} d_tok, ids from the table")
    check_table(ba, ref["f64"]["d_byte"], dt == "bf16", f"{name} {dt} d_byte, ids from the table")
    check_scalars({"scale_tok": sa[2], "scale_byte": sa[1]}, ref, inp, f"{name} {dt} ids from the table")


@pytest.mark.parametrize("dt", list(DTYPES))
def test_module_with_its_attached_table_under_autograd(mot, dt):
    """What INTEGRATION.md shows: SplitX0FrontEnd(..., ttb=table), front(token_inputs), loss.backward()."""
    D, Db, bpt, B, T, Vt, seed, case = SHAPES["S3"]
    toks, tab, ids, inp = problem("S3")
    ref = reference("S3")
    m = mot.SplitX0FrontEnd(Vt, gi.BYTE_VOCAB, D, Db, bytes_per_token=bpt, ttb=torch.from_numpy(tab)).to(DEV)
    m.embed_tokens.to(DTYPES[dt]); m.embed_bytes.to(DTYPES[dt])
    with torch.no_grad():
        m.embed_tokens.weight.copy_(dev(inp["tok_table"], DTYPES[dt]))
        m.embed_bytes.weight.copy_(dev(inp["byte_table"], DTYPES[dt]))
        m.scalars.copy_(dev(np.array([sx.S_BYTE, sx.S_TOK], dtype=np.float32)))
    x, x0t, x0b = m(dev(toks))
    torch.autograd.backward([x0t, x0b, x], [dev(inp["g"][w], DTYPES[dt]) for w in sx.OUTS])
    mot.check_status()
    check_forward({"x0t": x0t, "x0b": x0b, "x": x}, ref, dt, f"S3 module with its table {dt}")
    check_table(m.embed_tokens.weight.grad, ref["f64"]["d_tok"], dt == "bf16", f"S3 module with its table {dt} embed_tokens.weight.grad")
    check_table(m.embed_bytes.weight.grad, ref["f64"]["d_byte"], dt == "bf16", f"S3 module with its table {dt} embed_bytes.weight.grad")
    check_scalars({"scale_tok": m.scalars.grad[1], "scale_byte": m.scalars.grad[0]}, ref, inp, f"S3 module with its table {dt}")
