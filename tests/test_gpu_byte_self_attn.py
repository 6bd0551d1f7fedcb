"""Byte self-attention in HIP (functional.byte_self_attn / ByteSelfAttn / ByteMixinConcat(use_byte_self_attn=True), csrc/mot_bsa.hip)
against float64: the reference's own fixture cases, production shapes and odd sizes against the restatement of
tests/byte_self_attn_ref.py in float64 on the device, a run-1.3 model front, determinism, hipGraph capture, gradient accumulation.

The bar of every quantity is TWICE the error of the same computation in float32 by the reference (fixture cases: the reference's own
float32 CPU run, recorded in the fixture; other shapes: the restatement in float32 on the device) against float64 -- the "2 x
CPU-fp32" bar of test_gpu_products.py.  d lambdas[0] is a single sum whose float32 reference error can be small by luck, so its
bar is twice the LARGEST relative float32 reference error of d lambdas over all fixture cases.  Every figure is printed.

Measured on an MI355X (largest over the five fixture cases, as a fraction of the largest float64 element; in brackets the bar):
see DESIGN.md, "Byte self-attention", which holds the table this run printed."""
import pytest
import torch
import torch.nn.functional as F

import byte_self_attn_ref as br
import golden_inputs as gi
from mixture_of_tokenizers_amd import functional as fn
from mixture_of_tokenizers_amd import modules as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GOLDEN = br.load_golden()
DLAMBDA_F32ERR = max(float(GOLDEN[br.case_key(name, "f32err", "dlambdas")]) for name in br.CASES)


def fused(x, w, pw, lam, g, *, bpt, window, block_causal):
    leaf = lambda t: t.detach().to(DEV).clone().requires_grad_(True)
    xl, wl, pl, ll = leaf(x), leaf(w), leaf(pw), leaf(lam)
    cos, sin = (t.to(DEV) for t in br.rotary_tables(x.shape[1]))
    out = fn.byte_self_attn(xl, wl, pl, ll, cos, sin, bpt=bpt, window=window, block_causal=block_causal)
    out.backward(g.to(DEV))
    f = lambda a: a.detach().double()
    return {"out": f(out), "attn": f(out) - f(xl), "dx": f(xl.grad), "dqkv_w": f(wl.grad), "dproj_w": f(pl.grad), "dlambdas": f(ll.grad),
            "raw": (out.detach(), xl.grad, wl.grad, pl.grad, ll.grad)}


def check(label, got, ref, own, quantities=br.QUANTITIES):
    """own[what]: the float32 reference's error; asserts err <= 2 * own after printing every figure."""
    rows, bad = [], []
    for what in quantities:
        assert got[what].shape == ref[what].shape and torch.isfinite(got[what]).all(), what
        err = br.rel_err(got[what].cpu(), ref[what].cpu())
        bar = 2 * (DLAMBDA_F32ERR if what == "dlambdas" else own[what])
        rows.append(f"{label:28s} {what:12s} err {err:.3e}  bar {bar:.3e}  ({err / bar:.2f} of it)")
        if not err <= bar:
            bad.append(rows[-1])
    print("\n" + "\n".join(rows))
    assert not bad, "\n".join(bad)


def own_errors(r32, r64, quantities=br.QUANTITIES):
    return {what: br.rel_err(r32[what].cpu(), r64[what].cpu()) for what in quantities}


@pytest.mark.parametrize("name", list(br.CASES))
def test_fixture_cases(name):
    (x, w, pw, lam, g), kw = br.case_inputs(name)
    ref, f32err = br.golden_case(GOLDEN, name, x)
    got = fused(x, w, pw, lam, g, **kw)
    assert got["dlambdas"][1] == 0 and got["raw"][4].shape == (2,)
    check(name, got, ref, f32err)


@pytest.mark.parametrize("D, block_causal", [(48, False), (48, True), (768, False)])
def test_production_shapes(D, block_causal):
    B, T, bpt, swt = 8, 1024, 16, 8
    inputs = br.make_inputs(300 + D + block_causal, D, B, T * bpt)
    kw = dict(bpt=bpt, window=swt * bpt, block_causal=block_causal)
    got = fused(*inputs, **kw)
    r64 = br.run(*inputs, dtype=torch.float64, device=DEV, **kw)
    r32 = br.run(*inputs, dtype=torch.float32, device=DEV, **kw)
    check(f"B8 T1024 D{D} bc{int(block_causal)}", got, r64, own_errors(r32, r64))


@pytest.mark.parametrize("D, B, T, bpt, swt, block_causal", [
    (48, 3, 37, 4, 5, False),     # L = 148: not a multiple of the 128-query tile nor of the 32-key chunk
    (48, 3, 37, 4, 5, True),
    (48, 1, 1, 16, 8, False),     # one token; the window (128) is longer than the row (16)
    (48, 1, 1, 16, 8, True),
    (64, 2, 13, 20, 4, True),     # bpt = 20: token boundaries fall inside tiles and chunks, the look-ahead crosses them
    (48, 2, 23, 18, 3, True),
    (128, 2, 40, 16, 16, False),  # the longest window, 256 bytes
    (256, 1, 9, 16, 16, True),    # window > L with two heads
])
def test_odd_sizes(D, B, T, bpt, swt, block_causal):
    inputs = br.make_inputs(500 + D + T + bpt, D, B, T * bpt)
    kw = dict(bpt=bpt, window=swt * bpt, block_causal=block_causal)
    got = fused(*inputs, **kw)
    r64 = br.run(*inputs, dtype=torch.float64, device=DEV, **kw)
    r32 = br.run(*inputs, dtype=torch.float32, device=DEV, **kw)
    check(f"D{D} B{B} T{T} bpt{bpt} swt{swt} bc{int(block_causal)}", got, r64, own_errors(r32, r64))


# ---- a run-1.3 model front: FlexibleEmbedding + ByteMixin (concat, use_byte_self_attn), model_dim 1024, byte_dim 48, token_dim 256
FRONT = ("x", "d_tok_table", "d_byte_table", "dqkv_w", "dlambdas", "dproj_w", "d_mixin_w")


def front_data(B, T, bpt, vocab=4096, seed=7):
    from mixture_of_tokenizers_amd import loader
    tab = torch.from_numpy(gi.synth_ttb(seed, vocab, bpt, "left")).to(DEV)
    bp = M.ByteHyperparameters(bytes_per_token=bpt, byte_mixin_method="concat", pull_in=True, byte_mixout_method="noop", pull_out=False)
    toks = torch.from_numpy(gi.fineweb_like_tokens(seed, B, T + 1, vocab=vocab, eot_p=0.01)).to(DEV)
    toks_in, padded, pulled, _ = loader.make_create_data_from_toks(bp, tab, tab)(toks)
    assert pulled.shape == (B, T * bpt) and pulled.dtype == torch.int64
    return toks_in, padded, pulled


def front_restated(params, toks, ids, g, dtype, *, bpt, window, block_causal):
    """norm(mixin(cat[norm(E_t[tok]), rearrange(ByteSelfAttn(norm(E_b[ids])))])) in plain torch, forward + backward in `dtype`."""
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    n = lambda t: F.rms_norm(t, (t.size(-1),))
    te, be = n(p["tok"][toks.long()]), n(p["byte"][ids])
    cos, sin = (t.to(device=DEV, dtype=dtype) for t in br.rotary_tables(ids.shape[1]))
    be = br.byte_self_attn(be, p["qkv_w"], p["proj_w"], p["lambdas"], cos, sin, bpt=bpt, window=window, block_causal=block_causal)
    be = be.reshape(be.shape[0], be.shape[1] // bpt, bpt * be.shape[2])
    x = n(F.linear(torch.cat([te, be], dim=-1), p["mixin_w"]))
    x.backward(g.to(dtype))
    f = lambda a: a.detach().double()
    return {"x": f(x), "d_tok_table": f(p["tok"].grad), "d_byte_table": f(p["byte"].grad), "dqkv_w": f(p["qkv_w"].grad),
            "dlambdas": f(p["lambdas"].grad), "dproj_w": f(p["proj_w"].grad), "d_mixin_w": f(p["mixin_w"].grad)}


@pytest.mark.parametrize("within", [False, True])
def test_run_1_3_model_front(within):
    B, T, bpt, swt, vocab = 2, 256, 16, 8, 4096
    torch.manual_seed(11 + within)
    bp = M.ByteHyperparameters(bytes_per_token=bpt, byte_mixin_method="concat", use_byte_self_attn=True, sliding_window_tokens=swt,
                               mix_bytes_within_tok_in=within)
    dims = M.ModelDims(model_dim=1024, byte_dim=48, token_dim=256)
    emb, mixin = M.FlexibleEmbedding(dims, vocab, bp).to(DEV), M.ByteMixin(dims, T, bp).to(DEV)
    attn = mixin.mixin.attention.attention
    with torch.no_grad():
        attn.c_proj.reset_parameters()            # the zero initialisation would hide the branch
        attn.lambdas.copy_(torch.tensor([0.6, 0.4]))
    toks, padded, pulled = front_data(B, T, bpt, vocab)
    g = torch.randn(B, T, 1024, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    x = mixin(*emb(toks, padded, pulled))
    assert x.shape == (B, T, 1024) and x.dtype == torch.float32
    x.backward(g)
    got = {"x": x, "d_tok_table": emb.embed_tokens.weight.grad, "d_byte_table": emb.embed_bytes.weight.grad, "dqkv_w": attn.qkv_w.grad,
           "dlambdas": attn.lambdas.grad, "dproj_w": attn.c_proj.weight.grad, "d_mixin_w": mixin.mixin.mixin.weight.grad}
    assert all(v is not None for v in got.values())
    got = {k: v.detach().double() for k, v in got.items()}
    params = {"tok": emb.embed_tokens.weight, "byte": emb.embed_bytes.weight, "qkv_w": attn.qkv_w, "proj_w": attn.c_proj.weight,
              "lambdas": attn.lambdas, "mixin_w": mixin.mixin.mixin.weight}
    kw = dict(bpt=bpt, window=swt * bpt, block_causal=within)
    r64 = front_restated(params, toks, pulled, g, torch.float64, **kw)
    r32 = front_restated(params, toks, pulled, g, torch.float32, **kw)
    check(f"run 1.3 front within={int(within)}", got, r64, own_errors(r32, r64, FRONT), FRONT)


def test_without_the_switch_the_mixin_takes_its_fused_path():
    B, T, bpt = 2, 64, 16
    bp = M.ByteHyperparameters(bytes_per_token=bpt, byte_mixin_method="concat", pull_in=True)
    dims = M.ModelDims(model_dim=256, byte_dim=48, token_dim=128)
    emb, mixin = M.FlexibleEmbedding(dims, 4096, bp).to(DEV), M.ByteMixin(dims, T, bp).to(DEV)
    toks, padded, pulled = front_data(B, T, bpt)
    h, none = emb(toks, padded, pulled)
    assert isinstance(h, M.EmbedHandle) and none is None
    x = mixin(h, none)
    n = lambda t: F.rms_norm(t, (t.size(-1),))
    te, be = n(emb.embed_tokens.weight[toks.long()]), n(emb.embed_bytes.weight[pulled])
    ref = n(F.linear(torch.cat([te, be.reshape(B, T, bpt * 48)], dim=-1), mixin.mixin.mixin.weight))
    assert br.rel_err(x.detach().cpu(), ref.detach().double().cpu()) < 1e-5


# ---- determinism, hipGraph, accumulation
def test_same_inputs_same_bits():
    """Forward, dx and d lambdas are written once per element / summed in a fixed order: the same bits on every run.  d qkv_w and
    d c_proj.weight are summed over the byte positions with fp32 atomics (launch_gemm_tn): they are held to the bar instead."""
    inputs = br.make_inputs(77, 48, 4, 2048)
    kw = dict(bpt=16, window=128, block_causal=True)
    a, b = fused(*inputs, **kw), fused(*inputs, **kw)
    for i in (0, 1, 4):
        assert torch.equal(a["raw"][i], b["raw"][i]), ("out", "dx", "dqkv_w", "dproj_w", "dlambdas")[i]
    r64 = br.run(*inputs, dtype=torch.float64, device=DEV, **kw)
    r32 = br.run(*inputs, dtype=torch.float32, device=DEV, **kw)
    own = own_errors(r32, r64)
    check("atomically summed, run 1", a, r64, own, ("dqkv_w", "dproj_w"))
    check("atomically summed, run 2", b, r64, own, ("dqkv_w", "dproj_w"))


def test_hipgraph_capture_and_replay():
    kw = dict(bpt=16, window=128, block_causal=False)
    x1, w, pw, lam, g1 = (t.to(DEV) for t in br.make_inputs(81, 48, 2, 1024))
    x2, _, _, _, g2 = (t.to(DEV) for t in br.make_inputs(82, 48, 2, 1024))
    cos, sin = (t.to(DEV) for t in br.rotary_tables(1024))
    xs, gs = x1.clone().requires_grad_(True), g1.clone()
    ws, ps, ls = w.clone().requires_grad_(True), pw.clone().requires_grad_(True), lam.clone().requires_grad_(True)
    leaves = (xs, ws, ps, ls)

    def step():
        out = fn.byte_self_attn(xs, ws, ps, ls, cos, sin, **kw)
        out.backward(gs)
        return out

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            for t in leaves:
                t.grad = None
            step()
    torch.cuda.current_stream().wait_stream(s)
    for t in leaves:
        t.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    with torch.no_grad():
        xs.copy_(x2)
        gs.copy_(g2)
    graph.replay()
    torch.cuda.synchronize()
    ref = fused(x2, w, pw, lam, g2, **kw)["raw"]
    assert torch.equal(out.detach(), ref[0]) and torch.equal(xs.grad, ref[1]) and torch.equal(ls.grad, ref[4])
    assert br.rel_err(ws.grad.cpu(), ref[2].double().cpu()) < 1e-5 and br.rel_err(ps.grad.cpu(), ref[3].double().cpu()) < 1e-5


def test_gradients_accumulate_and_non_contiguous_x():
    (x, w, pw, lam, g), kw = br.case_inputs("d48_block")
    cos, sin = (t.to(DEV) for t in br.rotary_tables(x.shape[1]))
    base = fused(x, w, pw, lam, g, **kw)["raw"]
    xl = x.to(DEV).requires_grad_(True)
    xl.grad = torch.ones_like(xl)
    args = [t.to(DEV).requires_grad_(True) for t in (w, pw, lam)]
    fn.byte_self_attn(xl, *args, cos, sin, **kw).backward(g.to(DEV))
    assert torch.allclose(xl.grad, base[1] + 1, rtol=0, atol=1e-6 * float(base[1].abs().max()) + 1e-7)
    # x as a strided view: copied, same result, gradient in the view's shape
    wide = torch.zeros(x.shape[0], x.shape[1], 2 * x.shape[2], device=DEV)
    wide[..., ::2] = x.to(DEV)
    wide.requires_grad_(True)
    view = wide[..., ::2]
    assert not view.is_contiguous()
    out = fn.byte_self_attn(view, *[t.detach() for t in args], cos, sin, **kw)
    out.backward(g.to(DEV))
    assert torch.equal(out.detach(), base[0]) and torch.equal(wide.grad[..., ::2], base[1]) and not wide.grad[..., 1::2].any()


def test_bf16_is_refused_as_the_follow_up():
    (x, w, pw, lam, g), kw = br.case_inputs("d48_causal")
    cos, sin = (t.to(DEV) for t in br.rotary_tables(x.shape[1]))
    with pytest.raises(NotImplementedError, match="follow-up"):
        fn.byte_self_attn(x.to(DEV).bfloat16(), w.to(DEV), pw.to(DEV), lam.to(DEV), cos, sin, **kw)
