"""-m gpu: the feed-forward of the character mixer's decode step (functional.char_ffn_step / mot_ffn_step) and
CharMixerFrontEnd.step(fused_ffn=True) on top of it.

Reference for values: tests/ffn_step_ref.py, a float64 restatement evaluated on the GPU once per (dim, inter, dtype) for 16 seeded
rows; a case of B rows takes the first B (rows are independent).  Error is max|got - ref| / max|ref|.
  fp32 bar   5e-6 of max|ref|, the bar of this front-end's fp32 rows (tests/test_gpu_swa.py, test_gpu_char_swa_step.py).
  bf16 bar   measured in each case: twice the error of the eager bf16 module (reference_module(torch.bfloat16), on the GPU) against
             the restatement that rounds at the call's bf16 points, for the same bf16-valued inputs (2x: DESIGN section 8).
Inputs: h normal; weights by nn.Linear's default init; the norm weight uniform in [0.8, 1.2]."""
import functools

import pytest
import torch

from ffn_step_ref import ffn_step_ref, reference_module
from util_gpu import DEV, dev

pytestmark = pytest.mark.gpu

BAR = 5e-6
SHAPES = [(256, 512, 1), (256, 512, 3), (256, 512, 16), (264, 1384, 1), (264, 1384, 3), (264, 1384, 16), (2048, 8192, 1), (2048, 8192, 16)]
DTYPES = [torch.float32, torch.bfloat16]


@pytest.fixture(scope="module")
def mot():
    import mixture_of_tokenizers_amd as m
    return m


@functools.lru_cache(maxsize=None)
def case(dim, inter, dtype):
    """The eager module on the GPU, 16 rows of h in `dtype`, and both float64 references of those rows."""
    m = reference_module(dtype, dim=dim, inter=inter, seed=dim + inter, device=DEV)
    h = torch.randn(16, dim, generator=torch.Generator().manual_seed(7 + dim)).to(DEV).to(dtype)
    nw, w1, w2, w3 = m.weights()
    return dict(m=m, h=h, w=(nw, w1, w2, w3), ref=ffn_step_ref(h, nw, w1, w2, w3), ref16=ffn_step_ref(h, nw, w1, w2, w3, round_bf16=True))


def relerr(got, ref, scale=None):
    scale = ref.abs().max() if scale is None else scale
    return float((got.double() - ref).abs().max() / scale)


def fused(mot, h, w, eps=1e-5, cache=None):
    nw, w1, w2, w3 = w
    return mot.char_ffn_step(h, nw, w1, w2, w3, norm_eps=eps, cache=cache)


@pytest.mark.parametrize("dim,inter,B", SHAPES)
def test_fp32_rows_vs_float64(mot, dim, inter, B):
    c = case(dim, inter, torch.float32)
    got = fused(mot, c["h"][:B].contiguous(), c["w"])
    mot.check_status()
    assert got.shape == (B, dim) and got.dtype == torch.float32
    ref = c["ref"][:B]
    err, eager = relerr(got, ref), relerr(c["m"](c["h"][:B]), ref)
    print(f"ffn_step fp32 dim={dim} inter={inter} B={B}: fused {err:.3e}, eager module {eager:.3e} of max|ref64|")
    assert torch.isfinite(got).all() and err <= BAR


@pytest.mark.parametrize("dim,inter,B", SHAPES)
def test_bf16_rows_vs_the_rounding_restatement(mot, dim, inter, B):
    c = case(dim, inter, torch.bfloat16)
    hb = c["h"][:B].contiguous()
    got = fused(mot, hb, c["w"], cache={})
    mot.check_status()
    assert got.shape == (B, dim) and got.dtype == torch.bfloat16
    ref = c["ref16"][:B]
    err, eager = relerr(got, ref), relerr(c["m"](hb), ref)
    step = 2.0 ** -8 * torch.maximum(ref.abs(), torch.full_like(ref, 2.0 ** -6))
    share = float(((got.double() - ref).abs() <= step).double().mean())
    print(f"ffn_step bf16 dim={dim} inter={inter} B={B}: fused {err:.3e}, eager module {eager:.3e} (bar {2 * eager:.3e}) of max|ref|; "
          f"{100 * share:.2f} % of the elements within one bf16 step; against the unrounded float64: {relerr(got, c['ref'][:B]):.3e}")
    assert torch.isfinite(got).all() and err <= 2 * eager


def _bits_zero(t):
    return not t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).any()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_zero_row_scaled_rows_and_large_preactivations(mot, dtype):
    dim, inter, B = 256, 512, 3
    c = case(dim, inter, dtype)
    bf = dtype == torch.bfloat16

    def check(what, h, m, on_delta=False):
        """The dtype's bar; on_delta: the error is taken relative to max|ref - h| ((got - h) - (ref - h) = got - ref)."""
        got = fused(mot, h, m.weights())
        mot.check_status()
        ref = ffn_step_ref(h, *m.weights(), round_bf16=bf)
        scale = (ref - h.double()).abs().max() if on_delta else None
        err = relerr(got, ref, scale)
        bar = 2 * relerr(m(h), ref, scale) if bf else BAR
        print(f"ffn_step {what} {dtype}: {err:.3e} (bar {bar:.3e})")
        assert torch.isfinite(got).all() and err <= bar, what
        return got

    # an all-zero row gives an all-zero row, bit for bit
    h = c["h"][:B].clone()
    h[1] = 0
    got = check("zero row", h, c["m"])
    assert _bits_zero(got[1]) and not _bits_zero(got[0])
    # rows scaled by 1e4 and 1e-4: fp32 on out (the residual dominates), bf16 on out - h
    h = c["h"][:B].clone()
    h[0] *= 1e4
    h[1] *= 1e-4
    check("rows x 1e4, x 1e-4", h, c["m"], on_delta=bf)
    # w1 scaled so that the pre-activations reach about +-120
    h = c["h"][:B].contiguous()
    hd = h.double()
    n = (hd / torch.sqrt((hd * hd).mean(-1, keepdim=True) + 1e-5)) * c["w"][0].double()
    m2 = reference_module(dtype, dim=dim, inter=inter, seed=dim + inter, device=DEV)
    w1 = m2.feed_forward.w1.weight
    w1.copy_((w1.double() * (120.0 / float((n @ w1.double().T).abs().max()))).to(dtype))
    pre = n @ w1.double().T
    assert 110 < float(pre.abs().max()) < 130 and float(pre.max()) > 60 and float(pre.min()) < -60, (float(pre.min()), float(pre.max()))
    check("pre-activations +-120", h, m2)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("dim,inter", [(256, 512), (264, 1384)])
def test_rows_do_not_depend_on_the_padding_or_on_their_neighbours(mot, dim, inter, dtype):
    c = case(dim, inter, dtype)
    full = fused(mot, c["h"], c["w"])                                        # B 16
    for B in (2, 5, 1, 8):                                                   # R 2 full, 5 in R 8, R 1, R 8 full
        part = fused(mot, c["h"][:B].contiguous(), c["w"])
        assert torch.equal(part, full[:B]), B
    # the padding rows of the staged tile are zeros whatever the memory behind h holds
    buf = torch.full((16, dim), float("nan"), device=DEV, dtype=dtype)
    buf[:5] = c["h"][:5]
    assert torch.equal(fused(mot, buf[:5], c["w"]), full[:5])
    mot.check_status()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_eager_runs_are_bit_equal_and_a_captured_call_replays(mot, dtype):
    dim, inter, B = 264, 1384, 3
    c = case(dim, inter, dtype)
    cache = {}
    h = c["h"][:B].clone()
    a, b = fused(mot, h, c["w"], cache=cache), fused(mot, h, c["w"], cache=cache)
    assert torch.equal(a, b)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fused(mot, h, c["w"], cache=cache)                                   # warm-up: allocates the workspace of this stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        out = fused(mot, h, c["w"], cache=cache)
    for i in range(5):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, a), i
    h.copy_(c["h"][8:8 + B])                                                 # the graph reads h in place
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, fused(mot, c["h"][8:8 + B].contiguous(), c["w"], cache=cache))
    mot.check_status()


def test_front_end_step_with_the_fused_feed_forward(mot):
    """The loop of test_decode_loop_reads_nothing_on_the_host (dim 256, inter 512, vocabulary 768, B 2, 10 steps) with
    step(fused_ffn=True), recorded under torch.cuda.graph and replayed: it agrees with front(ids, char_ids) over the produced
    sequence (rtol = atol = 1e-5).  step(fused_ffn=False) in the same process still returns the torch line on char_swa_step's h,
    bit for bit."""
    import numpy as np
    from mixture_of_tokenizers_amd import modules as M
    V, VC, B, P, N = 768, 132, 2, 5, 10
    args = M.ModelArgs(version="two_residual", n_heads=4, dim=256, intermediate_dim=512, head_dim=64, norm_eps=1e-5)
    torch.manual_seed(17)
    fe = M.CharMixerFrontEnd(V, VC, args).to(DEV)
    head = M.PlainLMHead(torch.nn.Linear(256, V, bias=False).to(DEV), norm_in=True)
    blk, ta = fe.char_token_mixer, fe.char_token_mixer.tok_attention
    with torch.no_grad():
        blk.lambda_tok.fill_(0.9); blk.lambda_char.fill_(0.4)
        blk.attention_norm.weight.uniform_(0.8, 1.2); blk.char_norm.weight.uniform_(0.8, 1.2); blk.ffn_norm.weight.uniform_(0.8, 1.2)
    rs = np.random.RandomState(18)
    fe.set_token_chars(torch.from_numpy(rs.randint(0, VC, (V, 8)).astype(np.int32)))
    ids = dev(rs.randint(0, V, (B, P)).astype(np.int64))
    cids = fe.token_chars[ids].long()

    def loop(state, first):
        toks, rows, tok = [], [], first
        for _ in range(N):
            toks.append(tok)
            mixed = fe.step(state, tok, fused_ffn=True)
            rows.append(mixed)
            tok = head.next_token(mixed, greedy=True).token
        return torch.stack(toks, 1), torch.cat(rows, 1)

    with torch.no_grad():
        first = head.next_token(fe(ids, cids), greedy=True).token.clone()       # the prefill: fills the mixer's key / value tables
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            loop(fe.decode_state(ids, cids), first)                             # warm-up: workspaces
        torch.cuda.current_stream().wait_stream(s)
        state = fe.decode_state(ids, cids)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            toks, rows = loop(state, first)
        graph.replay()
        torch.cuda.synchronize()
        mot.check_status()
        assert state.pos.tolist() == [P + N] * B and rows.shape == (B, N, 256)
        full_ids = torch.cat([ids, toks], 1)
        full = fe(full_ids, fe.token_chars[full_ids].long())
        assert torch.allclose(rows, full[:, P:], rtol=1e-5, atol=1e-5), float((rows - full[:, P:]).abs().max())
        # the default path: the torch line on the step's h, as before
        sa, sb = fe.decode_state(ids, cids), fe.decode_state(ids, cids)
        for i in range(3):
            tok = toks[:, i].contiguous()
            plain = fe.step(sa, tok)
            h = mot.char_swa_step(tok, sb, fe.embed_tokens.weight, fe.char_embeddings.weight, tok_chars=fe.token_chars,
                                  attn_norm_w=blk.attention_norm.weight, char_norm_w=blk.char_norm.weight, wq=ta.wq.weight, wk=ta.wk.weight,
                                  wv=ta.wv.weight, wo=ta.wo.weight, n_heads=ta.n_heads, head_dim=ta.head_dim, window=ta.window_size,
                                  norm_eps=blk.attention_norm.eps, version=blk.version, lambda_tok=blk.lambda_tok, lambda_char=blk.lambda_char,
                                  kv_cache=blk._kv_cache)
            assert plain.shape == (B, 1, 256) and torch.equal(plain[:, 0], h + blk.feed_forward(blk.ffn_norm(h)))
            assert torch.allclose(blk.ffn_step(h), plain[:, 0], rtol=1e-5, atol=1e-5)
        mot.check_status()


def test_refusals_reached_from_python(mot):
    c = case(256, 512, torch.float32)
    nw, w1, w2, w3 = c["w"]
    with pytest.raises(NotImplementedError, match="FeedForward"):
        mot.char_ffn_step(torch.zeros(17, 256, device=DEV), nw, w1, w2, w3, norm_eps=1e-5)
    with pytest.raises(TypeError):
        mot.char_ffn_step(c["h"][:2].contiguous(), nw, w1.bfloat16(), w2, w3, norm_eps=1e-5)
    with pytest.raises(TypeError):
        mot.char_ffn_step(c["h"][:2].bfloat16(), nw, w1, w2, w3, norm_eps=1e-5)
    with pytest.raises(TypeError):
        mot.char_ffn_step(c["h"][:2].double(), nw, w1, w2, w3, norm_eps=1e-5)
    with pytest.raises(ValueError):
        mot.char_ffn_step(c["h"][:2].contiguous(), nw, w1, w2.T, w3, norm_eps=1e-5)
    with pytest.raises(RuntimeError, match="HIP device only"):
        mot.char_ffn_step(c["h"][:2].cpu(), nw, w1, w2, w3, norm_eps=1e-5)
    mot.check_status()
