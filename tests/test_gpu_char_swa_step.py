"""-m gpu: one decode step of the Llama character mixer (functional.char_swa_step / mot_char_swa_step) with its device-side state,
and CharMixerFrontEnd.step on top of it.

Reference for values: oracle.char_swa (float64) over the FULL sequence, as in tests/test_gpu_swa.py (parity unpinned by the
reference, see there); the step's row at position t is held to the oracle's row t at that file's bar, 5e-6 of max|ref64|.  The
inputs are the case() recipe of that file (tests/char_swa_step_ref.py holds the copy) with one change: the character ids of a
token are a function of the token, cid = table[token], so that the same data runs through both id sources of the call (the
token -> character table and the caller's ids).  One sequence set per geometry (16 rows x 60 tokens; 8 rows at config-5 dims) and
one oracle evaluation per (geometry, version) serve every (prompt, steps, rows) case: a row depends on its own prefix only."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from char_swa_step_ref import case
from util_gpu import DEV, dev, host

pytestmark = pytest.mark.gpu

VT, VC, TMAX = 700, 132, 60
LT, LC = 0.8, 1.3
BAR = 5e-6
VERSIONS = ("two_residual", "one_residual", "no_residual")


@pytest.fixture(scope="module")
def mot():
    import mixture_of_tokenizers_amd as m
    return m


@functools.lru_cache(maxsize=None)
def inputs(d, H, hd, c_v):
    """numpy inputs of one geometry: case() + the token -> character table `tc` that defines cid."""
    B = 8 if d == 2048 else 16
    c = case(1000 + d + hd + c_v, B, TMAX, c_v, d, H, hd, VT, VC)
    c["tc"] = np.random.RandomState(7 + d + c_v).randint(0, VC, (VT, c_v)).astype(np.int32)
    c["cid"] = c["tc"][c["toks"]].astype(np.int64)
    return c


@functools.lru_cache(maxsize=None)
def on_gpu(d, H, hd, c_v):
    g = {k: dev(v) for k, v in inputs(d, H, hd, c_v).items()}
    g["toks64"] = g["toks"].long()
    g["lt"], g["lc"] = torch.tensor([LT], device=DEV), torch.tensor([LC], device=DEV)
    return g


@functools.lru_cache(maxsize=None)
def reference(d, H, hd, c_v, window, version):
    """oracle.char_swa over the whole sequence set, one batch row at a time (rows are independent; the oracle unfolds the keys)."""
    c = inputs(d, H, hd, c_v)
    rows = [orc.char_swa(c["toks"][b:b + 1], c["cid"][b:b + 1], c["Et"], c["Ec"], c["wa"], c["wc"], c["wq"], c["wk"], c["wv"], c["wo"], n_heads=H,
                         head_dim=hd, window=window, norm_eps=1e-5, version=version, lambda_tok=LT, lambda_char=LC)[0] for b in range(c["toks"].shape[0])]
    return np.stack(rows)


def params(g, H, hd, window, version):
    two = version == "two_residual"
    return dict(attn_norm_w=g["wa"], char_norm_w=g["wc"], wq=g["wq"], wk=g["wk"], wv=g["wv"], wo=g["wo"], n_heads=H, head_dim=hd, window=window,
                norm_eps=1e-5, version=version, lambda_tok=g["lt"] if two else None, lambda_char=g["lc"] if two else None)


def prefill(mot, g, kw, B, P, cache):
    """char_swa over the first P tokens with `cache` (the call that builds the key / value tables; an empty prompt still needs them,
    so one token is run then), and the state after the prompt."""
    n = max(P, 1)
    x = mot.functional.char_swa(g["toks"][:B, :n].contiguous(), g["cid"][:B, :n].contiguous(), g["Et"], g["Ec"], kv_cache=cache, **kw)
    c_v = g["cid"].shape[2]
    if P == 0:
        return x, mot.char_swa_state(None, n_rows=B, window=kw["window"], c_v=c_v, device=DEV)
    return x, mot.char_swa_state(g["cid"][:B, :P], window=kw["window"], c_v=c_v)


def run_steps(mot, g, kw, state, cache, B, P, N, source="table"):
    rows = []
    for i in range(N):
        src = dict(tok_chars=g["tc"]) if source == "table" else dict(char_ids_new=g["cid"][:B, P + i].contiguous())
        rows.append(mot.char_swa_step(g["toks64"][:B, P + i].contiguous(), state, g["Et"], g["Ec"], kv_cache=cache, **src, **kw))
    return torch.stack(rows, 1)


GEOMETRIES = [(256, 4, 64, 1), (256, 4, 64, 3), (256, 4, 64, 16), (512, 4, 128, 1), (512, 4, 128, 3), (512, 4, 128, 16),
              (2048, 32, 64, 1), (2048, 32, 64, 8)]


@pytest.mark.parametrize("version", VERSIONS)
@pytest.mark.parametrize("c_v,window", [(8, 8), (5, 6)])
@pytest.mark.parametrize("d,H,hd,B", GEOMETRIES)
@pytest.mark.parametrize("P,N", [(0, 12), (3, 10), (7, 3), (40, 20)])   # an empty state; padding keys and the ring's wrap; t = 7 fills the window of 8 exactly; deep in a row
def test_step_rows_vs_oracle(mot, P, N, d, H, hd, B, c_v, window, version):
    g, ref = on_gpu(d, H, hd, c_v), reference(d, H, hd, c_v, window, version)[:B, :P + N]
    kw, cache = params(g, H, hd, window, version), {}
    x, state = prefill(mot, g, kw, B, P, cache)
    got = run_steps(mot, g, kw, state, cache, B, P, N)
    mot.check_status()
    assert got.shape == (B, N, d) and got.dtype == torch.float32
    scale = np.abs(ref).max()
    err = np.abs(host(got).astype(np.float64) - ref[:, P:]).max()
    print(f"step fp32 P={P} N={N} B={B} dim={d} {H}x{hd} c_v={c_v} window={window} {version}: max err {err / scale:.3e} of max|ref|")
    assert err <= BAR * scale, f"max abs err {err:.3e} vs max|ref| {scale:.3e}"
    if P:   # the prefill itself, for scale: the same bar
        assert np.abs(host(x).astype(np.float64) - ref[:, :P]).max() <= BAR * scale
    # the state after the loop is the state of the whole character matrix as a prompt
    want = mot.char_swa_state(g["cid"][:B, :P + N], window=window, c_v=c_v)
    assert torch.equal(state.ring, want.ring) and torch.equal(state.pos, want.pos) and state.pos.tolist() == [P + N] * B


@pytest.mark.parametrize("d,H,hd,c_v,window", [(256, 4, 64, 8, 8), (512, 4, 128, 5, 6)])
def test_rows_at_different_positions(mot, d, H, hd, c_v, window):
    """One call whose rows stand at different positions: row 0 after a prompt of 2 tokens, row 1 after 20."""
    version, N = "two_residual", 10
    g, ref = on_gpu(d, H, hd, c_v), reference(d, H, hd, c_v, window, version)
    kw, cache = params(g, H, hd, window, version), {}
    prefill(mot, g, kw, 2, 20, cache)
    s0, s1 = mot.char_swa_state(g["cid"][0:1, :2], window=window, c_v=c_v), mot.char_swa_state(g["cid"][1:2, :20], window=window, c_v=c_v)
    state = mot.CharSwaState(torch.cat([s0.ring, s1.ring]).contiguous(), torch.cat([s0.pos, s1.pos]).contiguous())
    rows = []
    for i in range(N):
        tok = torch.stack([g["toks64"][0, 2 + i], g["toks64"][1, 20 + i]])
        rows.append(mot.char_swa_step(tok, state, g["Et"], g["Ec"], tok_chars=g["tc"], kv_cache=cache, **kw))
    mot.check_status()
    got = host(torch.stack(rows, 1)).astype(np.float64)
    want = np.stack([ref[0, 2:2 + N], ref[1, 20:20 + N]])
    assert np.abs(got - want).max() <= BAR * np.abs(ref[:2]).max()
    assert state.pos.tolist() == [2 + N, 20 + N]
    assert torch.equal(state.ring[0], mot.char_swa_state(g["cid"][0:1, :2 + N], window=window, c_v=c_v).ring[0])
    assert torch.equal(state.ring[1], mot.char_swa_state(g["cid"][1:2, :20 + N], window=window, c_v=c_v).ring[0])


@pytest.mark.parametrize("d,H,hd,B,c_v,window,version", [(256, 4, 64, 3, 8, 8, "two_residual"), (512, 4, 128, 16, 5, 6, "one_residual"),
                                                         (2048, 32, 64, 8, 8, 8, "two_residual")])
def test_both_id_sources_give_the_same_bits(mot, d, H, hd, B, c_v, window, version):
    g = on_gpu(d, H, hd, c_v)
    kw, cache, P, N = params(g, H, hd, window, version), {}, 3, 10
    _, sa = prefill(mot, g, kw, B, P, cache)
    _, sb = prefill(mot, g, kw, B, P, cache)
    a = run_steps(mot, g, kw, sa, cache, B, P, N, "table")
    b = run_steps(mot, g, kw, sb, cache, B, P, N, "ids")
    mot.check_status()
    assert torch.equal(a, b) and torch.equal(sa.ring, sb.ring) and torch.equal(sa.pos, sb.pos)


def test_step_bf16_tables(mot):
    """bf16 tables and weights, read in place: the dims, inputs and bounds of test_char_swa_bf16_tables (seed 21), a prompt of 40
    tokens through char_swa and 20 steps, B 2.  Every element within that test's `allowed` bound of the oracle that rounds the
    same tensors (round_token_products_bf16) and within its three-step bound of the plain oracle; the share within one bf16 step is
    printed (measured on an MI355X: see DESIGN section 24), not asserted."""
    B, T, P, c_v, d, H, hd, window = 2, 60, 40, 8, 256, 4, 64, 8
    c = case(21, B, T, c_v, d, H, hd, 700, 132)
    c16 = {k: (orc.bf16_round(v) if v.dtype == np.float32 else v) for k, v in c.items()}
    lt, lc = (float(np.asarray(orc.bf16_round(np.float32(v))).reshape(-1)[0]) for v in (0.8, 1.3))
    oracle = lambda version="two_residual", **kw: orc.char_swa(c16["toks"], c16["cid"], c16["Et"], c16["Ec"], c16["wa"], c16["wc"], c16["wq"], c16["wk"],
                                                               c16["wv"], c16["wo"], n_heads=H, head_dim=hd, window=window, norm_eps=1e-5, version=version,
                                                               lambda_tok=lt, lambda_char=lc, **kw)
    b16 = lambda a: dev(a).bfloat16()
    t = {k: (b16(v) if v.dtype == np.float32 else dev(v)) for k, v in c16.items()}
    kw = dict(attn_norm_w=t["wa"], char_norm_w=t["wc"], wq=t["wq"], wk=t["wk"], wv=t["wv"], wo=t["wo"], n_heads=H, head_dim=hd, window=window,
              norm_eps=1e-5, version="two_residual", lambda_tok=torch.tensor([0.8], device=DEV).bfloat16(),
              lambda_char=torch.tensor([1.3], device=DEV).bfloat16())
    cache = {}
    mot.functional.char_swa(t["toks"][:, :P].contiguous(), t["cid"][:, :P].contiguous(), t["Et"], t["Ec"], kv_cache=cache, **kw)
    state = mot.char_swa_state(t["cid"][:, :P], window=window, c_v=c_v)
    rows = [mot.char_swa_step(t["toks"][:, P + i].long(), state, t["Et"], t["Ec"], char_ids_new=t["cid"][:, P + i].contiguous(), kv_cache=cache, **kw)
            for i in range(T - P)]
    mot.check_status()
    x = torch.stack(rows, 1)
    assert x.dtype == torch.bfloat16 and x.shape == (B, T - P, d)
    got = host(x.float()).astype(np.float64)
    emul, plain, attn = oracle(round_token_products_bf16=True), oracle(), oracle("no_residual", round_token_products_bf16=True)
    allowed = 1.5 * 2.0 ** -8 * np.maximum(np.abs(emul), np.sqrt((emul ** 2).mean())) + 2.0 ** -7 * np.abs(attn)
    three = 3 * 2.0 ** -8 * np.maximum(np.abs(plain), np.sqrt((plain ** 2).mean())) + 2.0 ** -7 * np.abs(attn)
    em = np.abs(got - emul[:, P:]) / (2.0 ** -8 * np.maximum(np.abs(emul[:, P:]), 2.0 ** -6))
    print(f"step bf16: {100 * (em <= 1).mean():.2f} % of the elements within one bf16 step of the rounding oracle, {em.max():.2f} steps at most")
    assert (np.abs(got - emul[:, P:]) <= allowed[:, P:]).all(), em.max()
    assert (np.abs(got - plain[:, P:]) <= three[:, P:]).all()
    want = mot.char_swa_state(t["cid"], window=window, c_v=c_v)
    assert torch.equal(state.ring, want.ring) and torch.equal(state.pos, want.pos)


def test_status_token_and_character_ids(mot):
    d, H, hd, c_v, window, B, P = 256, 4, 64, 8, 8, 3, 3
    g = on_gpu(d, H, hd, c_v)
    kw, cache = params(g, H, hd, window, "two_residual"), {}
    _, clean = prefill(mot, g, kw, B, P, cache)
    tok = g["toks64"][:B, P].contiguous()
    good = mot.char_swa_step(tok, clean, g["Et"], g["Ec"], tok_chars=g["tc"], kv_cache=cache, **kw)
    mot.check_status()
    for bad_token in (-1, VT):                       # next_token's "no token" and the first id past the table
        _, st = prefill(mot, g, kw, B, P, cache)
        bad = tok.clone()
        bad[1] = bad_token
        out = mot.char_swa_step(bad, st, g["Et"], g["Ec"], tok_chars=g["tc"], kv_cache=cache, **kw)
        with pytest.raises(IndexError, match="token id"):
            mot.check_status()
        assert torch.equal(out[0], good[0]) and torch.equal(out[2], good[2])         # the other rows: bit for bit
        assert st.pos.tolist() == [P + 1] * B and torch.equal(st.ring[1, P % window], g["tc"][0])   # treated as row 0
    _, st = prefill(mot, g, kw, B, P, cache)
    ids = g["cid"][:B, P].clone()
    ids[2, 4] = VC
    out = mot.char_swa_step(tok, st, g["Et"], g["Ec"], char_ids_new=ids, kv_cache=cache, **kw)
    with pytest.raises(IndexError, match="byte id"):
        mot.check_status()
    assert torch.equal(out[:2], good[:2])
    mot.check_status()                               # the word is clear again


def test_eager_runs_are_bit_equal_and_a_captured_step_replays(mot):
    """Two eager runs of the same 12 steps give the same bits; one step captured into a hipGraph and replayed 12 times, the new
    tokens copied into its static token buffer between the replays, gives those bits and the same final state (the stream discipline
    of test_char_swa_is_capturable_in_a_hip_graph)."""
    d, H, hd, c_v, window, B, P, N = 256, 4, 64, 8, 8, 3, 5, 12
    g = on_gpu(d, H, hd, c_v)
    kw, cache = params(g, H, hd, window, "two_residual"), {}
    _, s1 = prefill(mot, g, kw, B, P, cache)
    _, s2 = prefill(mot, g, kw, B, P, cache)
    a, b = run_steps(mot, g, kw, s1, cache, B, P, N), run_steps(mot, g, kw, s2, cache, B, P, N)
    assert torch.equal(a, b) and torch.equal(s1.ring, s2.ring) and torch.equal(s1.pos, s2.pos)
    _, st = prefill(mot, g, kw, B, P, cache)
    scratch = mot.CharSwaState(st.ring.clone(), st.pos.clone())
    tok = g["toks64"][:B, P].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        mot.char_swa_step(tok, scratch, g["Et"], g["Ec"], tok_chars=g["tc"], kv_cache=cache, **kw)      # warm-up: allocates the workspace
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        out = mot.char_swa_step(tok, st, g["Et"], g["Ec"], tok_chars=g["tc"], kv_cache=cache, **kw)
    assert st.pos.tolist() == [P] * B                # capturing runs nothing
    rows = []
    for i in range(N):
        tok.copy_(g["toks64"][:B, P + i])
        graph.replay()
        rows.append(out.clone())
    torch.cuda.synchronize()
    mot.check_status()
    assert torch.equal(torch.stack(rows, 1), a) and torch.equal(st.ring, s1.ring) and torch.equal(st.pos, s1.pos)


def test_decode_loop_reads_nothing_on_the_host(mot):
    """CharMixerFrontEnd.step -> a stand-in trunk (identity) -> PlainLMHead.next_token(greedy=True), 10 steps at dim 256 with the
    token -> character table.  The whole loop is recorded under torch.cuda.graph capture, which refuses .item(), .tolist() and .cpu():
    that it records at all is the check.  Afterwards front(ids, char_ids) over the produced sequence agrees with the step rows,
    feed_forward included (torch.allclose, rtol = atol = 1e-5).
    The vocabulary is 768, not the 700 of the other tests: next_token takes a multiple of 128 classes."""
    from mixture_of_tokenizers_amd import modules as M
    V, B, P, N = 768, 2, 5, 10
    args = M.ModelArgs(version="two_residual", n_heads=4, dim=256, intermediate_dim=512, head_dim=64, norm_eps=1e-5)
    torch.manual_seed(17)
    fe = M.CharMixerFrontEnd(V, VC, args).to(DEV)
    head = M.PlainLMHead(torch.nn.Linear(256, V, bias=False).to(DEV), norm_in=True)
    blk = fe.char_token_mixer
    with torch.no_grad():
        blk.lambda_tok.fill_(0.9); blk.lambda_char.fill_(0.4)
        blk.attention_norm.weight.uniform_(0.8, 1.2); blk.char_norm.weight.uniform_(0.8, 1.2)
    rs = np.random.RandomState(18)
    tc = torch.from_numpy(rs.randint(0, VC, (V, 8)).astype(np.int32))
    fe.set_token_chars(tc)
    assert "token_chars" not in fe.state_dict() and fe.token_chars.device.type == "cuda"
    ids = dev(rs.randint(0, V, (B, P)).astype(np.int64))
    cids = fe.token_chars[ids].long()

    def loop(state, first):
        toks, rows, tok = [], [], first
        for _ in range(N):
            toks.append(tok)
            mixed = fe.step(state, tok)                       # (B, 1, dim); the trunk would run here
            rows.append(mixed)
            tok = head.next_token(mixed, greedy=True).token
        return torch.stack(toks, 1), torch.cat(rows, 1)

    with torch.no_grad():
        first = head.next_token(fe(ids, cids), greedy=True).token.clone()       # the prefill: fills the mixer's key / value tables
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            loop(fe.decode_state(ids, cids), first)                             # warm-up: workspaces, the dense layers' handles
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
    want = fe.decode_state(full_ids, fe.token_chars[full_ids].long())
    assert torch.equal(state.ring, want.ring)


def test_refusals_reached_from_python(mot):
    d, H, hd, c_v, window = 256, 4, 64, 8, 8
    g = on_gpu(d, H, hd, c_v)
    kw, cache = params(g, H, hd, window, "two_residual"), {}
    tok = g["toks64"][:2, 0].contiguous()
    st = mot.char_swa_state(None, n_rows=2, window=window, c_v=c_v, device=DEV)
    with pytest.raises(RuntimeError, match="char_swa"):                       # no tables yet
        mot.char_swa_step(tok, st, g["Et"], g["Ec"], tok_chars=g["tc"], kv_cache=cache, **kw)
    prefill(mot, g, kw, 2, 1, cache)
    mot.char_swa_step(tok, st, g["Et"], g["Ec"], tok_chars=g["tc"], kv_cache=cache, **kw)
    st17 = mot.char_swa_state(None, n_rows=17, window=window, c_v=c_v, device=DEV)
    with pytest.raises(NotImplementedError, match="char_swa"):
        mot.char_swa_step(torch.zeros(17, dtype=torch.int64, device=DEV), st17, g["Et"], g["Ec"], tok_chars=g["tc"], kv_cache=cache, **kw)
    assert st17.pos.tolist() == [0] * 17
    wk = g["wk"].clone()
    kw2 = dict(kw, wk=wk)
    cache2 = {}
    mot.functional.char_swa(g["toks"][:2, :1].contiguous(), g["cid"][:2, :1].contiguous(), g["Et"], g["Ec"], kv_cache=cache2, **kw2)
    mot.char_swa_step(tok, st, g["Et"], g["Ec"], tok_chars=g["tc"], kv_cache=cache2, **kw2)
    wk.mul_(1.5)                                                              # in place: the tables in cache2 are stale
    with pytest.raises(RuntimeError, match="char_swa"):
        mot.char_swa_step(tok, st, g["Et"], g["Ec"], tok_chars=g["tc"], kv_cache=cache2, **kw2)
    mot.check_status()
