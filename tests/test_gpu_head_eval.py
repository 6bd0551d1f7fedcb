"""The evaluation form of the two output heads (functional.token_head_eval / byte_head_eval, ByteMixout.evaluate; the EVAL row
passes of csrc/mot_tokhead.hip and csrc/mot_head.hip) on the device.

1. Exact integer data: x and W in {-1, 0, 1}, so every stored product is a small integer, exact in fp32 and bf16, and ties are
   frequent; pred, rank and counts must equal their int64 restatement bit for bit.
2. Random data against float64 on the values the kernel sees.  row_loss, as `relerr` measures it (largest error over the largest
   float64 element): fp32 within 2e-6; bf16 err <= 2 * own + 2^-12, `own` being the eager bf16 restatement's error.  pred and rank
   are taken on the stored products s = x_r W^T, in front of the row factor c_r > 0 and the increasing softcap, so they are judged on
   the float64 products s64, whose order is the logits' order.  With
       delta_r = 2 * (K * 2^-24 * ||x_r|| * max_v ||W_v||  +  [stored in bf16] 2^-8 * max_v |s64[r, v]|)
   (an fp32 dot product of length K errs by at most K 2^-24 ||x_r|| ||W_v||; a stored bf16 logit carries one more rounding of
   2^-8 |s|; two logits are compared, hence the factor 2): pred is valid when s64[r, pred] >= max_v s64[r, v] - delta_r, and rank
   must lie between the numbers of classes above s64[r, y] + delta_r and above s64[r, y] - delta_r.  The byte head stores fp32
   logits in both dtypes.  delta_r comes from this rounding model, not from a measurement.
3. HeadEval.loss has the bits of the loss call under no_grad.  4. Targets out of range.  5. Determinism and hipGraph capture.
6. ByteMixout.evaluate.  Every figure is printed before it is asserted (pytest -s shows them)."""
import pytest
import torch
import torch.nn.functional as F

import byte_head_ref as br
import mixture_of_tokenizers_amd as mot
import token_head_ref as tr
from mixture_of_tokenizers_amd import _capi as capi
from mixture_of_tokenizers_amd import functional as fn
from mixture_of_tokenizers_amd.modules import ByteHyperparameters, ByteMixout, CastedLinear, ModelDims

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DTYPES = [torch.float32, torch.bfloat16]
FP32_LOSS = 2e-6
V_REAL, D_REAL, N_REAL = 50304, 768, 40
BV = br.VOCAB


def relerr(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    return float((got - ref).abs().max() / max(ref.abs().max().item(), 1e-300))


def first_argmax(s):
    """The lowest class among a row's largest entries."""
    cls = torch.arange(s.shape[1], device=s.device).expand_as(s)
    return torch.where(s == s.max(1, keepdim=True).values, cls, s.shape[1]).min(1).values


def expected(s, t, per=None):
    """pred, rank and counts of rows with stored logits s [M, V] (exact) and targets t [M]; per: rows per token (byte head)."""
    V = s.shape[1]
    ok = (t >= 0) & (t < V)
    pred = first_argmax(s)
    sy = s.gather(1, t.clamp(0, V - 1)[:, None])
    rank = torch.where(ok, (s > sy).sum(1), -1)
    hit = ok & (pred == t)
    counts = [int(ok.sum()), int(hit.sum())]
    if per:
        counts.append(int(hit.reshape(-1, per).all(1).sum()))
    return pred, rank, counts


def check_exact(what, ev, s, t, per=None):
    pred, rank, counts = expected(s, t, per)
    got = ev.counts.tolist()
    print(f"{what}: counts {got} (expected {counts}), ties for the maximum in {int(((s == s.max(1, keepdim=True).values).sum(1) > 1).sum())} of {s.shape[0]} rows")
    assert ev.pred.dtype == ev.rank.dtype == torch.int32 and ev.counts.dtype == torch.int64 and ev.row_loss.dtype == torch.float32
    assert torch.equal(ev.pred.reshape(-1).long(), pred), what
    assert torch.equal(ev.rank.reshape(-1).long(), rank), what
    assert got == counts, what
    assert torch.isfinite(ev.row_loss).all() and torch.isfinite(ev.loss)


def ternary(shape, g):
    return torch.randint(-1, 2, shape, device=DEV, generator=g).float()


def signs(n, g):
    return torch.randint(0, 2, (n,), device=DEV, generator=g).float() * 2 - 1


# ---- 1. exact integer data
TOKEN_SHAPES = [  # (what, N, D, V by dtype, chunk_rows)
    ("smallest vocabulary", 40, 64, (128, 128), None),
    ("ragged last round of 256 threads", 40, 64, (384, 384), None),
    ("first rows on 1024 threads", 40, 64, (4224, 8320), None),
    ("the real width: 16 / 8 vectors a thread", 8, 16, (50304, 50304), None),
    ("rows read twice", 8, 16, (65664, 65664), None),
    ("three chunks, the last ragged", 70, 64, (384, 384), 32),
]


def token_int_inputs(N, D, V, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x, w = ternary((N, D), g), ternary((V, D), g)
    x[0], x[1] = signs(D, g), signs(D, g)
    w[0], w[V - 1] = x[0], x[1]            # row 0 has its maximum D at the first class, row 1 at the last
    t = torch.randint(0, V, (N,), device=DEV, generator=g)
    t[:6] = torch.tensor([0, V - 1, V - 1, 0, 1, V - 2], device=DEV)
    return x, w, t


@pytest.mark.parametrize("kind", tr.SOFTCAPS)
@pytest.mark.parametrize("norm_in", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("what, N, D, Vs, chunk", TOKEN_SHAPES)
def test_token_head_exact_integers(what, N, D, Vs, chunk, dtype, norm_in, kind):
    V = Vs[DTYPES.index(dtype)]
    x, w, t = token_int_inputs(N, D, V, N + D + V)
    s = (x.double() @ w.double().T).long()   # |s| <= D <= 128: exact in float64, fp32 and bf16
    assert int(s[0, 0]) == D == int(s[0].max()) and int(s[1, V - 1]) == D == int(s[1].max())
    ev = fn.token_head_eval(x.to(dtype), w, t, softcap=kind, norm_in=norm_in, chunk_rows=chunk)
    check_exact(f"{what}, V {V} {dtype} norm {norm_in} {kind}", ev, s, t)
    assert int(ev.pred[0]) == 0 and int(ev.rank[0]) == 0 and int(ev.rank[1]) == 0   # targets 0 and V - 1 at those rows' maxima


BYTE_SHAPES = [  # (what, n_tokens, bpt, model_dim)
    ("37 tokens, bpt 16", 37, 16, 256),
    ("37 tokens, bpt 4", 37, 4, 64),
]
BYTE_CHUNKED = [  # two chunks with a ragged last one: rows x (2048 + 4 K) bytes pass the 48 MiB of a chunk
    ("split, 24 000 rows in chunks of 23 808", "split", 1500, 16, 256),
    ("copy, 21 800 rows in chunks of 21 760", "copy", 21800, 4, 64),
]


def byte_rows(x, method, bpt):
    """The rows the head contracts, one per byte position (copy: the token's row at each of its positions)."""
    return x.repeat_interleave(bpt, 0) if method == "copy" else x.reshape(-1, x.shape[-1] // bpt)


def byte_int_inputs(method, T, bpt, D, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    K = D if method == "copy" else D // bpt
    x, w = ternary((T, D), g), ternary((BV, K), g)
    x[0], x[1] = signs(D, g), signs(D, g)
    w[0], w[BV - 1] = x[0, :K], x[1, :K]   # the first row of token 0 peaks at class 0, of token 1 at class 511
    t = torch.randint(0, 458, (T * bpt,), device=DEV, generator=g)
    t[torch.rand(t.shape, device=DEV, generator=g) < 0.2] = 456                 # pad-heavy, like real targets
    t[:4] = torch.tensor([0, BV - 1, 458, 0], device=DEV)                       # the first class, the last, the padding
    t[bpt:bpt + 2] = torch.tensor([BV - 1, 500], device=DEV)
    return x, w, t


@pytest.mark.parametrize("L", [0, 2])
@pytest.mark.parametrize("method", ["copy", "split"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("what, T, bpt, D", BYTE_SHAPES)
def test_byte_head_exact_integers(what, T, bpt, D, dtype, method, L):
    x, w, t = byte_int_inputs(method, T, bpt, D, T + bpt + D)
    s = (byte_rows(x, method, bpt).double() @ w.double().T).long()   # fp32 logits in both dtypes: exact up to 2^24
    K = w.shape[1]
    assert int(s[0, 0]) == K == int(s[0].max()) and int(s[bpt, BV - 1]) == K == int(s[bpt].max())
    # token 2 is all-correct whatever the data: its targets are its predictions
    t[2 * bpt:3 * bpt] = first_argmax(s[2 * bpt:3 * bpt])
    ev = fn.byte_head_eval(x.to(dtype), w, t, method=method, bytes_per_token=bpt, n_layer_out=L)
    check_exact(f"{what} {method} L {L} {dtype}", ev, s, t, per=bpt)
    assert ev.counts[2] >= 1 and ev.row_loss.shape == t.shape


@pytest.mark.parametrize("what, method, T, bpt, D", BYTE_CHUNKED)
def test_byte_head_exact_integers_across_chunks(what, method, T, bpt, D):
    x, w, t = byte_int_inputs(method, T, bpt, D, T)
    s = (byte_rows(x, method, bpt).double() @ w.double().T).long()
    t[-bpt:] = first_argmax(s[-bpt:])   # the last token, in the ragged chunk, is all-correct
    ev = fn.byte_head_eval(x, w, t, method=method, bytes_per_token=bpt, n_layer_out=1)
    check_exact(what, ev, s, t, per=bpt)
    with torch.no_grad():
        assert torch.equal(ev.loss, fn.byte_head_loss(x, w, t, method=method, bytes_per_token=bpt, n_layer_out=1))


# ---- 2. random data against float64
def delta_rows(rows64, w64, s64, stored_bf16):
    K = rows64.shape[1]
    d = K * 2.0 ** -24 * rows64.norm(dim=1) * w64.norm(dim=1).max()
    if stored_bf16:
        d = d + 2.0 ** -8 * s64.abs().max(1).values
    return 2 * d


def check_float(what, ev, s64, delta, loss64, own, t, per=None):
    """s64 [M, V]: float64 products per row; delta [M]; loss64 [M]: float64 row losses; own: the eager bf16 ones (None in fp32)."""
    M, V = s64.shape
    pred, rank = ev.pred.reshape(-1).long(), ev.rank.reshape(-1).long()
    e = relerr(ev.row_loss.reshape(-1), loss64)
    if own is None:
        print(f"{what}: row_loss {e:.3e} (bar {FP32_LOSS:.0e})")
        assert e < FP32_LOSS, what
    else:
        o = relerr(own, loss64)
        print(f"{what}: row_loss {e:.3e} (eager bf16 {o:.3e})")
        assert e <= 2 * o + 2 ** -12, what
    assert ((pred >= 0) & (pred < V)).all()
    short = s64.max(1).values - s64.gather(1, pred[:, None])[:, 0]
    sy = s64.gather(1, t[:, None])
    lo, hi = (s64 > sy + delta[:, None]).sum(1), (s64 > sy - delta[:, None]).sum(1)
    print(f"{what}: pred short of the maximum by at most {float(short.max()):.3e} (delta >= {float(delta.min()):.3e}); "
          f"rank window widths up to {int((hi - lo).max())}; top-1 {int(ev.counts[1])} of {M}")
    assert (short <= delta).all(), what                 # every row: none is left out
    assert ((lo <= rank) & (rank <= hi)).all(), what
    assert int(ev.counts[0]) == M and int(ev.counts[1]) == int((pred == t).sum()), what
    if per:
        assert int(ev.counts[2]) == int((pred == t).reshape(-1, per).all(1).sum()), what


_real = {}


def real_inputs():
    """x [40, 768] and W [50304, 768] with std(l) = 10, well into the curved part of both caps (real_inputs(10.0) of
    test_gpu_token_head.py), targets with the first class, the last real one and padded ones."""
    if not _real:
        g = torch.Generator(device=DEV).manual_seed(7)
        x = torch.randn(N_REAL, D_REAL, device=DEV, generator=g)
        w = (torch.rand(V_REAL, D_REAL, device=DEV, generator=g) * 2 - 1) * (3 ** 0.5) * 10.0 * D_REAL ** -0.5
        t = torch.randint(0, 50257, (N_REAL,), device=DEV, generator=g)
        t[:8] = torch.tensor([0, 50256, 50303, 50303, 0, 17, 17, 50257], device=DEV)
        t[8:16] = (x[8:16].double() @ w.double().T).argmax(1)   # rows whose target is (in fp32, and likely in bf16) the largest logit
        _real["in"] = (x, w, t)
    return _real["in"]


def real_reference(dtype):
    """float64 products of the values the kernel sees, shared by the two softcaps."""
    if dtype not in _real:
        x, w, _ = real_inputs()
        x64, w64 = x.to(dtype).double(), w.to(dtype).double()
        s64 = x64 @ w64.T
        _real[dtype] = (x64, s64, delta_rows(x64, w64, s64, dtype == torch.bfloat16))
    return _real[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", tr.SOFTCAPS)
def test_token_head_real_width_against_float64(kind, dtype):
    x, w, t = real_inputs()
    x64, s64, delta = real_reference(dtype)
    c = (x64.square().mean(1, keepdim=True) + torch.finfo(torch.float64).eps).rsqrt()   # F.rms_norm's factor per row, in float64
    assert 9 < (c * s64).std().item() < 11
    loss64 = F.cross_entropy(tr.softcap(c * s64, kind), t, reduction="none")
    own = None
    if dtype == torch.bfloat16:   # the eager bf16 path of tests/token_head_ref.py, per row
        xb = x.to(dtype)
        own = F.cross_entropy(tr.softcap(F.linear(F.rms_norm(xb, (D_REAL,)), w.to(dtype)).float(), kind), t, reduction="none")
    ev = fn.token_head_eval(x.to(dtype), w, t, softcap=kind)
    check_float(f"50304 x 768 x 40 {kind} {dtype}", ev, s64, delta, loss64, own, t)
    with torch.no_grad():   # 3. the bits of the loss call
        loss = fn.token_head_loss(x.to(dtype), w, t, softcap=kind)
    assert torch.equal(ev.loss, loss)
    assert abs(float(ev.row_loss.double().sum() / N_REAL) - float(loss)) <= 1e-6 * abs(float(loss))


def byte_float_inputs(method, T, bpt, D, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    K = D if method == "copy" else D // bpt
    x = torch.randn(T, D, device=DEV, generator=g)
    w = (torch.rand(BV, K, device=DEV, generator=g) * 2 - 1) * (3 ** 0.5) * 10.0 * K ** -0.5   # std(l) 10
    t = torch.randint(0, 458, (T * bpt,), device=DEV, generator=g)
    t[:4] = torch.tensor([0, BV - 1, 458, 0], device=DEV)
    t[2 * bpt:4 * bpt] = (byte_rows(x, method, bpt)[2 * bpt:4 * bpt].double() @ w.double().T).argmax(1)   # tokens 2 and 3 (all but) right
    return x, w, t


@pytest.mark.parametrize("L", [0, 2])
@pytest.mark.parametrize("method", ["copy", "split"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("what, T, bpt, D", BYTE_SHAPES)
def test_byte_head_against_float64(what, T, bpt, D, dtype, method, L):
    x, w, t = byte_float_inputs(method, T, bpt, D, T + bpt + D + L)
    x64, w64 = x.to(dtype).double(), w.to(dtype).double()
    rows64 = byte_rows(x64, method, bpt)
    s64 = rows64 @ w64.T
    delta = delta_rows(rows64, w64, s64, False)

    def row_losses(xv, wv):   # tests/byte_head_ref.py's forward, per byte position
        h = br.byte_states(xv, method, bpt, L)
        l = F.linear(F.rms_norm(h, (h.size(-1),)), wv)
        return F.cross_entropy(30 * torch.sigmoid((l if l.dtype == torch.float64 else l.float()) / 7.5), t, reduction="none")

    own = row_losses(x.to(dtype), w.to(dtype)) if dtype == torch.bfloat16 else None
    ev = fn.byte_head_eval(x.to(dtype), w, t, method=method, bytes_per_token=bpt, n_layer_out=L)
    check_float(f"{what} {method} L {L} {dtype}", ev, s64, delta, row_losses(x64, w64), own, t, per=bpt)
    with torch.no_grad():   # 3. the bits of the loss call
        loss = fn.byte_head_loss(x.to(dtype), w, t, method=method, bytes_per_token=bpt, n_layer_out=L)
    assert torch.equal(ev.loss, loss)
    assert abs(float(ev.row_loss.double().sum() / t.numel()) - float(loss)) <= 1e-6 * abs(float(loss))


# ---- 3. the same bits as the loss call, over chunks and on every path of the row pass
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N, D, V, chunk", [(70, 64, 384, 32), (40, 64, 8320, None), (8, 16, 65664, None), (300, 64, 640, None)])
def test_token_head_loss_has_the_bits_of_the_loss_call(N, D, V, chunk, dtype):
    g = torch.Generator(device=DEV).manual_seed(N + V)
    x = torch.randn(N, D, device=DEV, generator=g).to(dtype)
    w = torch.randn(V, D, device=DEV, generator=g) * 1.5
    t = torch.randint(0, V, (N,), device=DEV, generator=g)
    for kind in tr.SOFTCAPS:
        ev = fn.token_head_eval(x, w, t, softcap=kind, chunk_rows=chunk)
        with torch.no_grad():
            loss = fn.token_head_loss(x, w, t, softcap=kind, chunk_rows=chunk)
        mean = float(ev.row_loss.double().sum() / N)
        print(f"N {N} V {V} {kind} {dtype}: loss {float(loss):.7f}, mean of row_loss {mean:.7f}")
        assert torch.equal(ev.loss, loss)
        assert abs(mean - float(loss)) <= 1e-6 * abs(float(loss))


# ---- 4. targets outside [0, vocab)
@pytest.mark.parametrize("dtype", DTYPES)
def test_token_head_out_of_range_targets(dtype):
    x, w, t = (a.to(DEV) for a in tr.case_inputs("rsqrt15", True))
    x = x.to(dtype)
    ok = fn.token_head_eval(x, w, t, softcap="rsqrt15")
    bad = t.clone()
    bad[5], bad[17] = -100, tr.VOCAB
    bad[6] = ok.pred[6]   # a hit next to a dropped row
    mot.check_status()
    ev = fn.token_head_eval(x, w, bad, softcap="rsqrt15")
    assert int(capi.status_word(DEV).item()) & capi.STATUS_TARGET_OOR
    with pytest.raises(IndexError, match="target"):
        mot.check_status()
    assert ev.row_loss[[5, 17]].tolist() == [0.0, 0.0] and ev.rank[[5, 17]].tolist() == [-1, -1]
    assert torch.equal(ev.pred, ok.pred)   # pred is still written
    keep = torch.ones_like(t, dtype=torch.bool)
    keep[[5, 17]] = False
    same_target = keep & (bad == t)
    assert torch.equal(ev.row_loss[same_target], ok.row_loss[same_target]) and torch.equal(ev.rank[same_target], ok.rank[same_target])
    assert int(ev.rank[6]) == 0 and (ev.rank[keep] >= 0).all()
    assert ev.counts.tolist() == [tr.ROWS - 2, int((ev.pred == bad)[keep].sum())] and ev.counts[1] >= 1
    with torch.no_grad():
        assert torch.equal(ev.loss, fn.token_head_loss(x, w, bad, softcap="rsqrt15"))
    with pytest.raises(IndexError, match="target"):
        mot.check_status()


@pytest.mark.parametrize("method", ["copy", "split"])
def test_byte_head_out_of_range_targets(method):
    T, bpt, D = 37, 16, 256
    x, w, t = byte_float_inputs(method, T, bpt, D, 5)
    first = fn.byte_head_eval(x, w, t, method=method, bytes_per_token=bpt)
    t = t.clone()
    t[3 * bpt:5 * bpt] = first.pred[3 * bpt:5 * bpt]   # tokens 3 and 4 are all-correct
    ok = fn.byte_head_eval(x, w, t, method=method, bytes_per_token=bpt)
    bad = t.clone()
    bad[3 * bpt + 2], bad[7 * bpt] = -100, BV         # token 3 loses a target, token 7 too
    mot.check_status()
    ev = fn.byte_head_eval(x, w, bad, method=method, bytes_per_token=bpt)
    assert int(capi.status_word(DEV).item()) & capi.STATUS_TARGET_OOR
    with pytest.raises(IndexError, match="target"):
        mot.check_status()
    at = [3 * bpt + 2, 7 * bpt]
    assert ev.row_loss[at].tolist() == [0.0, 0.0] and ev.rank[at].tolist() == [-1, -1]
    assert torch.equal(ev.pred, ok.pred)
    keep = torch.ones_like(t, dtype=torch.bool)
    keep[at] = False
    assert torch.equal(ev.row_loss[keep], ok.row_loss[keep]) and torch.equal(ev.rank[keep], ok.rank[keep])
    hits = (ev.pred == bad) & keep
    print(f"{method}: counts {ok.counts.tolist()} -> {ev.counts.tolist()}")
    assert ev.counts.tolist() == [T * bpt - 2, int(hits.sum()), int(hits.reshape(T, bpt).all(1).sum())]
    assert int(ok.counts[2]) - int(ev.counts[2]) == 1 and int(ev.counts[2]) >= 1   # token 3 is not all-correct any more, token 4 is
    with torch.no_grad():
        assert torch.equal(ev.loss, fn.byte_head_loss(x, w, bad, method=method, bytes_per_token=bpt))
    with pytest.raises(IndexError, match="target"):
        mot.check_status()


# ---- 5. determinism and hipGraph capture
def same(a, b):
    return all(torch.equal(u, v) for u, v in zip(a, b))


def captured(call, x1, t1, x2, t2):
    """One evaluation captured on (x1, t1), replayed after x.copy_(x2) and targets.copy_(t2); returns (replayed, eager on new data)."""
    xs, ts = x1.clone(), t1.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            call(xs, ts)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ev = call(xs, ts)
    xs.copy_(x2)
    ts.copy_(t2)
    graph.replay()
    torch.cuda.synchronize()
    return ev, call(x2, t2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", tr.SOFTCAPS)
def test_token_head_deterministic_and_capturable(kind, dtype):
    N, D, V = 96, 64, 640
    g = torch.Generator(device=DEV).manual_seed(11)
    x1, x2 = (torch.randn(N, D, device=DEV, generator=g).to(dtype) for _ in range(2))
    w = torch.randn(V, D, device=DEV, generator=g) * 0.5
    t1, t2 = (torch.randint(0, V, (N,), device=DEV, generator=g) for _ in range(2))
    call = lambda x, t: fn.token_head_eval(x, w, t, softcap=kind, chunk_rows=32)
    assert same(call(x1, t1), call(x1, t1))
    replayed, eager = captured(call, x1, t1, x2, t2)
    assert same(replayed, eager) and not torch.equal(eager.pred, call(x1, t1).pred)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", ["copy", "split"])
def test_byte_head_deterministic_and_capturable(method, dtype):
    T, bpt, D = 37, 16, 256
    x1, w, t1 = byte_float_inputs(method, T, bpt, D, 21)
    x2, _, t2 = byte_float_inputs(method, T, bpt, D, 22)
    x1, x2 = x1.to(dtype), x2.to(dtype)
    call = lambda x, t: fn.byte_head_eval(x, w, t, method=method, bytes_per_token=bpt, n_layer_out=1)
    assert same(call(x1, t1), call(x1, t1))
    replayed, eager = captured(call, x1, t1, x2, t2)
    assert same(replayed, eager) and not torch.equal(eager.pred, call(x1, t1).pred)


# ---- 6. the module
@pytest.mark.parametrize("method", ["noop", "copy", "split"])
def test_mixout_evaluate_is_the_functional_call_and_builds_no_graph(method):
    bpt, L = 16, 2
    if method == "noop":
        x, w, t = (a.to(DEV) for a in tr.case_inputs("sigmoid30", True))
    else:
        x, w, t = byte_float_inputs(method, 37, bpt, 256, 31)
    lm = CastedLinear(w.shape[1], w.shape[0]).to(DEV)
    with torch.no_grad():
        lm.weight.copy_(w)
    m = ByteMixout(ModelDims(model_dim=x.shape[1]), 64, ByteHyperparameters(bytes_per_token=bpt, byte_mixout_method=method, n_layer_out=L)).to(DEV)
    xb = x.to(torch.bfloat16).requires_grad_(True)
    with torch.enable_grad():
        ev = m.evaluate(xb[None], lm, t[None])   # (B, T, D) and (B, T or T * bpt), as GPT.forward holds them
        loss = m.loss(xb[None], lm, t[None])
    assert not any(a.requires_grad for a in ev) and ev.row_loss.grad_fn is None and loss.requires_grad
    assert ev.row_loss.shape == ev.pred.shape == ev.rank.shape == t[None].shape
    if method == "noop":
        direct = fn.token_head_eval(xb, w, t, softcap="sigmoid30", norm_in=True)
    else:
        direct = fn.byte_head_eval(xb, w, t, method=method, bytes_per_token=bpt, n_layer_out=L)
    assert same([a.reshape(-1) for a in ev], [a.reshape(-1) for a in direct])
    assert torch.equal(ev.loss, loss.detach()) and ev.counts.numel() == (2 if method == "noop" else 3)
