"""The compacted plain head (functional.plain_head_loss / plain_head_eval with max_kept, PlainLMHead, mot_plain_head_compact_*)
against float64 on the device (plain_head_ref.head on the values the kernel sees): kept counts from 0 to all rows at row counts that
are no multiple of any workgroup's share, kept runs across chunk seams, padding slots and whole padding chunks, the wide shapes of
the row pass, dropped and out-of-range targets between the kept ones, every element of dx written, the un-compacted call on the same
inputs, overflow, the evaluation form, determinism, hipGraph replay through a changing kept count (into and out of overflow),
autograd with a tied weight, and peak memory.

Bars, those of tests/test_gpu_plain_head.py: fp32 loss 2e-6 and gradients 2e-5 of the largest float64 element; bf16
err <= 2 * own + 2^-12, `own` being the eager bf16 restatement's error against float64 on the same bf16-valued inputs.  Every
figure is printed before it is asserted (pytest -s shows them).  Targets are built by construction: every kept count is known.

Measured on MI355X (worst over the sweep; compacted, then the eager path it is judged against): fp32 within the fixed bars
everywhere; bf16 with the norm dx 1.29e-2 (eager 1.78e-2), dW 1.64e-2 (1.49e-2), both at one kept row of 37.  With the norm the
compacted call rounds norm(x) to bf16 in front of the product, as F.rms_norm does in front of lm_head, so its bf16 loss equals the
eager restatement's to the printed digits; the un-compacted call scales the stored product in fp32 instead, another rounding of
equal standing."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mixture_of_tokenizers_amd as mot
import plain_head_ref as pr
from mixture_of_tokenizers_amd import _capi as capi
from mixture_of_tokenizers_amd import functional as fn
from mixture_of_tokenizers_amd.modules import PlainLMHead

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GOLDEN = np.load(Path(__file__).parent / "golden" / "plain_head.npz")
FP32_LOSS, FP32_GRAD = 2e-6, 2e-5
KEYS = ("loss", "dx", "dW")
BOTH = [torch.float32, torch.bfloat16]


def clear_status():
    capi.status_word(DEV).zero_()


def status():
    return int(capi.status_word(DEV).item())


def relerr(got, ref):
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    return float((got - ref).abs().max() / max(ref.abs().max().item(), 1e-300))


def fused(x, w, t, max_kept, norm_in=True, chunk_rows=32, ignore_index=-100):
    xl = x.detach().clone().requires_grad_(True)
    wl = w.detach().clone().requires_grad_(True)
    loss = fn.plain_head_loss(xl, wl, t, norm_in=norm_in, ignore_index=ignore_index, chunk_rows=chunk_rows, max_kept=max_kept)
    loss.backward()
    return {"loss": loss.detach(), "dx": xl.grad, "dW": wl.grad}


def references(x, w, t, dtype, norm_in=True, ignore_index=-100):
    """(float64 on the values the kernel sees, the eager restatement in bf16 or None)"""
    if dtype == torch.float32:
        return pr.head(x, w, t, norm_in, torch.float64, ignore_index), None
    xin = x.to(dtype)
    return (pr.head(xin.double(), w.to(dtype).double(), t, norm_in, torch.float64, ignore_index),
            pr.head(xin, w, t, norm_in, torch.bfloat16, ignore_index))


def bars(ref, eager):
    """the bar of each of loss, dx, dW as a share of the largest float64 element"""
    if eager is None:
        return {"loss": FP32_LOSS, "dx": FP32_GRAD, "dW": FP32_GRAD}
    return {k: 2 * relerr(eager[k], ref[k]) + 2 ** -12 for k in KEYS}


def hold(what, got, ref, eager):
    errs, bar = {k: relerr(got[k], ref[k]) for k in KEYS}, bars(ref, eager)
    print(f"{what}: " + ", ".join(f"{k} {errs[k]:.3e} (bar {bar[k]:.3e})" for k in KEYS))
    for k in KEYS:
        if eager is None:
            assert errs[k] < bar[k], (k, errs[k], bar[k])
        else:
            assert errs[k] <= bar[k], (k, errs[k], bar[k])


def check(what, x, w, t, dtype, max_kept, norm_in=True, chunk_rows=32, ignore_index=-100):
    """The compacted call on (x in dtype, fp32 w) against float64; the dropped rows of dx are +0 in every element."""
    got = fused(x.to(dtype), w, t, max_kept, norm_in, chunk_rows, ignore_index)
    assert got["dx"].dtype == dtype and got["dx"].shape == x.shape and got["dW"].dtype == torch.float32
    hold(f"{what} {dtype}", got, *references(x, w, t, dtype, norm_in, ignore_index))
    dropped = ~pr.kept_mask(t.reshape(-1), w.shape[0], ignore_index)
    rows = got["dx"].reshape(-1, x.shape[-1])[dropped]
    assert torch.equal(rows, torch.zeros_like(rows)) and not torch.signbit(rows).any()
    return got


def inputs(N, D, V, seed=0, std=4.0):
    g = torch.Generator(device=DEV).manual_seed(1000 * seed + N + D + V)
    x = torch.randn(N, D, device=DEV, generator=g)
    w = (torch.rand(V, D, device=DEV, generator=g) * 2 - 1) * (3 ** 0.5) * std * D ** -0.5   # std(l) about `std` with the norm
    y = torch.randint(0, V, (N,), device=DEV, generator=g)
    y[0], y[-1] = V - 1, 0   # the first and the last class occur
    return x, w, y


def keep_only(y, rows, ignore_index=-100):
    """y with every row but `rows` ignored: exactly len(rows) kept targets"""
    t = torch.full_like(y, ignore_index)
    rows = torch.as_tensor(rows, dtype=torch.long, device=y.device)
    t[rows] = y[rows]
    return t


def spread(N, k):
    """k distinct rows of N, ascending, spread over the whole range, the first and the last row among them (k >= 2)"""
    return sorted({int(r) for r in torch.linspace(0, N - 1, k).round().tolist()})


# ---- 1. the shape and count sweep at D 16, V 128, chunk_rows 32
def sweep_cases():
    out = []
    for N in (1, 37, 257, 1025):
        out.append((N, "none", [], min(N, 8)))
        out.append((N, "first", [0], 1))
        if N > 1:
            out.append((N, "last", [N - 1], min(N, 5)))
            out.append((N, "middle", [N // 2], min(N, 5)))
        out.append((N, "all", list(range(N)), N))
    out.append((257, "70 across two seams", spread(257, 70), 70))
    out.append((257, "20 of 70 slots", spread(257, 20), 70))
    out.append((1025, "70 across two seams", spread(1025, 70), 70))
    out.append((37, "9 of 10 slots", spread(37, 9), 10))
    out.append((37, "bound above the rows", spread(37, 9), 1000))
    # with and without the norm where cheap: the largest row count runs with it alone
    return [pytest.param(*c, dt, nrm, id=f"N{c[0]}-{c[1].replace(' ', '_')}-{str(dt)[6:]}-{'norm' if nrm else 'plain'}")
            for c in out for dt in BOTH for nrm in ((True, False) if c[0] < 1025 else (True,))]


@pytest.mark.parametrize("N, what, rows, max_kept, dtype, norm_in", sweep_cases())
def test_count_sweep(N, what, rows, max_kept, dtype, norm_in):
    x, w, y = inputs(N, 16, 128)
    t = keep_only(y, rows)
    assert len(set(rows)) == len(rows) and int((t != -100).sum()) == len(rows) <= max_kept
    clear_status()
    if not rows:   # nothing kept: NaN as torch's, gradients exactly zero, no status bit
        got = fused(x.to(dtype), w, t, max_kept, norm_in)
        assert torch.isnan(got["loss"])
        assert torch.equal(got["dx"], torch.zeros_like(got["dx"])) and torch.equal(got["dW"], torch.zeros_like(got["dW"]))
        with torch.no_grad():
            assert torch.isnan(fn.plain_head_loss(x.to(dtype), w, t, norm_in=norm_in, chunk_rows=32, max_kept=max_kept))
    else:
        got = check(f"N {N} kept {what} max_kept {max_kept} norm {norm_in}", x, w, t, dtype, max_kept, norm_in)
        assert (got["dx"][rows] != 0).any(-1).all()
    assert status() == 0


# ---- 2. the wide shapes: every register variant of the row pass meets gathered rows
WIDE = [  # (D, V, N, kept, max_kept, chunk_rows)
    (768, 50304, 70, 9, 32, 32), (2048, 640, 70, 40, 48, 32), (16, 65664, 37, 9, 12, 32), (16, 4224, 37, 20, 37, None),
]


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("D, V, N, kept, max_kept, chunk", WIDE)
def test_wide_shapes(D, V, N, kept, max_kept, chunk, dtype):
    x, w, y = inputs(N, D, V, seed=1)
    t = keep_only(y, spread(N, kept))
    clear_status()
    check(f"D {D} V {V} N {N} kept {kept} max_kept {max_kept}", x, w, t, dtype, max_kept, chunk_rows=chunk)
    assert status() == 0


# ---- 3. kept rows between ignored rows and out-of-range targets
@pytest.mark.parametrize("dtype", BOTH)
def test_dropped_and_out_of_range_targets_between_kept_rows(dtype):
    N, D, V = 70, 64, 640
    x, w, y = inputs(N, D, V, seed=2, std=2.0)
    t = y.clone()
    t[1::3] = -100
    bad = {5: -1, 17: V, 41: 1 << 40, 44: -(1 << 40)}
    for r, v in bad.items():
        t[r] = v
    kept = int(pr.kept_mask(t, V).sum())
    assert kept == N - len(range(1, N, 3)) - len([r for r in bad if r % 3 != 1])
    clear_status()
    got = check("out of range between kept rows", x, w, t, dtype, kept)
    assert status() == capi.STATUS_TARGET_OOR   # and nothing else
    with pytest.raises(IndexError, match="target"):
        mot.check_status()
    for r in bad:
        assert (got["dx"][r] == 0).all()
    # a non-default ignore_index inside [0, V): its class is dropped silently, -100 is then out of range
    t2 = y.clone()
    t2[::4] = 7
    kept2 = int(pr.kept_mask(t2, V, 7).sum())
    check("ignore_index 7", x, w, t2, dtype, kept2, ignore_index=7)
    assert status() == 0
    check("ignore_index 2^40 (no target takes it)", x, w, y, dtype, N, ignore_index=1 << 40)
    assert status() == 0


# ---- 4. every element of dx is written: the C call on caller-owned buffers, dx and dW prefilled with NaN
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("kept, max_kept", [(20, 70), (0, 16), (70, 70)])
def test_every_element_of_dx_is_written(kept, max_kept, dtype):
    N, D, V = 257, 64, 640
    x, w, y = inputs(N, D, V, seed=3, std=2.0)
    rows = spread(N, kept) if kept else []
    t = keep_only(y, rows)
    xin, win = x.to(dtype).contiguous(), w.to(dtype).contiguous()
    dx = torch.full_like(xin, float("nan"))
    dw = torch.full((V, D), float("nan"), device=DEV)
    loss = torch.full((), float("nan"), device=DEV)
    d = capi.MotPlainHeadDesc()
    d.struct_size = C.sizeof(capi.MotPlainHeadDesc)
    d.dtype, d.norm_in, d.chunk_rows, d.n_rows, d.model_dim, d.vocab, d.ignore_index = capi.dtype_code(dtype), 1, 32, N, D, V, -100
    d.x, d.weight, d.targets, d.loss, d.dx, d.dW = (capi.ptr(a) for a in (xin, win, t, loss, dx, dw))
    c = capi.MotPlainHeadCompact()
    c.struct_size, c.reserved, c.max_kept = C.sizeof(capi.MotPlainHeadCompact), 0, max_kept
    need = capi.lib.mot_plain_head_compact_workspace_bytes(C.byref(d), C.byref(c))
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)   # a stale index entry would name row 0, a kept row when any is kept
    clear_status()
    d.workspace, d.workspace_bytes, d.status = capi.ptr(ws), need, capi.ptr(capi.status_word(DEV))
    capi.check(capi.lib.mot_plain_head_compact_fwd(C.byref(d), C.byref(c), capi.stream_of(DEV)))
    torch.cuda.synchronize()
    assert status() == 0
    assert torch.isfinite(dx).all() and torch.isfinite(dw).all()
    dropped = t == -100
    assert torch.equal(dx[dropped], torch.zeros_like(dx[dropped])) and not torch.signbit(dx[dropped]).any()
    if kept:
        assert (dx[~dropped] != 0).any(-1).all()
        hold(f"C call kept {kept} max_kept {max_kept} {dtype}", {"loss": loss, "dx": dx, "dW": dw}, *references(x, w, t, dtype))
    else:
        assert torch.isnan(loss) and torch.equal(dw, torch.zeros_like(dw))


# ---- 5. against the un-compacted call on the same inputs: no further apart than the sum of the two bars
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("D, V, N, kept, max_kept", [(64, 640, 257, 70, 70), (768, 50304, 70, 9, 32)])
def test_against_the_uncompacted_call(D, V, N, kept, max_kept, dtype):
    x, w, y = inputs(N, D, V, seed=4, std=2.0)
    t = keep_only(y, spread(N, kept))
    xin = x.to(dtype)
    a, b = fused(xin, w, t, max_kept), fused(xin, w, t, None)
    ref, eager = references(x, w, t, dtype)
    bar = bars(ref, eager)
    for k in KEYS:
        gap = float((a[k].double() - b[k].double()).abs().max() / ref[k].abs().max())
        print(f"D {D} V {V} {dtype}: {k} compacted against un-compacted {gap:.3e} (two bars {2 * bar[k]:.3e})")
        assert gap <= 2 * bar[k]


# ---- 6. overflow: kept = max_kept + 1 scores nothing and says so
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("N, max_kept", [(37, 8), (257, 32), (257, 64), (1025, 1)])
def test_overflow_scores_nothing_and_raises_the_status_bit(N, max_kept, dtype):
    x, w, y = inputs(N, 16, 128, seed=5)
    t = keep_only(y, spread(N, max_kept + 1))
    assert int((t != -100).sum()) == max_kept + 1
    clear_status()
    got = fused(x.to(dtype), w, t, max_kept)
    assert torch.isnan(got["loss"])
    assert torch.equal(got["dx"], torch.zeros_like(got["dx"])) and torch.equal(got["dW"], torch.zeros_like(got["dW"]))
    assert status() == capi.STATUS_KEPT_OVERFLOW
    with pytest.raises(IndexError, match="kept overflow"):
        mot.check_status()
    assert status() == 0
    ev = fn.plain_head_eval(x.to(dtype), w, t, chunk_rows=32, max_kept=max_kept)
    assert torch.isnan(ev.loss) and (ev.pred == -1).all() and (ev.rank == -1).all() and (ev.row_loss == 0).all()
    assert ev.counts.tolist() == [max_kept + 1, 0]
    assert status() == capi.STATUS_KEPT_OVERFLOW
    clear_status()
    t[N // 2 if t[N // 2] != -100 else 0] = -100   # one fewer: back inside the bound
    assert int((t != -100).sum()) == max_kept
    check(f"N {N} kept = max_kept = {max_kept}", x, w, t, dtype, max_kept)
    assert status() == 0


# ---- 7. the evaluation form on the reference's fixture
@pytest.mark.parametrize("vocab", pr.VOCABS)
def test_evaluation_on_the_math_fixture(vocab):
    x, w, y, idx = pr.case_inputs("math", vocab)
    max_kept = mot.window_kept_bound(idx, pr.T)   # host ranges: no device read
    x, w, t = x.to(DEV), w.to(DEV), mot.window_targets(y.to(DEV), idx.to(DEV))
    assert max_kept == int((t != -100).sum()) < t.numel()
    clear_status()
    ev = fn.plain_head_eval(x, w, t, group_rows=pr.T, max_kept=max_kept)
    full = fn.plain_head_eval(x, w, t, group_rows=pr.T)
    want = GOLDEN[pr.case_key("math", vocab, "f64", "counts")].tolist()   # scored rows, right rows, sequences all right
    assert ev.counts.tolist() == want == full.counts.tolist()
    assert ev.pred.shape == ev.rank.shape == ev.row_loss.shape == t.shape
    keep = t != -100
    e = relerr(ev.row_loss[keep], full.row_loss[keep])
    print(f"V {vocab}: row_loss of the kept rows against the un-compacted evaluation {e:.3e}")
    assert e < FP32_LOSS
    assert torch.equal(ev.rank[keep], full.rank[keep]) and torch.equal(ev.pred[keep], full.pred[keep])
    assert (ev.pred[~keep] == -1).all() and (ev.rank[~keep] == -1).all() and (ev.row_loss[~keep] == 0).all()
    assert (full.pred[~keep] >= 0).all()   # the documented difference: the un-compacted evaluation still writes them
    with torch.no_grad():
        assert torch.equal(fn.plain_head_loss(x, w, t, max_kept=max_kept), ev.loss)
    ref = float(GOLDEN[pr.case_key("math", vocab, "f64", "loss")])
    assert abs(ev.loss.item() - ref) < FP32_LOSS * ref
    two = fn.plain_head_eval(x, w, t, max_kept=max_kept + 3)   # a looser bound, two counts
    assert two.counts.tolist() == want[:2] and torch.equal(two.pred, ev.pred) and torch.equal(two.rank, ev.rank)
    assert status() == 0


@pytest.mark.parametrize("dtype", BOTH)
def test_evaluation_on_exact_integer_products(dtype):
    """x and W in {-1, 0, 1}: every stored product is a small integer, exact in fp32 and bf16 on every product route, so pred,
    rank and the counts are judged exactly, ties included, with out-of-range targets between the kept rows."""
    N, D, V, group = 96, 64, 640, 8
    g = torch.Generator(device=DEV).manual_seed(N + V)
    x = torch.randint(-1, 2, (N, D), device=DEV, generator=g).float()
    w = torch.randint(-1, 2, (V, D), device=DEV, generator=g).float()
    s = x.double() @ w.double().T
    t = torch.randint(0, V, (N,), device=DEV, generator=g)
    t[::2] = s[::2].argmax(-1)
    t[1::5] = -100
    t[2] = V
    t[8:16] = -100                      # a group with no kept row
    kept = pr.kept_mask(t, V)
    clear_status()
    ev = fn.plain_head_eval(x.to(dtype), w, t, norm_in=False, chunk_rows=32, group_rows=group, max_kept=int(kept.sum()) + 2)
    assert status() == capi.STATUS_TARGET_OOR
    clear_status()
    row_loss, pred, rank = pr.rows(s, torch.ones(N, device=DEV), t)
    assert torch.equal(ev.pred[kept], pred[kept]) and (ev.pred[~kept] == -1).all() and torch.equal(ev.rank, rank)
    e = relerr(ev.row_loss, row_loss)
    print(f"{dtype}: row_loss {e:.3e}")
    assert e < FP32_LOSS
    assert ev.counts.tolist() == pr.counts(pred, t, V, group_rows=group)


# ---- 8. determinism
@pytest.mark.parametrize("dtype", BOTH)
def test_deterministic(dtype):
    N, D, V = 257, 64, 640
    x, w, y = inputs(N, D, V, seed=6, std=2.0)
    t = keep_only(y, spread(N, 70))
    xin = x.to(dtype)
    a, b = fused(xin, w, t, 80), fused(xin, w, t, 80)
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["dx"], b["dx"])
    ref, eager = references(x, w, t, dtype)
    hold(f"first run {dtype}", a, ref, eager)    # dW is summed with atomics: both runs are held to the bar
    hold(f"second run {dtype}", b, ref, eager)


# ---- 9. hipGraph capture of forward + backward; the targets change in place between replays, and with them `kept`
@pytest.mark.parametrize("dtype", BOTH)
def test_hipgraph_replay_follows_the_kept_count(dtype):
    N, D, V, max_kept = 257, 64, 640, 64
    x, w, y = inputs(N, D, V, seed=7, std=2.0)
    xin = x.to(dtype)
    g = torch.Generator(device=DEV).manual_seed(70)
    sets = {k: keep_only(y, sorted(torch.randperm(N, device=DEV, generator=g)[:k].tolist())) for k in (64, 5, 65, 40)}
    xs, ws, ts = xin.clone().requires_grad_(True), w.clone().requires_grad_(True), sets[40].clone()

    def step():
        loss = fn.plain_head_loss(xs, ws, ts, chunk_rows=32, max_kept=max_kept)
        loss.backward()
        return loss

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            xs.grad = ws.grad = None
            step()
    torch.cuda.current_stream().wait_stream(s)
    xs.grad = ws.grad = None
    clear_status()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = step()
    for k in (64, 5, 65, 40):   # the shrinking count must not pick up the index entries of the replay before it
        with torch.no_grad():
            ts.copy_(sets[k])
        graph.replay()
        torch.cuda.synchronize()
        if k > max_kept:
            assert torch.isnan(loss)
            assert torch.equal(xs.grad, torch.zeros_like(xs.grad)) and torch.equal(ws.grad, torch.zeros_like(ws.grad))
            assert status() == capi.STATUS_KEPT_OVERFLOW
            with pytest.raises(IndexError, match="kept overflow"):
                mot.check_status()
            continue
        assert status() == 0
        hold(f"replay with {k} kept {dtype}", {"loss": loss, "dx": xs.grad, "dW": ws.grad}, *references(x, w, sets[k], dtype))
        dropped = sets[k] == -100
        assert torch.equal(xs.grad[dropped], torch.zeros_like(xs.grad[dropped]))


# ---- 10. autograd
@pytest.mark.parametrize("dtype", BOTH)
def test_tied_embedding_and_lm_head_receive_both_gradients(dtype):
    """wte.weight = lm_head.weight (mathblations/model.py:317): the one parameter gets the embedding's gradient and the head's."""
    V, D, Bq, Tq = 256, 32, 4, 16
    g = torch.Generator(device=DEV).manual_seed(21)
    lm_head = torch.nn.Linear(D, V, bias=False).to(DEV)
    wte = torch.nn.Embedding(V, D).to(DEV)
    wte.weight = lm_head.weight
    head = PlainLMHead(lm_head)
    idx = torch.randint(0, V, (Bq, Tq), device=DEV, generator=g)
    y = torch.randint(0, V, (Bq, Tq), device=DEV, generator=g)
    ranges = [(3, 9), (0, 16), (15, 16), (7, 8)]
    max_kept = mot.window_kept_bound(ranges, Tq)
    assert max_kept == 6 + 16 + 1 + 1
    t = mot.window_targets(y, ranges)
    body = lambda e: (e * 1.5 + 0.25).to(dtype)   # stands for the blocks
    loss = head.loss(body(wte(idx)), t, max_kept=max_kept)
    loss.backward()
    got = lm_head.weight.grad.clone()
    assert got.dtype == torch.float32 and lm_head.weight.grad is wte.weight.grad
    w2 = lm_head.weight.detach().clone().requires_grad_(True)
    x2 = body(F.embedding(idx, w2))
    if dtype == torch.float32:
        l = F.linear(F.rms_norm(x2.double(), (D,)), w2.double())
    else:
        l = F.linear(F.rms_norm(x2, (D,)), w2.to(dtype)).float()
    ref = F.cross_entropy(l.reshape(-1, V), t.reshape(-1))
    ref.backward()
    e = relerr(got, w2.grad)
    emb_only = torch.autograd.grad(body(F.embedding(idx, w2)).float().sum(), w2)[0]
    print(f"tied weight {dtype}: loss {loss.item():.6f} vs {ref.item():.6f}, grad {e:.3e}")
    assert (emb_only != 0).any() and e < (FP32_GRAD if dtype == torch.float32 else 2 ** -5)
    assert abs(loss.item() - ref.item()) < (FP32_LOSS if dtype == torch.float32 else 2 ** -7) * ref.item()
    ev = head.evaluate(body(wte(idx)), t, group_rows=Tq, max_kept=max_kept)
    assert torch.equal(ev.loss, loss.detach()) and ev.counts.shape == (3,) and ev.counts[0].item() == max_kept
    assert (ev.pred[t == -100] == -1).all()


def test_grad_loss_scales_both_gradients():
    N, D, V = 70, 64, 640
    x, w, y = inputs(N, D, V, seed=8, std=2.0)
    t = keep_only(y, spread(N, 20))
    one = fused(x, w, t, 24)
    xl, wl = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    (3.5 * fn.plain_head_loss(xl, wl, t, chunk_rows=32, max_kept=24)).backward()
    ex, ew = relerr(xl.grad, 3.5 * one["dx"]), relerr(wl.grad, 3.5 * one["dW"])
    print(f"grad_loss 3.5: dx {ex:.3e}, dW {ew:.3e}")
    assert xl.grad.shape == x.shape and ex < 1e-6 and ew < 1e-6
    xo = x.clone().requires_grad_(True)   # one-sided: dx alone, the same bits
    fn.plain_head_loss(xo, w, t, chunk_rows=32, max_kept=24).backward()
    assert torch.equal(xo.grad, one["dx"])
    with torch.no_grad():
        assert torch.equal(fn.plain_head_loss(x, w, t.int(), chunk_rows=32, max_kept=24), one["loss"])


# ---- 11. memory: the compacted step's peak lies below the un-compacted step's on the same inputs
def test_peak_memory_below_the_uncompacted_step():
    N, D, V = 4096, 768, 50304
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn(N, D, device=DEV, generator=g).requires_grad_(True)
    w = ((torch.rand(V, D, device=DEV, generator=g) * 2 - 1) * 0.03).requires_grad_(True)
    t = torch.full((N,), -100, device=DEV)
    t[::16] = torch.randint(0, 50257, (N // 16,), device=DEV, generator=g)   # 1 row in 16 kept: 256

    def peak(max_kept):
        x.grad = w.grad = None
        fn.release_workspaces()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        loss = fn.plain_head_loss(x, w, t, max_kept=max_kept)
        loss.backward()
        torch.cuda.synchronize()
        assert torch.isfinite(loss) and torch.isfinite(w.grad).all()
        return torch.cuda.max_memory_allocated() - base, loss.item()

    compact, loss_c = peak(256)
    plain, loss_p = peak(None)
    fn.release_workspaces()
    mib = lambda b: f"{b / 2**20:.1f} MiB"
    print(f"peak extra memory of forward + backward at 4096 x 768 x 50 304 fp32, 256 rows kept: compacted {mib(compact)}, "
          f"un-compacted {mib(plain)}; losses {loss_c:.6f} / {loss_p:.6f}")
    assert compact < plain
    assert abs(loss_c - loss_p) < 2 * FP32_LOSS * abs(loss_p)
