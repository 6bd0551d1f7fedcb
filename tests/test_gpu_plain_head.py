"""The fused plain cross-entropy head (functional.plain_head_loss / plain_head_eval, modules.PlainLMHead, csrc/mot_plainhead.hip)
against float64 on the device: the reference's fixture cases (a scored window equals ignored targets), every variant of the row
pass, logits far beyond what a softcap leaves, ignore_index and other dropped targets, the evaluation form with grouped counts,
determinism, hipGraph replay with a changing number of kept targets, autograd with a tied weight, and peak memory.

Bars, as tests/test_gpu_token_head.py sets them: fp32 loss 2e-6 and gradients 2e-5 of the largest float64 element; bf16
err <= 2 * own + 2^-12, `own` being the eager bf16 restatement's error against float64 on the same bf16-valued inputs.  The
large-logit cases are judged against the eager fp32 restatement instead: err <= 2 * its own error against float64.  Every figure is
printed before it is asserted (pytest -s shows them).

Measured on MI355X (worst over the cases of each test; fused, then the eager path it is judged against):
  fixtures fp32: loss 5.9e-8, dx 7.6e-7, dW 7.7e-7;  variant sweep fp32: loss 1.4e-7, dx 1.7e-6, dW 7.3e-7
  logits to +-100 / +-300, fp32: loss 8.0e-8 (eager fp32 8.0e-8), dx 2.95e-6 (2.95e-6), dW 1.45e-6 (1.45e-6)
  the same on random bf16 inputs (finiteness and the loss are asserted): dW 1.3e-2 against eager bf16's 6.1e-3 at +-300
  exactly representable logits -368 .. 352: fp32 dx 2.6e-7, bf16 dx 9.8e-4 (eager 9.8e-4)
  peak extra memory at 4096 x 50 304 fp32: 658 MiB (workspace 499, dx 12, dW 147) against 786 MiB of logits."""
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


def relerr(got, ref):
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    return float((got - ref).abs().max() / max(ref.abs().max().item(), 1e-300))


def fused(x, w, t, norm_in=True, chunk_rows=None, ignore_index=-100):
    xl = x.detach().clone().requires_grad_(True)
    wl = w.detach().clone().requires_grad_(True)
    loss = fn.plain_head_loss(xl, wl, t, norm_in=norm_in, ignore_index=ignore_index, chunk_rows=chunk_rows)
    loss.backward()
    return {"loss": loss.detach(), "dx": xl.grad, "dW": wl.grad}


def check_fp32(what, got, ref):
    errs = {k: relerr(got[k], ref[k]) for k in KEYS}
    print(f"{what} fp32: " + ", ".join(f"{k} {errs[k]:.3e}" for k in KEYS) + f"  (bars {FP32_LOSS:.0e} / {FP32_GRAD:.0e})")
    assert errs["loss"] < FP32_LOSS, errs
    assert errs["dx"] < FP32_GRAD and errs["dW"] < FP32_GRAD, errs


def check_bf16(what, got, ref, eager):
    errs = {k: relerr(got[k], ref[k]) for k in KEYS}
    own = {k: relerr(eager[k], ref[k]) for k in KEYS}
    print(f"{what} bf16: " + ", ".join(f"{k} {errs[k]:.3e} (eager {own[k]:.3e})" for k in KEYS))
    for k in KEYS:
        assert errs[k] <= 2 * own[k] + 2 ** -12, f"{k}: {errs[k]:.3e} vs eager bf16 {own[k]:.3e}"


def check(what, x, w, t, dtype, norm_in=True, chunk_rows=None, ignore_index=-100):
    """The fused call on (x in dtype, fp32 w) against float64 on the values the kernel sees."""
    xin = x.to(dtype)
    got = fused(xin, w, t, norm_in, chunk_rows, ignore_index)
    assert got["dx"].dtype == dtype and got["dx"].shape == x.shape and got["dW"].dtype == torch.float32
    if dtype == torch.float32:
        check_fp32(what, got, pr.head(x, w, t, norm_in, torch.float64, ignore_index))
    else:
        ref = pr.head(xin.double(), w.to(dtype).double(), t, norm_in, torch.float64, ignore_index)
        check_bf16(what, got, ref, pr.head(xin, w, t, norm_in, torch.bfloat16, ignore_index))
    return got


# ---- 1. the fixture cases: the reference's sliced loss equals the fused loss on window_targets; the shifted labels with -100
def fixture_operands(kind, vocab):
    x, w, y, idx = (None if a is None else a.to(DEV) for a in pr.case_inputs(kind, vocab))
    if kind == "math":
        return x, w, mot.window_targets(y, idx), True, slice(None)
    return x[:, :-1].contiguous(), w, y[:, 1:].contiguous(), False, slice(0, -1)


@pytest.mark.parametrize("vocab", pr.VOCABS)
@pytest.mark.parametrize("kind", pr.KINDS)
def test_fixture_fp32(kind, vocab):
    x, w, t, norm_in, cut = fixture_operands(kind, vocab)
    assert t.is_cuda and (t == -100).any()
    got = fused(x, w, t, norm_in)
    ref = {k: torch.from_numpy(np.asarray(GOLDEN[pr.case_key(kind, vocab, "f64", k)])) for k in KEYS}
    ref["dx"] = ref["dx"][:, cut]
    own = GOLDEN[pr.case_key(kind, vocab, "f32", "err")]
    print(f"fixture {kind} V {vocab}: the reference's own float32 error loss {own[0]:.3e}, dx {own[1]:.3e}, dW {own[2]:.3e}")
    check_fp32(f"fixture {kind} V {vocab}", got, ref)


@pytest.mark.parametrize("vocab", pr.VOCABS)
@pytest.mark.parametrize("kind", pr.KINDS)
def test_fixture_bf16(kind, vocab):
    x, w, t, norm_in, _ = fixture_operands(kind, vocab)
    check(f"fixture {kind} V {vocab}", x, w, t, torch.bfloat16, norm_in)


@pytest.mark.parametrize("vocab", pr.VOCABS)
def test_fixture_evaluation_counts_are_the_reference_accuracies(vocab):
    x, w, t, _, _ = fixture_operands("math", vocab)
    ev = fn.plain_head_eval(x, w, t, group_rows=pr.T)
    want = GOLDEN[pr.case_key("math", vocab, "f64", "counts")].tolist()   # scored rows, right rows, sequences all right
    assert ev.counts.tolist() == want and ev.pred.shape == t.shape
    ref = float(GOLDEN[pr.case_key("math", vocab, "f64", "loss")])
    assert abs(ev.loss.item() - ref) < FP32_LOSS * ref


# ---- 2. every variant of the row pass and both workgroup sizes.  Row pass per shape, fp32 / bf16:
#   V 128: 256 threads NV 4 / same;  V 4224: 1024 threads NV 4 with a ragged round / 256 threads NV 4;  V 32 768: NV 8 / NV 4;
#   V 50 304: NV 16 ragged / NV 8 ragged;  V 65 536: NV 16 / NV 8, both full;  V 65 664: read twice (NV 0) / same
SWEEP = [  # (D, V, N, chunk_rows)
    (16, 128, 1, None), (2048, 128, 257, None), (16, 4224, 37, 32), (2048, 640, 37, None), (16, 32768, 37, None),
    (768, 50304, 70, 32), (16, 65536, 37, None), (16, 65664, 37, 32), (48, 65664, 1, None),
]


@pytest.mark.parametrize("norm_in", [True, False])
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("D, V, N, chunk", SWEEP)
def test_variant_sweep(D, V, N, chunk, dtype, norm_in):
    g = torch.Generator(device=DEV).manual_seed(D + V + N)
    x = torch.randn(N, D, device=DEV, generator=g)
    w = (torch.rand(V, D, device=DEV, generator=g) * 2 - 1) * (3 ** 0.5) * 4.0 * D ** -0.5   # std(l) 4
    t = torch.randint(0, V, (N,), device=DEV, generator=g)
    t[0], t[-1] = V - 1, 0 if N > 1 else V - 1
    if N > 4:
        t[3::5] = -100   # kept and ignored rows in every chunk; rows 0 and N - 1 stay kept
    check(f"D {D} V {V} N {N} norm {norm_in}", x, w, t, dtype, norm_in=norm_in, chunk_rows=chunk)


# ---- 3. logits the capped head could not take
def large_logit_inputs(reach, norm_in=True):
    """33 rows x 1024 classes at D 64: 29 random rows whose logits reach about +-`reach`, a row with one logit `reach` above equal
    others, a row of equal logits, a zero row, and one more random row.  Columns 0 and 1 of W and its first 64 rows are set by hand
    so that those rows can be written down exactly."""
    D, V, N = 64, 1024, 33
    g = torch.Generator(device=DEV).manual_seed(int(reach))
    x = torch.randn(N, D, device=DEV, generator=g)
    w = torch.randn(V, D, device=DEV, generator=g)
    w[:64] = 0
    w[:, :2] = 0
    l = (F.rms_norm(x, (D,)) if norm_in else x) @ w.T
    w = w * (reach / l[:29].abs().max())
    w[0, 0] = reach / 8                  # with x = 8 e_0 (the norm's c = 1): logit `reach` in class 0, every other class exactly 0
    x[29] = 0
    x[29, 0] = 8.0
    w[:, 1] = 0.25                       # with x = 8 e_1: a row of equal logits, 2 each
    x[30] = 0
    x[30, 1] = 8.0
    x[31] = 0                            # the zero row: logits 0 whatever the norm's factor
    t = torch.randint(0, V, (N,), device=DEV, generator=g)
    t[29], t[30], t[31] = 5, 1023, 0
    return x, w, t


@pytest.mark.parametrize("norm_in", [True, False])
@pytest.mark.parametrize("reach", [100.0, 300.0])
def test_large_logits_fp32_against_eager_fp32(reach, norm_in):
    x, w, t = large_logit_inputs(reach, norm_in)
    ref = pr.head(x, w, t, norm_in, torch.float64)
    l = (F.rms_norm(x.double(), (64,), eps=pr.FLT_EPS) if norm_in else x.double()) @ w.double().T
    assert reach * 0.9 < l[:29].abs().max().item() and l[29, 0].item() - l[29, 1:].max().item() >= reach * 0.99
    assert (l[30] == l[30, 0]).all() and (l[31] == 0).all()
    eager = pr.head(x, w, t, norm_in, torch.float32)
    assert all(torch.isfinite(eager[k]).all() for k in KEYS)
    got = fused(x, w, t, norm_in)
    errs = {k: relerr(got[k], ref[k]) for k in KEYS}
    own = {k: relerr(eager[k], ref[k]) for k in KEYS}
    print(f"logits to +-{reach:.0f} norm {norm_in} fp32: " + ", ".join(f"{k} {errs[k]:.3e} (eager fp32 {own[k]:.3e})" for k in KEYS))
    assert torch.isfinite(got["loss"]) and ref["loss"].item() > reach / 4
    for k in KEYS:
        assert errs[k] <= 2 * own[k], f"{k}: {errs[k]:.3e} vs twice eager fp32's {own[k]:.3e}"


@pytest.mark.parametrize("reach", [100.0, 300.0])
def test_large_logits_bf16_stay_finite(reach):
    """A bf16 logit near 300 is stored to a spacing of 2, so every softmax probability of such a row carries a factor of up to e:
    on random inputs the fused call and the eager bf16 path are two different roundings of a result that bf16 does not determine,
    and their gradients cannot be held to one another (both figures are printed).  What holds is that nothing overflows, and that
    the loss, a mean of lse - l[y] whose terms err by about one spacing each, stays within the bf16 bar of the eager path.  The
    gradients at large bf16 logits are judged on exactly representable logits in the next test."""
    x, w, t = large_logit_inputs(reach)
    xin = x.to(torch.bfloat16)
    got = fused(xin, w, t)
    ref = pr.head(xin.double(), w.bfloat16().double(), t, True, torch.float64)
    eager = pr.head(xin, w, t, True, torch.bfloat16)
    errs = {k: relerr(got[k], ref[k]) for k in KEYS}   # relerr asserts finiteness
    own = {k: relerr(eager[k], ref[k]) for k in KEYS}
    print(f"logits to +-{reach:.0f} bf16: " + ", ".join(f"{k} {errs[k]:.3e} (eager {own[k]:.3e})" for k in KEYS))
    assert torch.isfinite(got["loss"]) and errs["loss"] <= 2 * own["loss"] + 2 ** -12


@pytest.mark.parametrize("dtype", BOTH)
def test_large_logits_exactly_representable(dtype):
    """x in {-1, 0, 1}^64 and W in 16 {-1, 0, 1}: every logit is a multiple of 16 up to 1024 in size, exact in fp32 and in bf16
    (16 k with |k| <= 64 needs 7 bits), so the stored product carries no rounding and the fused call and the eager path see the same
    logits, hundreds apart.  fp32 is held to the fixed bars, bf16 to err <= 2 own + 2^-12."""
    N, D, V = 70, 64, 1024
    g = torch.Generator(device=DEV).manual_seed(8)
    x = torch.randint(-1, 2, (N, D), device=DEV, generator=g).float()
    w = torch.randint(-1, 2, (V, D), device=DEV, generator=g).float() * 16
    t = torch.randint(0, V, (N,), device=DEV, generator=g)
    t[::9] = -100
    l = x.double() @ w.double().T
    assert l.max().item() >= 250 and l.min().item() <= -250 and torch.equal(l.to(dtype).double(), l)
    check(f"exact logits {l.min().item():.0f} .. {l.max().item():.0f}", x, w, t, dtype, norm_in=False, chunk_rows=32)


# ---- 4. ignore_index and the other dropped targets
def small_inputs(seed=5, N=70, D=64, V=640):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(N, D, device=DEV, generator=g)
    w = torch.randn(V, D, device=DEV, generator=g) * 0.5
    t = torch.randint(0, V, (N,), device=DEV, generator=g)
    return x, w, t


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("share", ["none", "some"])
def test_ignored_rows_leave_the_mean(share, dtype):
    x, w, t = small_inputs()
    if share == "some":
        t[::3] = -100
        t[33:64] = -100   # a whole chunk of 32 but one row
    clear_status()
    got = check(f"ignored {share}", x, w, t, dtype, chunk_rows=32)
    assert int(capi.status_word(DEV).item()) == 0   # ignored rows raise nothing
    keep = t != -100
    assert (got["dx"][~keep] == 0).all() and (got["dx"][keep] != 0).any(-1).all()
    l = F.rms_norm(x.to(dtype).double(), (64,)) @ w.to(dtype).double().T
    ce = F.cross_entropy(l, t, ignore_index=-100)   # the mean over the kept rows, not over all 70
    bar = FP32_LOSS if dtype == torch.float32 else 2 ** -8
    assert abs(got["loss"].item() - ce.item()) < bar * ce.item()


@pytest.mark.parametrize("dtype", BOTH)
def test_all_rows_ignored(dtype):
    x, w, t = small_inputs()
    t[:] = -100
    clear_status()
    xl, wl = x.to(dtype).requires_grad_(True), w.clone().requires_grad_(True)
    loss = fn.plain_head_loss(xl, wl, t, chunk_rows=32)
    loss.backward()
    assert torch.isnan(loss) and (xl.grad == 0).all() and (wl.grad == 0).all()
    assert int(capi.status_word(DEV).item()) == 0
    with torch.no_grad():
        assert torch.isnan(fn.plain_head_loss(xl, wl, t))


@pytest.mark.parametrize("dtype", BOTH)
def test_non_default_ignore_index(dtype):
    x, w, t = small_inputs()
    t[::4] = 7
    t[1] = -100   # no longer the ignored value: out of range, dropped with the status bit
    clear_status()
    got = check("ignore_index 7", x, w, t, dtype, ignore_index=7)
    assert (got["dx"][::4] == 0).all() and (got["dx"][1] == 0).all()
    with pytest.raises(IndexError, match="target"):
        mot.check_status()
    t[1] = 3
    got = check("ignore_index 2^40 (no target takes it)", x, w, t, dtype, ignore_index=1 << 40)
    assert (got["dx"] != 0).any(-1).all()
    mot.check_status()


@pytest.mark.parametrize("dtype", BOTH)
def test_out_of_range_targets_are_dropped_with_the_status_bit(dtype):
    x, w, t = small_inputs()
    V = w.shape[0]
    bad = {5: -1, 17: V, 40: 1 << 40, 41: -(1 << 40)}
    for r, v in bad.items():
        t[r] = v
    t[6] = -100
    clear_status()
    got = check("out of range", x, w, t, dtype, chunk_rows=32)
    assert int(capi.status_word(DEV).item()) & capi.STATUS_TARGET_OOR
    with pytest.raises(IndexError, match="target"):
        mot.check_status()
    for r in (*bad, 6):
        assert (got["dx"][r] == 0).all()
    keep = (t >= 0) & (t < V)
    l = F.rms_norm(x.to(dtype).double(), (64,)) @ w.to(dtype).double().T
    ce = F.cross_entropy(l[keep], t[keep])   # divides by the 65 kept rows
    assert int(keep.sum()) == 65 and abs(got["loss"].item() - ce.item()) < (FP32_LOSS if dtype == torch.float32 else 2 ** -8) * ce.item()


# ---- 5. the evaluation form
def ternary(shape, g):
    return torch.randint(-1, 2, shape, device=DEV, generator=g).float()


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("N, D, V, chunk", [(96, 64, 640, 32), (32, 16, 65664, None), (40, 32, 50304, 32)])
def test_evaluation_on_exact_integer_products(N, D, V, chunk, dtype):
    """x and W in {-1, 0, 1}: every stored product is a small integer, exact in fp32 and bf16, so pred, rank and the counts are
    judged exactly, ties (there are many) included, and row_loss against float64 of the same integers."""
    g = torch.Generator(device=DEV).manual_seed(N + V)
    x, w = ternary((N, D), g), ternary((V, D), g)
    t = torch.randint(0, V, (N,), device=DEV, generator=g)
    s = x.double() @ w.double().T
    t[::2] = s[::2].argmax(-1)          # right rows (an argmax; not always the lowest class of a tie)
    t[1] = -100
    t[2] = V
    group = 8
    t[8:16] = -100                      # a group with no kept row
    t[16:24] = pr.rows(s[16:24], torch.ones(8, device=DEV), t[16:24])[1].long()   # a group whose rows are all right
    t[17] = -100                        # ... one of them ignored: it does not break the group
    t[24:32] = pr.rows(s[24:32], torch.ones(8, device=DEV), t[24:32])[1].long()
    t[30] = (t[30] + 1) % V             # a group with a single wrong row: pred is the lowest class of the maximum, never this one
    clear_status()
    ev = fn.plain_head_eval(x.to(dtype), w, t, norm_in=False, chunk_rows=chunk, group_rows=group)
    clear_status()
    row_loss, pred, rank = pr.rows(s, torch.ones(N, device=DEV), t)
    assert torch.equal(ev.pred, pred) and torch.equal(ev.rank, rank)
    assert (ev.rank[[1, 2]] == -1).all() and (ev.row_loss[[1, 2]] == 0).all()
    e = relerr(ev.row_loss, row_loss)
    print(f"N {N} D {D} V {V} {dtype}: row_loss {e:.3e}")
    assert e < FP32_LOSS
    want = pr.counts(pred, t, V, group_rows=group)
    assert ev.counts.tolist() == want, (ev.counts.tolist(), want)
    k, h = ((t >= 0) & (t < V)).reshape(-1, group), (pred.long() == t).reshape(-1, group)
    assert not k[1].any() and bool((h | ~k)[2].all()) and k[2].sum() == 7
    two = fn.plain_head_eval(x.to(dtype), w, t, norm_in=False, chunk_rows=chunk)
    clear_status()
    assert two.counts.tolist() == want[:2] and torch.equal(two.pred, ev.pred)
    # the loss has the bits of the loss call, and the norm's factor changes no order
    with torch.no_grad():
        assert torch.equal(fn.plain_head_loss(x.to(dtype), w, t, norm_in=False, chunk_rows=chunk), ev.loss)
    normed = fn.plain_head_eval(x.to(dtype), w, t, norm_in=True, chunk_rows=chunk, group_rows=group)
    clear_status()
    assert torch.equal(normed.pred, pred) and torch.equal(normed.rank, rank) and normed.counts.tolist() == want


@pytest.mark.parametrize("dtype", BOTH)
def test_evaluation_rows_against_float64(dtype):
    x, w, t = small_inputs(seed=9)
    t[::6] = -100
    xin = x.to(dtype)
    ev = fn.plain_head_eval(xin, w, t, chunk_rows=32)
    xd, wd = xin.double(), w.to(dtype).double()
    c = (xd.square().mean(-1) + torch.finfo(torch.float32).eps).rsqrt()
    s = xd @ wd.T
    row_loss, pred, rank = pr.rows(s if dtype == torch.float32 else s.to(dtype), c, t)
    e = relerr(ev.row_loss, row_loss)
    print(f"{dtype}: row_loss against float64 {e:.3e}")
    assert e < (FP32_GRAD if dtype == torch.float32 else 2 ** -6)
    # a class is mistaken only where two stored products lie within the product's own rounding of each other
    top2 = s.topk(2, -1).values
    clear = (top2[:, 0] - top2[:, 1]) > (1e-4 if dtype == torch.float32 else 2 ** -6 * top2[:, 0].abs())
    assert clear.sum() > 50 and torch.equal(ev.pred[clear], pred[clear])
    with torch.no_grad():
        assert torch.equal(fn.plain_head_loss(xin, w, t, chunk_rows=32), ev.loss)
    assert ev.counts[0].item() == int((t != -100).sum())


# ---- 6. determinism
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("D, V, N", [(768, 50304, 70), (16, 65664, 37)])
def test_deterministic(D, V, N, dtype):
    g = torch.Generator(device=DEV).manual_seed(V)
    x = torch.randn(N, D, device=DEV, generator=g).to(dtype)
    w = torch.randn(V, D, device=DEV, generator=g) * D ** -0.5
    t = torch.randint(0, V, (N,), device=DEV, generator=g)
    t[::7] = -100
    a, b = fused(x, w, t, chunk_rows=32), fused(x, w, t, chunk_rows=32)
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["dx"], b["dx"])
    e = relerr(b["dW"], a["dW"])   # the order of the fp32 atomics is all that differs
    print(f"two runs, dW: {e:.3e}")
    assert e < FP32_GRAD


# ---- 7. hipGraph capture of forward + backward; the targets change in place between replays, and with them `kept`
@pytest.mark.parametrize("dtype", BOTH)
def test_hipgraph_replay_follows_the_kept_count(dtype):
    N, D, V = 96, 64, 640
    g = torch.Generator(device=DEV).manual_seed(11)
    x1, x2 = (torch.randn(N, D, device=DEV, generator=g).to(dtype) for _ in range(2))
    w = torch.randn(V, D, device=DEV, generator=g) * 0.5
    t1, t2 = (torch.randint(0, V, (N,), device=DEV, generator=g) for _ in range(2))
    t1[::2] = -100       # 48 kept
    t2[5::16] = -100     # 90 kept
    t3 = torch.full_like(t1, -100)
    xs, ws, ts = x1.clone().requires_grad_(True), w.clone().requires_grad_(True), t1.clone()

    def step():
        loss = fn.plain_head_loss(xs, ws, ts, chunk_rows=32)
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
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = step()
    for xn, tn in ((x2, t2), (x1, t1)):
        with torch.no_grad():
            xs.copy_(xn)
            ts.copy_(tn)
        graph.replay()
        torch.cuda.synchronize()
        ref = fused(xn, w, tn, chunk_rows=32)
        assert torch.equal(loss, ref["loss"]) and torch.equal(xs.grad, ref["dx"])
        assert relerr(ws.grad, ref["dW"]) < 1e-6
    with torch.no_grad():
        ts.copy_(t3)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.isnan(loss) and (xs.grad == 0).all() and (ws.grad == 0).all()


# ---- 8. autograd
def test_autograd_scaling_accumulation_and_retained_graph():
    x, w, t, _, _ = fixture_operands("math", 128)
    one = fused(x, w, t)
    xl, wl = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    (3.5 * fn.plain_head_loss(xl, wl, t)).backward()
    assert xl.grad.shape == x.shape and relerr(xl.grad, 3.5 * one["dx"]) < 1e-6 and relerr(wl.grad, 3.5 * one["dW"]) < 1e-6
    fn.plain_head_loss(xl, wl, t).backward()   # .grad accumulates
    assert relerr(xl.grad, 4.5 * one["dx"]) < 1e-6 and relerr(wl.grad, 4.5 * one["dW"]) < 1e-6
    xl.grad = wl.grad = None
    loss = fn.plain_head_loss(xl, wl, t)
    loss.backward(retain_graph=True)
    g1 = (xl.grad.clone(), wl.grad.clone())
    xl.grad = wl.grad = None
    (2 * loss).backward()
    assert torch.equal(g1[0], one["dx"]) and relerr(g1[1], one["dW"]) < 1e-6
    assert relerr(xl.grad, 2 * g1[0]) < 1e-6 and relerr(wl.grad, 2 * g1[1]) < 1e-6
    # no_grad and tensors that need no gradient: the loss alone, the same bits; one-sided gradients; int32 targets
    with torch.no_grad():
        assert torch.equal(fn.plain_head_loss(xl, wl, t), one["loss"])
    assert torch.equal(fn.plain_head_loss(x, w, t.int()), one["loss"])
    xo = x.clone().requires_grad_(True)
    fn.plain_head_loss(xo, w, t).backward()
    assert torch.equal(xo.grad, one["dx"])


@pytest.mark.parametrize("dtype", BOTH)
def test_tied_embedding_and_lm_head_receive_both_gradients(dtype):
    """wte.weight = lm_head.weight (mathblations/model.py:317): the one parameter gets the embedding's gradient and the head's."""
    V, D, Bq, Tq = 256, 32, 4, 16
    g = torch.Generator(device=DEV).manual_seed(21)
    lm_head = torch.nn.Linear(D, V, bias=False).to(DEV)
    wte = torch.nn.Embedding(V, D).to(DEV)
    wte.weight = lm_head.weight
    head = PlainLMHead(lm_head)
    assert [n for n, _ in head.named_parameters()] == ["lm_head.weight"]
    idx = torch.randint(0, V, (Bq, Tq), device=DEV, generator=g)
    y = torch.randint(0, V, (Bq, Tq), device=DEV, generator=g)
    t = mot.window_targets(y, [(3, 9), (0, 16), (15, 16), (7, 8)])
    body = lambda e: (e * 1.5 + 0.25).to(dtype)   # stands for the blocks
    loss = head.loss(body(wte(idx)), t)
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
    ev = head.evaluate(body(wte(idx)), t, group_rows=Tq)
    assert torch.equal(ev.loss, loss.detach()) and ev.counts.shape == (3,) and ev.counts[0].item() == 6 + 16 + 1 + 1


# ---- 9. memory: forward + backward at 4096 x 50 304 stay near workspace + dx + dW, far below the 786 MiB of fp32 logits
def test_peak_memory_far_below_the_logits():
    N, D, V = 4096, 768, 50304
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn(N, D, device=DEV, generator=g).requires_grad_(True)
    w = ((torch.rand(V, D, device=DEV, generator=g) * 2 - 1) * 0.03).requires_grad_(True)
    t = torch.randint(0, 50257, (N,), device=DEV, generator=g)
    t[::16] = -100
    d = capi.MotPlainHeadDesc()
    d.struct_size = C.sizeof(capi.MotPlainHeadDesc)
    d.dtype, d.norm_in, d.n_rows, d.model_dim, d.vocab, d.ignore_index, d.dx = capi.F32, 1, N, D, V, -100, 256
    ws = capi.lib.mot_plain_head_workspace_bytes(C.byref(d))
    fn.release_workspaces()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = fn.plain_head_loss(x, w, t)
    torch.cuda.synchronize()
    fwd = torch.cuda.max_memory_allocated() - base
    loss.backward()
    torch.cuda.synchronize()
    both = torch.cuda.max_memory_allocated() - base
    dx_b, dw_b, logits = N * D * 4, V * D * 4, N * V * 4
    mib = lambda b: f"{b / 2**20:.1f} MiB"
    print(f"peak extra memory: the call {mib(fwd)} (workspace {mib(ws)}, dx {mib(dx_b)}, dW {mib(dw_b)}), with backward {mib(both)}; "
          f"fp32 logits {mib(logits)}")
    assert ws < 2560 * (V + D) * 4 + (1 << 20)
    assert fwd < ws + dx_b + dw_b + (8 << 20)                     # the call: its workspace and the two gradients it keeps
    assert fwd < logits
    assert both < ws + 2 * (dx_b + dw_b) + (8 << 20)              # backward adds the scaled copies autograd hands on
    assert torch.isfinite(loss) and torch.isfinite(w.grad).all()
    fn.release_workspaces()
