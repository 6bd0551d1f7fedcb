"""The training path of the byte output head (functional.byte_head_loss -> mot_byte_head_fwd / mot_byte_head_bwd, csrc/mot_head.hip
with head_chain_rows, row_scale and the loss close of csrc/mot_headcore.*) where tests/test_gpu_byte_head.py does not reach:
1. a shape grid: bpt 1, 64 and odd ones, K 16 and 2048 and widths that are no multiple of 64, one row, row counts that are no
   multiple of 4, n_layer_out up to 4; 2. a chunk seam in every method x dtype; 3. targets out of range, whole rows of them and
   nothing else; 4. rows that are zero, tiny or huge.

The reference is tests/byte_head_ref.py in float64 on the device, on the values the kernel sees (x and W rounded to bf16 first in
bf16), always with eps = HEAD_EPS: the head's epsilon is fp32's 2^-23 in every dtype, float64's own 2.2e-16 is another function for
a row near zero.  Bars, as tests/test_gpu_byte_head.py sets them: fp32 loss 2e-6 and gradients 2e-5 of the largest float64
element; bf16 err <= 2 * own + 2^-12, `own` being the eager bf16 restatement's error on the same inputs.  Every figure is printed
before it is asserted (pytest -s shows them)."""
import pytest
import torch

import byte_head_ref as br
import mixture_of_tokenizers_amd as mot
from mixture_of_tokenizers_amd import _capi as capi
from mixture_of_tokenizers_amd import functional as fn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DTYPES = [torch.float32, torch.bfloat16]
FP32_LOSS, FP32_GRAD = 2e-6, 2e-5
KEYS = ("loss", "dx", "dW")
V = br.VOCAB
OOR = (-1, -100, V, 2 ** 40)


@pytest.fixture(autouse=True)
def status_left_clean():
    """A test that fails between a call with targets out of range and its check_status() leaves the bit to no later test."""
    yield
    try:
        mot.check_status()
    except IndexError:
        pass


def relerr(got, ref):
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    return float((got - ref).abs().max() / max(ref.abs().max().item(), 1e-300))


def row_relerr(got, ref, K):
    """The largest error of each row the head sees (K wide) over that row's own largest float64 element: the worst row's."""
    got, ref = got.detach().double().cpu().reshape(-1, K), ref.detach().double().cpu().reshape(-1, K)
    assert got.shape == ref.shape
    assert torch.isfinite(got).all(), f"non-finite rows: {(~torch.isfinite(got)).any(1).nonzero().flatten().tolist()}"
    return float(((got - ref).abs().max(1).values / ref.abs().max(1).values.clamp_min(1e-300)).max())


def width(method, D, bpt):
    return D if method == "copy" else D // bpt


def inputs(method, T, bpt, D, seed):
    """x [T, D] standard normal, W [512, K] with CastedLinear's bound, targets uniform over all 512 classes (the padded ones above
    457 too) with the first class first and the last class last."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    K = width(method, D, bpt)
    x = torch.randn(T, D, device=DEV, generator=g)
    w = (torch.rand(V, K, device=DEV, generator=g) * 2 - 1) * (3 ** 0.5) * 0.5 * K ** -0.5
    t = torch.randint(0, V, (T * bpt,), device=DEV, generator=g)
    t[0], t[-1] = 0, V - 1
    return x, w, t


def fused(x, w, t, method, bpt, L):
    xl = x.detach().clone().requires_grad_(True)
    wl = w.detach().clone().requires_grad_(True)
    loss = fn.byte_head_loss(xl, wl, t, method=method, bytes_per_token=bpt, n_layer_out=L)
    loss.backward()
    return {"loss": loss.detach(), "dx": xl.grad, "dW": wl.grad}


def check(what, x, w, t, method, bpt, L, dtype, dx_per_row=False):
    """The fused call on (x in dtype, fp32 w) against float64 with the head's epsilon on the values the kernel sees; targets out of
    range leave the reference's sum.  dx_per_row: dx is judged row by row, each against its own largest float64 element."""
    xin = x.to(dtype)
    got = fused(xin, w, t, method, bpt, L)
    assert got["dx"].dtype == dtype and got["dx"].shape == x.shape and got["dW"].dtype == torch.float32
    bad = ((t < 0) | (t >= V)).nonzero().flatten()
    drop = bad if bad.numel() else None
    ref = br.head(xin.double(), w.to(dtype).double(), t, method, bpt, L, torch.float64, drop=drop, eps=br.HEAD_EPS)
    K = w.shape[1]
    err = lambda a: {k: row_relerr(a[k], ref[k], K) if dx_per_row and k == "dx" else relerr(a[k], ref[k]) for k in KEYS}
    errs = err(got)
    tag = f"{what} {method} L {L} {'per-row dx ' if dx_per_row else ''}"
    if dtype == torch.float32:
        print(f"{tag}fp32: " + ", ".join(f"{k} {errs[k]:.3e}" for k in KEYS) + f"  (bars {FP32_LOSS:.0e} / {FP32_GRAD:.0e})")
        assert errs["loss"] < FP32_LOSS, errs
        assert errs["dx"] < FP32_GRAD and errs["dW"] < FP32_GRAD, errs
    else:
        own = err(br.head(xin, w, t, method, bpt, L, torch.bfloat16, drop=drop, eps=br.HEAD_EPS))
        print(f"{tag}bf16: " + ", ".join(f"{k} {errs[k]:.3e} (eager {own[k]:.3e})" for k in KEYS))
        for k in KEYS:
            assert errs[k] <= 2 * own[k] + 2 ** -12, f"{k}: {errs[k]:.3e} vs eager bf16 {own[k]:.3e}"
    return got, ref


def raised_and_cleared():
    """The status word carries the targets' bit; check_status() raises on it and clears it."""
    assert int(capi.status_word(DEV).item()) & capi.STATUS_TARGET_OOR
    with pytest.raises(IndexError, match="byte target"):
        mot.check_status()
    mot.check_status()


# ---- 1. the shape grid: (n_tokens, bpt, model_dim, n_layer_out); split has K = 16, 16, 16, 2048, 48, 80
GRID = {
    "copy": [(1, 1, 16, 0), (3, 3, 48, 1), (5, 64, 16, 2), (37, 5, 2048, 1), (257, 16, 80, 3), (63, 7, 768, 4)],
    "split": [(1, 1, 16, 0), (3, 3, 48, 1), (5, 64, 1024, 2), (37, 2, 4096, 1), (257, 16, 768, 3), (63, 5, 400, 4)],
}
GRID_CASES = [(m, *c) for m in ("copy", "split") for c in GRID[m]]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method, T, bpt, D, L", GRID_CASES)
def test_shape_grid(method, T, bpt, D, L, dtype):
    x, w, t = inputs(method, T, bpt, D, T + bpt + D + L)
    if method == "copy" and bpt >= 3:   # one token whose targets are one class (hist = bpt), one whose targets all differ
        t[bpt:2 * bpt] = 300
        t[-bpt:] = V - bpt + torch.arange(bpt, device=DEV)
        assert int(t[-1]) == V - 1
    what = f"grid T {T} bpt {bpt} D {D}"
    got, _ = check(what, x, w, t, method, bpt, L, dtype)
    ev = fn.byte_head_eval(x.to(dtype), w, t, method=method, bytes_per_token=bpt, n_layer_out=L)
    mean, loss = float(ev.row_loss.double().sum() / t.numel()), float(got["loss"])
    print(f"{what} {method} L {L} {dtype}: loss {loss:.7f}, the evaluation call's {float(ev.loss):.7f}, row_loss mean {mean:.7f}")
    assert torch.equal(ev.loss, got["loss"])
    assert abs(mean - loss) <= FP32_LOSS * abs(loss)
    mot.check_status()


# ---- 2. a chunk seam in every method x dtype: the widest row, K 2048, has the shortest chunk
def chunk_rows(rows, K, bf16):
    """The head's chunk rule restated (test_byte_head_refusals.py::test_workspace_query pins it at these shapes on the CPU)."""
    per_row = V * 4 + (V * 2 if bf16 else 0) + K * 4
    return min(rows, max(256, (48 << 20) // per_row // 256 * 256))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", ["copy", "split"])
def test_chunk_seam(method, dtype):
    bpt, K, L = 2, 2048, 1
    full = chunk_rows(1 << 40, K, dtype == torch.bfloat16)
    assert full == (4352 if dtype == torch.bfloat16 else 4864)
    T, D = (full + 37, K) if method == "copy" else ((full + 38) // 2, K * bpt)
    rows = T if method == "copy" else T * bpt
    chunk = chunk_rows(rows, K, dtype == torch.bfloat16)
    print(f"seam {method} {dtype}: {rows} rows in chunks of {chunk}")
    assert chunk == full and chunk < rows < 2 * chunk   # two chunks, the second of 37 or 38 rows
    x, w, t = inputs(method, T, bpt, D, 77)
    tpr = bpt if method == "copy" else 1
    t[(chunk - 1) * tpr + tpr - 1], t[chunk * tpr] = V, -1   # the last row of chunk 1 and the first of chunk 2 lose a target each
    mot.check_status()
    a, _ = check(f"seam T {T} bpt {bpt} D {D}", x, w, t, method, bpt, L, dtype)
    raised_and_cleared()
    b = fused(x.to(dtype), w, t, method, bpt, L)
    raised_and_cleared()
    e = relerr(b["dW"], a["dW"])   # the order of the fp32 atomics is all that differs
    print(f"seam {method} {dtype}: two runs, dW {e:.3e}")
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["dx"], b["dx"])
    assert e < FP32_GRAD


# ---- 3. targets outside [0, 512)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method, T, bpt, D, L", [("copy", *GRID["copy"][3]), ("split", *GRID["split"][4])])
def test_targets_out_of_range(method, T, bpt, D, L, dtype):
    x, w, t = inputs(method, T, bpt, D, 5 + T)
    K, M = w.shape[1], T * bpt
    at = torch.arange(3, M, max(M // 11, 1), device=DEV)[:8]   # spread over the rows, each value twice
    t[at] = torch.tensor(OOR * 2, device=DEV)[:at.numel()]
    gone = 2   # copy: a token that loses every target
    if method == "copy":
        t[gone * bpt:(gone + 1) * bpt] = torch.tensor((OOR * bpt)[:bpt], device=DEV)
    what = f"targets T {T} bpt {bpt} D {D}"
    mot.check_status()
    got, ref = check(what, x, w, t, method, bpt, L, dtype)
    raised_and_cleared()
    bad = (t < 0) | (t >= V)
    if method == "copy":
        # its dx row is zero, and dW does not see it: another row there moves dW by the order of its atomics alone
        assert (got["dx"][gone] == 0).all() and (ref["dx"][gone] == 0).all() and (got["dx"][gone + 1] != 0).any()
        x2 = x.clone()
        x2[gone] = 3 * x[gone].flip(0)
        e = relerr(fused(x2.to(dtype), w, t, method, bpt, L)["dW"], got["dW"])
        print(f"{what} {method} {dtype}: dW with another row at the token without targets {e:.3e}")
        assert e < FP32_GRAD
        raised_and_cleared()
    else:   # a byte row is one target: its K-wide slice of dx is zero
        dxr = got["dx"].reshape(-1, K)
        assert (dxr[bad] == 0).all() and (ref["dx"].reshape(-1, K)[bad] == 0).all() and (dxr[~bad] != 0).any(1).all()
    # the terms left the sum, the mean still divides by M: the reference's loss does (check above), as do the per-position losses
    ev = fn.byte_head_eval(x.to(dtype), w, t, method=method, bytes_per_token=bpt, n_layer_out=L)
    raised_and_cleared()
    mean, loss = float(ev.row_loss.double().sum() / M), float(got["loss"])
    print(f"{what} {method} {dtype}: loss {loss:.7f}, mean of row_loss over all {M} positions {mean:.7f}, {int(bad.sum())} dropped")
    assert (ev.row_loss.reshape(-1)[bad] == 0).all() and torch.equal(ev.loss, got["loss"])
    assert abs(mean - loss) <= FP32_LOSS * abs(loss)
    # nothing but targets out of range: every term and every gradient is exactly zero
    none = torch.tensor(OOR, device=DEV).repeat(M // 4 + 1)[:M]
    z = fused(x.to(dtype), w, none, method, bpt, L)
    raised_and_cleared()
    assert float(z["loss"]) == 0.0 and (z["dx"] == 0).all() and (z["dW"] == 0).all()


# ---- 4. rows that are zero, tiny or huge
SCALES = {1: 0.0, 2: 2.0 ** -20, 3: 2.0 ** 20, 4: 2.0 ** -60, 5: 2.0 ** 40}   # token -> factor; token 0 and the rest are ordinary


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("method, bpt, D", [("copy", 3, 48), ("split", 4, 64)])
def test_extreme_rows(method, bpt, D, L, dtype):
    T = 12
    x, w, t = inputs(method, T, bpt, D, 90 + L)
    for tok, s in SCALES.items():
        x[tok] *= s
    if method == "split":
        x[6, :D // bpt] = 0   # one zero byte row among a token's ordinary ones
    # the rows' gradients span 30 orders of magnitude, so dx is judged per row; loss and dW as everywhere
    check(f"extreme rows bpt {bpt} D {D}", x, w, t, method, bpt, L, dtype, dx_per_row=True)
    mot.check_status()
