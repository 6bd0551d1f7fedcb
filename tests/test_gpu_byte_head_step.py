"""mot_byte_head_step (functional.byte_head_loss(one_call=True), csrc/mot_headstep.hip): the split-mode byte head's loss, dx and dW
from one fused call, in float32 and bfloat16.

The reference is tests/byte_head_ref.py in float64 on the device, on the values the kernel sees (x and W rounded to bf16 first in
bf16), always with eps = HEAD_EPS.  The bars are the project's own, as tests/test_gpu_byte_head.py and test_gpu_byte_head_edges.py
set them: fp32 loss 2e-6 and gradients 2e-5 of the largest float64 element; bf16 err <= 2 * own + 2^-12, `own` being the eager bf16
restatement's error on the same inputs.
dW takes route (a) of the design (the kernel stores G per chunk, the shared product adds it into dW with fp32 atomics), so between
two runs dW is held to the fp32 gradient bar 2e-5, as test_chunk_seam does there; loss and dx have the same bits on every run.
Every figure is printed before it is asserted (pytest -s shows them).

The unit's constants, restated: a tile is 256 byte rows (8 waves of 32), the grid is min(tiles, 256) persistent workgroups that take
tiles blockIdx, blockIdx + 256, ..., and G is kept for chunks of 131 072 rows (one launch each)."""
from pathlib import Path

import numpy as np
import pytest
import torch

import byte_head_ref as br
import mixture_of_tokenizers_amd as mot
from mixture_of_tokenizers_amd import _capi as capi
from mixture_of_tokenizers_amd import functional as fn
from mixture_of_tokenizers_amd.modules import ByteHyperparameters, ByteMixout, CastedLinear, ModelDims

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BF = torch.bfloat16
GOLDEN = np.load(Path(__file__).parent / "golden" / "byte_head.npz")
FP32_LOSS, FP32_GRAD = 2e-6, 2e-5
DTYPES = [torch.float32, BF]
KEYS = ("loss", "dx", "dW")
V = br.VOCAB
OOR = (-1, -100, V, 2 ** 40)
TILE_ROWS, GRID_WGS, CHUNK_ROWS = 256, 256, 131072


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
    """The largest error of each byte row (K wide) over that row's own largest float64 element: the worst row's."""
    got, ref = got.detach().double().cpu().reshape(-1, K), ref.detach().double().cpu().reshape(-1, K)
    assert got.shape == ref.shape
    assert torch.isfinite(got).all(), f"non-finite rows: {(~torch.isfinite(got)).any(1).nonzero().flatten().tolist()}"
    return float(((got - ref).abs().max(1).values / ref.abs().max(1).values.clamp_min(1e-300)).max())


def inputs(T, bpt, K, seed, dtype=BF):
    """x [T, K * bpt] standard normal in dtype, W [512, K] fp32 with CastedLinear's bound, targets uniform over all 512 classes with
    the first class first and the last class last."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(T, K * bpt, device=DEV, generator=g).to(dtype)
    w = (torch.rand(V, K, device=DEV, generator=g) * 2 - 1) * (3 ** 0.5) * 0.5 * K ** -0.5
    t = torch.randint(0, V, (T * bpt,), device=DEV, generator=g)
    t[0], t[-1] = 0, V - 1
    return x, w, t


def fused(x, w, t, bpt, L, one_call=True):
    xl = x.detach().clone().requires_grad_(True)
    wl = w.detach().clone().requires_grad_(True)
    loss = fn.byte_head_loss(xl, wl, t, method="split", bytes_per_token=bpt, n_layer_out=L, one_call=one_call)
    loss.backward()
    return {"loss": loss.detach(), "dx": xl.grad, "dW": wl.grad}


def reference(x, w, t, bpt, L):
    """float64 on the values the kernel sees, and in bf16 the eager bf16 restatement; targets out of range leave both sums."""
    bad = ((t < 0) | (t >= V)).nonzero().flatten()
    drop = bad if bad.numel() else None
    ref = br.head(x.double(), w.to(x.dtype).double(), t, "split", bpt, L, torch.float64, drop=drop, eps=br.HEAD_EPS)
    own = br.head(x, w, t, "split", bpt, L, BF, drop=drop, eps=br.HEAD_EPS) if x.dtype == BF else None
    return ref, own


def judge(tag, got, ref, own, K, dx_per_row=False):
    """Prints every figure, asserts the dtype's bars and returns them (own None: the fp32 bars)."""
    err = lambda a: {k: row_relerr(a[k], ref[k], K) if dx_per_row and k == "dx" else relerr(a[k], ref[k]) for k in KEYS}
    errs = err(got)
    if own is None:
        bars = {"loss": FP32_LOSS, "dx": FP32_GRAD, "dW": FP32_GRAD}
        print(f"{tag}{' per-row dx' if dx_per_row else ''} fp32: " + ", ".join(f"{k} {errs[k]:.3e}" for k in KEYS) + f"  (bars {FP32_LOSS:.0e} / {FP32_GRAD:.0e})")
        for k in KEYS:
            assert errs[k] < bars[k], f"{k}: {errs[k]:.3e}"
        return bars
    owns = err(own)
    print(f"{tag}{' per-row dx' if dx_per_row else ''} bf16: " + ", ".join(f"{k} {errs[k]:.3e} (eager {owns[k]:.3e})" for k in KEYS))
    for k in KEYS:
        assert errs[k] <= 2 * owns[k] + 2 ** -12, f"{k}: {errs[k]:.3e} vs eager bf16 {owns[k]:.3e}"
    return {k: 2 * owns[k] + 2 ** -12 for k in KEYS}


def check(tag, x, w, t, bpt, L, dx_per_row=False):
    got = fused(x, w, t, bpt, L)
    assert got["dx"].dtype == x.dtype and got["dx"].shape == x.shape and got["dW"].dtype == torch.float32 and got["dW"].shape == w.shape
    ref, own = reference(x, w, t, bpt, L)
    bars = judge(tag, got, ref, own, w.shape[1], dx_per_row)
    return got, ref, bars


def raised_and_cleared():
    """The status word carries the targets' bit; check_status() raises on it and clears it."""
    assert int(capi.status_word(DEV).item()) & capi.STATUS_TARGET_OOR
    with pytest.raises(IndexError, match="byte target"):
        mot.check_status()
    mot.check_status()


# ---- the reference's own fixture: the three split cases (D 128, bpt 8, K 16)
@pytest.mark.parametrize("L", br.LAYERS)
def test_fixture_fp32(L):
    x, w, t = br.case_inputs("split", L)
    got = fused(x.to(DEV), w.to(DEV), t.to(DEV), br.BPT, L)
    ref = {k: torch.from_numpy(np.asarray(GOLDEN[br.case_key("split", L, "f64", k)])) for k in KEYS}   # the reference's own float64 run
    judge(f"fixture L {L}", got, ref, None, 16)


@pytest.mark.parametrize("L", br.LAYERS)
def test_fixture_bf16(L):
    x, w, t = br.case_inputs("split", L)
    xb = x.to(BF)
    ref = br.head(xb.double(), w.to(BF).double(), t, "split", br.BPT, L, torch.float64, eps=br.HEAD_EPS)   # the same bf16-valued inputs
    eager = {k: torch.from_numpy(np.asarray(GOLDEN[br.case_key("split", L, "bf16", k)])) for k in KEYS}   # the reference's own bf16 run
    got = fused(xb.to(DEV), w.to(DEV), t.to(DEV), br.BPT, L)
    assert got["dx"].dtype == BF and got["dW"].dtype == torch.float32
    judge(f"fixture L {L}", got, ref, eager, 16)


# ---- the shape grid: (n_tokens, bpt, K, n_layer_out): one row, fewer rows than a wave's 32, row counts that are no multiple of 32
# or of the 256-row tile, every K step of 16 that takes another instantiation among 16 .. 128 (W's second image in LDS up to 64,
# read through L2 above), every n_layer_out 0 .. 4
GRID_BF16 = [(1, 1, 16, 0), (1, 16, 64, 1), (3, 3, 48, 1), (3, 2, 128, 2), (5, 5, 80, 2), (5, 7, 16, 3), (37, 2, 64, 4), (37, 16, 48, 0),
        (37, 1, 128, 1), (257, 16, 64, 1), (257, 3, 16, 4), (257, 7, 80, 3), (257, 5, 128, 0), (5, 16, 128, 4), (3, 7, 64, 3),
        (1, 2, 80, 1), (37, 3, 48, 2), (257, 1, 48, 3), (5, 1, 64, 0), (1, 5, 16, 2), (37, 5, 32, 1), (3, 16, 96, 2), (5, 3, 112, 0)]
GRID_FP32 = [(1, 1, 16, 0), (1, 16, 64, 1), (3, 3, 48, 1), (3, 2, 64, 2), (5, 5, 32, 2), (5, 7, 16, 3), (37, 2, 64, 4), (37, 16, 48, 0),
             (37, 1, 16, 1), (257, 16, 64, 1), (257, 3, 16, 4), (257, 7, 48, 3), (257, 5, 64, 0), (5, 16, 32, 4), (3, 7, 64, 3),
             (1, 2, 48, 1), (37, 3, 32, 2), (257, 1, 48, 3), (5, 1, 64, 0), (1, 5, 16, 2)]
GRID = [(torch.float32, *c) for c in GRID_FP32] + [(BF, *c) for c in GRID_BF16]


@pytest.mark.parametrize("dtype, T, bpt, K, L", GRID)
def test_shape_grid(dtype, T, bpt, K, L):
    x, w, t = inputs(T, bpt, K, T + bpt + K + L, dtype)
    check(f"grid T {T} bpt {bpt} K {K} L {L}", x, w, t, bpt, L)
    mot.check_status()


# ---- the walk of a persistent workgroup
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [CHUNK_ROWS + TILE_ROWS + 37, 3 * TILE_ROWS + 5])
def test_tile_seam(rows, dtype):
    """The long shape: its first chunk is 512 tiles, two for each of the 256 workgroups; the second chunk is a launch of its own at a
    row offset, one whole tile and one of 37 rows.  The short one: 4 tiles, fewer than workgroups, the last of 5 rows."""
    K, L = 16, 1
    tiles = [-(-min(CHUNK_ROWS, rows - r0) // TILE_ROWS) for r0 in range(0, rows, CHUNK_ROWS)]
    print(f"seam {rows} rows: tiles per launch {tiles}")
    assert tiles == ([2 * GRID_WGS, 2] if rows > CHUNK_ROWS else [4]) and rows % TILE_ROWS
    x, w, t = inputs(rows, 1, K, 77, dtype)
    # a dropped target in the last row of one tile and the first of the next: inside a workgroup's walk, and across the chunks
    seams = [TILE_ROWS, GRID_WGS * TILE_ROWS, CHUNK_ROWS, CHUNK_ROWS + TILE_ROWS] if rows > CHUNK_ROWS else [TILE_ROWS, 3 * TILE_ROWS]
    for s in seams:
        t[s - 1], t[s] = V, -1
    mot.check_status()
    a, ref, _ = check(f"seam rows {rows}", x, w, t, 1, L)
    raised_and_cleared()
    bad = (t < 0) | (t >= V)
    assert int(bad.sum()) == 2 * len(seams)
    assert (a["dx"][bad] == 0).all() and (ref["dx"][bad] == 0).all() and (a["dx"][~bad] != 0).any(1).all()
    b = fused(x, w, t, 1, L)
    raised_and_cleared()
    e = relerr(b["dW"], a["dW"])   # the order of the fp32 atomics is all that differs
    print(f"seam rows {rows}: two runs, dW {e:.3e}")
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["dx"], b["dx"])
    assert e < FP32_GRAD


# ---- targets: the edges of the range and what lies outside it
@pytest.mark.parametrize("dtype", DTYPES)
def test_targets(dtype):
    T, bpt, K, L = 37, 7, 48, 2
    x, w, t = inputs(T, bpt, K, 5, dtype)
    M = T * bpt
    at = torch.arange(3, M, M // 13, device=DEV)[:12]   # spread over the rows: 0, 511 and each value out of range, twice
    t[at] = torch.tensor((0, V - 1) * 2 + OOR * 2, device=DEV)
    mot.check_status()
    got, ref, _ = check(f"targets T {T} bpt {bpt} K {K}", x, w, t, bpt, L)
    raised_and_cleared()
    bad = (t < 0) | (t >= V)
    assert int(bad.sum()) == 8
    dxr = got["dx"].reshape(-1, K)
    assert (dxr[bad] == 0).all() and (ref["dx"].reshape(-1, K)[bad] == 0).all() and (dxr[~bad] != 0).any(1).all()
    with torch.no_grad():   # the loss alone raises the bit too, and has the same bits
        alone = fn.byte_head_loss(x, w, t, method="split", bytes_per_token=bpt, n_layer_out=L, one_call=True)
    raised_and_cleared()
    assert torch.equal(alone, got["loss"])
    check("targets in range", x, w, t.clamp(0, V - 1), bpt, L)
    mot.check_status()                                   # nothing raised
    none = torch.tensor(OOR, device=DEV).repeat(M // 4 + 1)[:M]   # nothing but targets out of range: everything is exactly zero
    z = fused(x, w, none, bpt, L)
    raised_and_cleared()
    assert float(z["loss"]) == 0.0 and (z["dx"] == 0).all() and (z["dW"] == 0).all()


# ---- rows that are zero, tiny or huge
SCALES = {1: 0.0, 2: 2.0 ** -20, 3: 2.0 ** 20, 4: 2.0 ** -60, 5: 2.0 ** 40}   # token -> factor; token 0 and the rest are ordinary


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [0, 1, 2, 3, 4])
def test_extreme_rows(L, dtype):
    T, bpt, K = 12, 4, 16
    x, w, t = inputs(T, bpt, K, 90 + L, dtype)
    x = x.float()
    for tok, s in SCALES.items():
        x[tok] *= s
    x[6, :K] = 0   # one zero byte row among a token's ordinary ones
    # the rows' gradients span 30 orders of magnitude, so dx is judged per row; loss and dW as everywhere
    got, _, _ = check(f"extreme rows L {L}", x.to(dtype), w, t, bpt, L, dx_per_row=True)
    assert torch.isfinite(got["dx"]).all() and torch.isfinite(got["dW"]).all()
    mot.check_status()


# ---- the two-call path on the same inputs: within the sum of the two bars, not in bits
@pytest.mark.parametrize("dtype, T, bpt, K, L", [(BF, 257, 16, 64, 1), (BF, 37, 5, 128, 2), (torch.float32, 257, 16, 64, 1), (torch.float32, 37, 5, 48, 2)])
def test_agrees_with_the_two_call_path(dtype, T, bpt, K, L):
    x, w, t = inputs(T, bpt, K, 31, dtype)
    one, ref, bars = check(f"one call T {T} bpt {bpt} K {K}", x, w, t, bpt, L)
    two = fused(x, w, t, bpt, L, one_call=False)
    for k in KEYS:
        scale = max(ref[k].abs().max().item(), 1e-300)
        e = float((one[k].double() - two[k].double()).abs().max()) / scale
        print(f"one call vs two calls T {T} K {K}: {k} {e:.3e} (sum of the bars {2 * bars[k]:.3e})")
        assert e <= 2 * bars[k]


# ---- the same inputs twice; the loss alone
@pytest.mark.parametrize("dtype, T, bpt, K", [(BF, 1024, 16, 64), (BF, 300, 3, 128), (torch.float32, 1024, 16, 64), (torch.float32, 300, 3, 48)])
def test_same_inputs_same_bits(dtype, T, bpt, K):
    x, w, t = inputs(T, bpt, K, 9, dtype)
    a, b = fused(x, w, t, bpt, 1), fused(x, w, t, bpt, 1)
    e = relerr(b["dW"], a["dW"])
    print(f"two runs T {T} bpt {bpt} K {K}: dW {e:.3e}")
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["dx"], b["dx"])
    assert e < FP32_GRAD   # route (a): dW sums with fp32 atomics, held to the bar in both runs
    with torch.no_grad():
        alone = fn.byte_head_loss(x, w, t, method="split", bytes_per_token=bpt, n_layer_out=1, one_call=True)
    detached = fn.byte_head_loss(x.detach(), w.detach(), t, method="split", bytes_per_token=bpt, n_layer_out=1, one_call=True)
    assert not alone.requires_grad and not detached.requires_grad
    assert torch.equal(alone, a["loss"]) and torch.equal(detached, a["loss"])


# ---- autograd
@pytest.mark.parametrize("dtype", DTYPES)
def test_autograd_scales_accumulates_and_runs_twice(dtype):
    """dx is rounded once more where a product or a sum is stored in x's dtype: half an ulp, 2^-9 in bf16 and 2^-24 in fp32, of the
    element, so at most that of the largest; twice that is the bar."""
    T, bpt, K, L = 37, 16, 64, 1
    x, w, t = inputs(T, bpt, K, 3, dtype)
    ulp = 2 ** -8 if dtype == BF else 2 ** -23
    kw = dict(method="split", bytes_per_token=bpt, n_layer_out=L, one_call=True)
    base = fused(x, w, t, bpt, L)
    xl, wl = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    (3 * fn.byte_head_loss(xl, wl, t, **kw)).backward()
    ex, ew = relerr(xl.grad, 3 * base["dx"].float()), relerr(wl.grad, 3 * base["dW"])
    print(f"autograd {dtype}: 3 * loss: dx {ex:.3e} (one rounding), dW {ew:.3e}")
    assert ex <= ulp and ew < FP32_GRAD
    # into an existing .grad
    before = (xl.grad.clone(), wl.grad.clone())
    fn.byte_head_loss(xl, wl, t, **kw).backward()
    ex, ew = relerr(xl.grad, before[0].float() + base["dx"].float()), relerr(wl.grad, before[1] + base["dW"])
    print(f"autograd {dtype}: accumulated: dx {ex:.3e}, dW {ew:.3e}")
    assert ex <= ulp and ew < FP32_GRAD
    # a retained graph runs backward twice on the same saved gradients
    xl.grad = wl.grad = None
    loss = fn.byte_head_loss(xl, wl, t, **kw)
    loss.backward(retain_graph=True)
    once = (xl.grad.clone(), wl.grad.clone())
    loss.backward()
    assert torch.equal(xl.grad, (2 * once[0].float()).to(dtype)) and torch.equal(wl.grad, 2 * once[1])
    assert torch.equal(once[0], base["dx"]) and relerr(once[1], base["dW"]) < FP32_GRAD
    # one input alone
    xo = x.clone().requires_grad_(True)
    fn.byte_head_loss(xo, w, t, **kw).backward()
    assert torch.equal(xo.grad, base["dx"])


@pytest.mark.parametrize("xdtype", DTYPES)
@pytest.mark.parametrize("wdtype", [torch.float32, BF])
def test_weight_gradient_in_the_weights_dtype(wdtype, xdtype):
    x, w, t = br.case_inputs("split", 1)
    lm = CastedLinear(w.shape[1], 512).to(DEV)
    with torch.no_grad():
        lm.weight.copy_(w)
    lm.to(wdtype)
    xl = x.to(DEV).to(xdtype).requires_grad_(True)
    fn.byte_head_loss(xl, lm.weight, t.to(DEV), method="split", bytes_per_token=br.BPT, n_layer_out=1, one_call=True).backward()
    assert lm.weight.grad.dtype == wdtype and xl.grad.dtype == xdtype and torch.isfinite(lm.weight.grad).all()
    base = fused(xl.detach(), lm.weight.detach().float(), t.to(DEV), br.BPT, 1)   # the weight's values as the module holds them
    assert relerr(lm.weight.grad, base["dW"]) <= (2 ** -8 if wdtype == BF else FP32_GRAD)


def test_module_loss_one_call():
    D, bpt = 256, 16
    m = ByteMixout(ModelDims(model_dim=D), 512, ByteHyperparameters(bytes_per_token=bpt, byte_mixout_method="split", n_layer_out=1)).to(DEV)
    x, w, t = inputs(2 * 512, bpt, D // bpt, 21)
    lm = CastedLinear(D // bpt, 512).to(DEV)
    with torch.no_grad():
        lm.weight.copy_(w)
        a = m.loss(x.reshape(2, 512, D), lm, t.reshape(2, -1), one_call=True)
        b = fn.byte_head_loss(x, w, t, method="split", bytes_per_token=bpt, n_layer_out=1, one_call=True)
    assert torch.equal(a, b)


# ---- no_grad keeps nothing
@pytest.mark.parametrize("dtype", DTYPES)
def test_no_grad_allocates_neither_dx_nor_dw(dtype):
    T, bpt, K = 8 * 1024, 16, 64
    x, w, t = inputs(T, bpt, K, 3, dtype)
    wb = w.to(dtype)   # the cast is the caller's here: nothing of the weight's size is made by the call
    kw = dict(method="split", bytes_per_token=bpt, n_layer_out=1, one_call=True)
    with torch.no_grad():
        fn.byte_head_loss(x, wb, t, **kw)   # the workspace is the package's, kept between calls
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        loss = fn.byte_head_loss(x, wb, t, **kw)
        torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    print(f"no_grad: {extra} bytes beyond the inputs (dW would be {V * K * 4}, dx {x.numel() * x.element_size()})")
    assert extra < V * K * 4 and torch.isfinite(loss)


# ---- hipGraph
@pytest.mark.parametrize("dtype", DTYPES)
def test_hipgraph_capture_and_replay(dtype):
    T, bpt, K, L = 2 * 256, 16, 64, 1
    x1, w, t1 = inputs(T, bpt, K, 11, dtype)
    x2, _, t2 = inputs(T, bpt, K, 12, dtype)
    xs, ws, ts = x1.clone().requires_grad_(True), w.clone().requires_grad_(True), t1.clone()
    kw = dict(method="split", bytes_per_token=bpt, n_layer_out=L, one_call=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            xs.grad = ws.grad = None
            fn.byte_head_loss(xs, ws, ts, **kw).backward()
    torch.cuda.current_stream().wait_stream(s)
    xs.grad = ws.grad = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loss = fn.byte_head_loss(xs, ws, ts, **kw)
        loss.backward()
    with torch.no_grad():
        xs.copy_(x2)
        ts.copy_(t2)
    g.replay()
    torch.cuda.synchronize()
    ref = fused(x2, w, t2, bpt, L)
    e = relerr(ws.grad, ref["dW"])
    print(f"hipGraph replay vs eager: dW {e:.3e}")
    assert torch.equal(loss, ref["loss"]) and torch.equal(xs.grad, ref["dx"])
    assert e < FP32_GRAD
