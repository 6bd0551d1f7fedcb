"""The fused token-level output head (functional.token_head_loss / ByteMixout(noop).loss, csrc/mot_tokhead.hip) against float64 on
the device: the reference's fixture cases, the real width of 50 304 classes, both softcaps in their curved part, shape edges and
every path of the row pass, out-of-range targets, determinism, hipGraph capture, no_grad, autograd and peak memory.

Bars, as tests/test_gpu_byte_head.py sets them: fp32 loss 2e-6 and gradients 2e-5 of the largest float64 element; bf16
err <= 2 * own + 2^-12, `own` being the eager bf16 restatement's error against float64 on the same bf16-valued inputs.  Every
figure is printed before it is asserted (pytest -s shows them)."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

import mixture_of_tokenizers_amd as mot
import token_head_ref as tr
from mixture_of_tokenizers_amd import _capi as capi
from mixture_of_tokenizers_amd import functional as fn
from mixture_of_tokenizers_amd.modules import ByteHyperparameters, ByteMixout, CastedLinear, ModelDims

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GOLDEN = np.load(Path(__file__).parent / "golden" / "token_head.npz")
FP32_LOSS, FP32_GRAD = 2e-6, 2e-5
KEYS = ("loss", "dx", "dW")
V_REAL, D_REAL, N_REAL = 50304, 768, 300


def relerr(got, ref):
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    return float((got - ref).abs().max() / max(ref.abs().max().item(), 1e-300))


def fused(x, w, t, kind, norm_in=True, chunk_rows=None):
    xl = x.detach().clone().requires_grad_(True)
    wl = w.detach().clone().requires_grad_(True)
    loss = fn.token_head_loss(xl, wl, t, softcap=kind, norm_in=norm_in, chunk_rows=chunk_rows)
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


def check(what, x, w, t, kind, dtype, norm_in=True, chunk_rows=None, eager=None, drop=None):
    """The fused call on (x in dtype, fp32 w) against float64 on the values the kernel sees."""
    xin = x.to(dtype)
    got = fused(xin, w, t, kind, norm_in, chunk_rows)
    assert got["dx"].dtype == dtype and got["dW"].dtype == torch.float32
    if dtype == torch.float32:
        check_fp32(what, got, tr.head(x, w, t, kind, norm_in, torch.float64, drop=drop))
    else:
        ref = tr.head(xin.double(), w.to(dtype).double(), t, kind, norm_in, torch.float64, drop=drop)
        check_bf16(what, got, ref, eager if eager is not None else tr.head(xin, w, t, kind, norm_in, torch.bfloat16, drop=drop))
    return got


# ---- 1. the fixture cases: the reference's own float64 and bf16 outputs
@pytest.mark.parametrize("norm_in", [True, False])
@pytest.mark.parametrize("kind", tr.SOFTCAPS)
def test_fixture_fp32(kind, norm_in):
    x, w, t = tr.case_inputs(kind, norm_in)
    got = fused(x.to(DEV), w.to(DEV), t.to(DEV), kind, norm_in)
    ref = {k: torch.from_numpy(np.asarray(GOLDEN[tr.case_key(kind, norm_in, "f64", k)])) for k in KEYS}
    check_fp32(f"fixture {kind} norm {norm_in}", got, ref)


@pytest.mark.parametrize("norm_in", [True, False])
@pytest.mark.parametrize("kind", tr.SOFTCAPS)
def test_fixture_bf16(kind, norm_in):
    x, w, t = tr.case_inputs(kind, norm_in)
    eager = None   # without the norm the reference has no run of its own: the eager restatement on the device stands in
    if norm_in:
        eager = {k: torch.from_numpy(np.asarray(GOLDEN[tr.case_key(kind, True, "bf16", k)])) for k in KEYS}
    check(f"fixture {kind} norm {norm_in}", x.to(DEV), w.to(DEV), t.to(DEV), kind, torch.bfloat16, norm_in, eager=eager)


# ---- 2, 3. the real width
_real = {}


def real_inputs(scale):
    """x [300, 768], W [50304, 768] at CastedLinear's init (scale None: std(l) 0.5) or scaled to std(l) = `scale`; targets with the
    first class, the last real one, the last padded one and repeats."""
    if scale not in _real:
        g = torch.Generator(device=DEV).manual_seed(7)
        x = torch.randn(N_REAL, D_REAL, device=DEV, generator=g)
        std = 0.5 * D_REAL ** -0.5 if scale is None else scale * D_REAL ** -0.5
        w = (torch.rand(V_REAL, D_REAL, device=DEV, generator=g) * 2 - 1) * (3 ** 0.5) * std
        t = torch.randint(0, 50257, (N_REAL,), device=DEV, generator=g)
        t[:8] = torch.tensor([0, 50256, 50303, 50303, 0, 17, 17, 50257], device=DEV)
        t[128], t[255], t[256], t[299] = 50303, 0, 50256, 50303   # the ends of the chunks of 128, 128, 44
        _real[scale] = (x, w, t)
    return _real[scale]


@pytest.mark.parametrize("chunk_rows", [128, None])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", tr.SOFTCAPS)
def test_real_width(kind, dtype, chunk_rows):
    x, w, t = real_inputs(None)
    check(f"50304 x 768 x 300 {kind} chunk {chunk_rows}", x, w, t, kind, dtype, chunk_rows=chunk_rows)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", tr.SOFTCAPS)
def test_curved_part_of_the_softcaps(kind, dtype):
    x, w, t = real_inputs(10.0)
    l = torch.nn.functional.rms_norm(x[:32], (D_REAL,)) @ w.T
    assert 9 < l.std().item() < 11
    check(f"std(l) 10 {kind}", x, w, t, kind, dtype, chunk_rows=128)


# ---- 4. edges: the sizes the issue names, and every path of the row pass (workgroups of 256 and 1024 threads; 4, 8 and 16 vectors a
# thread in registers; rows above 65 536 classes, read twice)
EDGES = [  # (D, V, N)
    (16, 128, 1), (48, 640, 63), (1024, 128, 257), (2048, 640, 257), (16, 50304, 63), (2048, 50304, 1), (1024, 640, 1),
    (16, 8192, 3), (16, 32768, 3), (16, 65536, 3), (16, 131072, 3), (48, 262144, 2),
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("D, V, N", EDGES)
def test_edges(D, V, N, dtype):
    kind = tr.SOFTCAPS[(D + V // 128 + N) % 2]
    g = torch.Generator(device=DEV).manual_seed(D + V + N)
    x = torch.randn(N, D, device=DEV, generator=g)
    w = (torch.rand(V, D, device=DEV, generator=g) * 2 - 1) * (3 ** 0.5) * 4.0 * D ** -0.5   # std(l) 4
    t = torch.randint(0, V, (N,), device=DEV, generator=g)
    t[0], t[-1] = V - 1, 0 if N > 1 else V - 1
    check(f"D {D} V {V} N {N} {kind}", x, w, t, kind, dtype, norm_in=bool((D // 16 + N) % 2) or V > 50304)


# ---- 5. targets outside [0, V)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", tr.SOFTCAPS)
def test_out_of_range_targets(kind, dtype):
    x, w, t = (a.to(DEV) for a in tr.case_inputs(kind, True))
    t = t.clone()
    t[5], t[17] = -100, tr.VOCAB
    mot.check_status()
    t_ok = t.clone()
    t_ok[5] = t_ok[17] = 0
    xin = x.to(dtype)
    got = fused(xin, w, t, kind)
    assert int(capi.status_word(DEV).item()) & capi.STATUS_TARGET_OOR
    with pytest.raises(IndexError, match="target"):
        mot.check_status()
    assert (got["dx"][5] == 0).all() and (got["dx"][17] == 0).all() and (got["dx"][6] != 0).any()
    wv = w if dtype == torch.float32 else w.to(dtype).float()
    ref = tr.head(xin.double(), wv.double(), t_ok, kind, True, torch.float64, drop=[5, 17])
    assert (ref["dx"][5] == 0).all()
    if dtype == torch.float32:
        check_fp32(f"dropped rows {kind}", got, ref)
    else:
        check_bf16(f"dropped rows {kind}", got, ref, tr.head(xin, w, t_ok, kind, True, torch.bfloat16, drop=[5, 17]))


# ---- 6. determinism
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_deterministic_and_chunking_agrees(dtype):
    x, w, t = real_inputs(None)
    xin = x.to(dtype)
    a = fused(xin, w, t, "sigmoid30", chunk_rows=128)
    b = fused(xin, w, t, "sigmoid30", chunk_rows=128)
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["dx"], b["dx"])
    e = relerr(b["dW"], a["dW"])   # the order of the fp32 atomics is all that differs
    print(f"two runs, dW: {e:.3e}")
    assert e < FP32_GRAD
    # other chunkings (5 chunks, 2 chunks, one): the launchers take other routes, so bits may differ; each stays within the bar
    if dtype == torch.float32:
        ref = tr.head(x, w, t, "sigmoid30", True, torch.float64)
    else:
        ref = tr.head(xin.double(), w.to(dtype).double(), t, "sigmoid30", True, torch.float64)
        eager = tr.head(xin, w, t, "sigmoid30", True, torch.bfloat16)
    for chunk in (64, 160, None):
        c = fused(xin, w, t, "sigmoid30", chunk_rows=chunk)
        if dtype == torch.float32:
            check_fp32(f"chunk_rows {chunk}", c, ref)
        else:
            check_bf16(f"chunk_rows {chunk}", c, ref, eager)
        assert relerr(c["loss"], a["loss"]) < FP32_LOSS


# ---- 7. hipGraph capture of forward + backward, replayed on new inputs
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", tr.SOFTCAPS)
def test_hipgraph_capture_and_replay(kind, dtype):
    N, D, V = 96, 64, 640
    g = torch.Generator(device=DEV).manual_seed(11)
    x1, x2 = (torch.randn(N, D, device=DEV, generator=g).to(dtype) for _ in range(2))
    w = torch.randn(V, D, device=DEV, generator=g) * 0.5
    t1, t2 = (torch.randint(0, V, (N,), device=DEV, generator=g) for _ in range(2))
    xs, ws, ts = x1.clone().requires_grad_(True), w.clone().requires_grad_(True), t1.clone()

    def step():
        loss = fn.token_head_loss(xs, ws, ts, softcap=kind, chunk_rows=32)
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
    with torch.no_grad():
        xs.copy_(x2)
        ts.copy_(t2)
    graph.replay()
    torch.cuda.synchronize()
    ref = fused(x2, w, t2, kind, chunk_rows=32)
    assert torch.equal(loss, ref["loss"]) and torch.equal(xs.grad, ref["dx"])
    assert relerr(ws.grad, ref["dW"]) < 1e-6


# ---- 8. no_grad: the loss alone
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_no_grad_same_bits_and_no_gradient_sized_buffer(dtype):
    x, w, t = real_inputs(None)
    xin = x.to(dtype)
    with_grad = fused(xin, w, t, "rsqrt15")["loss"]
    xl, wl = xin.clone().requires_grad_(True), w.clone().requires_grad_(True)
    fn.release_workspaces()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with torch.no_grad():
        loss = fn.token_head_loss(xl, wl, t, softcap="rsqrt15")
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    assert not loss.requires_grad and torch.equal(loss, with_grad)
    dw_bytes = V_REAL * D_REAL * 4
    print(f"no_grad peak extra {extra / 2**20:.1f} MiB (the logits of one chunk, in bf16 the cast weight); dW would be {dw_bytes / 2**20:.1f} MiB")
    assert extra < dw_bytes
    # tensors that need no gradient take the same path with grad mode on
    assert torch.equal(fn.token_head_loss(xin, w, t, softcap="rsqrt15"), with_grad)


# ---- 9. autograd
def test_autograd_scaling_accumulation_and_retained_graph():
    x, w, t = (a.to(DEV) for a in tr.case_inputs("sigmoid30", True))
    one = fused(x, w, t, "sigmoid30")
    xl, wl = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    (3.5 * fn.token_head_loss(xl, wl, t)).backward()
    assert relerr(xl.grad, 3.5 * one["dx"]) < 1e-6 and relerr(wl.grad, 3.5 * one["dW"]) < 1e-6
    fn.token_head_loss(xl, wl, t).backward()   # .grad accumulates
    assert relerr(xl.grad, 4.5 * one["dx"]) < 1e-6 and relerr(wl.grad, 4.5 * one["dW"]) < 1e-6
    xl.grad = wl.grad = None
    loss = fn.token_head_loss(xl, wl, t)
    loss.backward(retain_graph=True)
    g1 = (xl.grad.clone(), wl.grad.clone())
    xl.grad = wl.grad = None
    (2 * loss).backward()
    assert torch.equal(g1[0], one["dx"]) and relerr(g1[1], one["dW"]) < 1e-6
    assert relerr(xl.grad, 2 * g1[0]) < 1e-6 and relerr(wl.grad, 2 * g1[1]) < 1e-6


def test_autograd_one_sided_and_int32_targets():
    x, w, t = (a.to(DEV) for a in tr.case_inputs("rsqrt15", True))
    one = fused(x, w, t, "rsqrt15")
    xl = x.clone().requires_grad_(True)
    fn.token_head_loss(xl, w, t.int(), softcap="rsqrt15").backward()
    assert torch.equal(xl.grad, one["dx"])
    wl = w.clone().requires_grad_(True)
    loss = fn.token_head_loss(x, wl, t, softcap="rsqrt15")
    loss.backward()
    assert torch.equal(loss, one["loss"]) and relerr(wl.grad, one["dW"]) < 1e-6


def test_fp32_parameter_with_bf16_x_and_the_module():
    x, w, t = (a.to(DEV) for a in tr.case_inputs("sigmoid30", True))
    lm = CastedLinear(tr.DIM, tr.VOCAB).to(DEV)
    with torch.no_grad():
        lm.weight.copy_(w)
    xb = x.to(torch.bfloat16).requires_grad_(True)
    m = ByteMixout(ModelDims(model_dim=tr.DIM), 64, ByteHyperparameters(bytes_per_token=16, byte_mixout_method="noop")).to(DEV)
    loss = m.loss(xb[None], lm, t[None])   # (B, T, D) and (B, T), as GPT.forward holds them
    loss.backward()
    assert lm.weight.grad.dtype == torch.float32 and xb.grad.dtype == torch.bfloat16 and xb.grad.shape == xb.shape
    direct = fused(xb, w, t, "sigmoid30")
    assert torch.equal(loss.detach(), direct["loss"]) and torch.equal(xb.grad, direct["dx"])
    assert relerr(lm.weight.grad, direct["dW"]) < 1e-6   # the same path twice: the order of the fp32 atomics is all that differs
    assert list(m.state_dict()) == []


def test_row_stats_of_the_c_abi():
    x, w, t = (a.to(DEV) for a in tr.case_inputs("rsqrt15", True))
    stats = torch.zeros(2 * tr.ROWS, device=DEV)
    loss = torch.zeros((), device=DEV)
    d = capi.MotTokenHeadDesc()
    d.struct_size = C.sizeof(capi.MotTokenHeadDesc)
    d.dtype, d.softcap, d.norm_in, d.n_rows, d.model_dim, d.vocab, d.chunk_rows = capi.F32, capi.SOFTCAP_RSQRT15, 1, tr.ROWS, tr.DIM, tr.VOCAB, 32
    d.x, d.weight, d.targets, d.loss, d.row_stats = x.data_ptr(), w.data_ptr(), t.data_ptr(), loss.data_ptr(), stats.data_ptr()
    ws = torch.empty(capi.lib.mot_token_head_workspace_bytes(C.byref(d)), dtype=torch.uint8, device=DEV)
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    capi.check(capi.lib.mot_token_head_fwd(C.byref(d), capi.stream_of(DEV)))
    torch.cuda.synchronize()
    xd = x.double()
    c = (xd.square().mean(-1) + torch.finfo(torch.float32).eps).rsqrt()
    z = tr.softcap((xd * c[:, None]) @ w.double().T, "rsqrt15")
    assert relerr(stats[tr.ROWS:], c) < 1e-6 and relerr(stats[:tr.ROWS], torch.logsumexp(z, -1)) < 1e-6
    assert relerr(loss, tr.head(x, w, t, "rsqrt15")["loss"]) < FP32_LOSS


# ---- 10. memory: forward + backward at 8192 rows stay below ONE fp32 logits tensor, of which eager keeps at least three
def test_peak_memory_below_one_logits_tensor():
    N = 8192
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn(N, D_REAL, device=DEV, generator=g).to(torch.bfloat16).requires_grad_(True)
    w = ((torch.rand(V_REAL, D_REAL, device=DEV, generator=g) * 2 - 1) * 0.03).requires_grad_(True)
    t = torch.randint(0, 50257, (N,), device=DEV, generator=g)
    fn.release_workspaces()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn.token_head_loss(x, w, t).backward()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    one_logits = N * V_REAL * 4
    print(f"peak extra memory of forward + backward {extra / 2**20:.1f} MiB; one fp32 logits tensor {one_logits / 2**20:.1f} MiB")
    assert x.grad is not None and w.grad is not None and torch.isfinite(w.grad).all()
    assert extra < one_logits
    fn.release_workspaces()
