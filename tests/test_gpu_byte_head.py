"""The fused byte output head (functional.byte_head_loss / ByteMixout.loss, csrc/mot_head.hip) against float64: the reference's
fixture cases, production shapes with loader-made targets, autograd, memory, determinism, hipGraph capture, out-of-range targets."""
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import byte_head_ref as br
import golden_inputs as gi
import mixture_of_tokenizers_amd as mot
from mixture_of_tokenizers_amd import functional as fn
from mixture_of_tokenizers_amd.modules import ByteHyperparameters, ByteMixout, CastedLinear, ModelDims

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GOLDEN = np.load(Path(__file__).parent / "golden" / "byte_head.npz")
FP32_LOSS, FP32_GRAD = 2e-6, 2e-5


def rel(got, ref):
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    return float((got - ref).abs().max() / max(ref.abs().max().item(), 1e-300))


def fused(x, w, t, method, L, bpt=br.BPT):
    xl = x.detach().clone().requires_grad_(True)
    wl = w.detach().clone().requires_grad_(True)
    loss = fn.byte_head_loss(xl, wl, t, method=method, bytes_per_token=bpt, n_layer_out=L)
    loss.backward()
    return {"loss": loss.detach(), "dx": xl.grad, "dW": wl.grad}


def check_fp32(got, ref):
    assert rel(got["loss"], ref["loss"]) < FP32_LOSS
    assert rel(got["dx"], ref["dx"]) < FP32_GRAD
    assert rel(got["dW"], ref["dW"]) < FP32_GRAD


def check_bf16(got, ref, eager):
    for k in ("loss", "dx", "dW"):
        ref_k = ref[k].double().cpu()
        scale = max(ref_k.abs().max().item(), 1e-300)
        err = (got[k].double().cpu() - ref_k).abs().max().item() / scale
        own = (eager[k].double().cpu() - ref_k).abs().max().item() / scale
        assert err <= 2 * own + 2 ** -12, f"{k}: {err:.3e} vs eager bf16 {own:.3e}"


@pytest.mark.parametrize("method", ["copy", "split"])
@pytest.mark.parametrize("L", br.LAYERS)
def test_fixture_fp32(method, L):
    x, w, t = br.case_inputs(method, L)
    got = fused(x.to(DEV), w.to(DEV), t.to(DEV), method, L)
    ref = {k: torch.from_numpy(np.asarray(GOLDEN[br.case_key(method, L, "f64", k)])) for k in ("loss", "dx", "dW")}
    check_fp32(got, ref)


@pytest.mark.parametrize("method", ["copy", "split"])
@pytest.mark.parametrize("L", br.LAYERS)
def test_fixture_bf16(method, L):
    x, w, t = br.case_inputs(method, L)
    xb = x.to(torch.bfloat16)
    ref = br.head(xb.double(), w.to(torch.bfloat16).double(), t, method, br.BPT, L, torch.float64)   # same bf16-valued inputs
    eager = {k: torch.from_numpy(np.asarray(GOLDEN[br.case_key(method, L, "bf16", k)])) for k in ("loss", "dx", "dW")}
    got = fused(xb.to(DEV), w.to(DEV), t.to(DEV), method, L)
    assert got["dx"].dtype == torch.bfloat16 and got["dW"].dtype == torch.float32
    check_bf16(got, ref, eager)


def loader_targets(B, T, bpt, seed=5):
    from mixture_of_tokenizers_amd import loader
    tab = torch.from_numpy(gi.synth_ttb(seed, 4096, bpt, "left")).to(DEV)
    bp = ByteHyperparameters(bytes_per_token=bpt, byte_mixin_method="noop", pull_in=False, byte_mixout_method="copy", pull_out=False)
    toks = torch.from_numpy(gi.fineweb_like_tokens(seed, B, T + 1, vocab=4096, eot_p=0.01)).to(DEV)
    _, _, _, targets = loader.make_create_data_from_toks(bp, tab, tab)(toks)
    assert targets.shape == (B, T * bpt) and targets.dtype == torch.int64
    return targets


def prod_inputs(D, K, seed, B=8, T=1024):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(B, T, D, device=DEV, generator=g)
    bound = (3 ** 0.5) * 0.5 * K ** -0.5
    w = (torch.rand(512, K, device=DEV, generator=g) * 2 - 1) * bound
    return x, w


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("L", [0, 1])
@pytest.mark.parametrize("method", ["copy", "split"])
@pytest.mark.parametrize("D", [1024, 768])
def test_production_shapes(D, method, L, dtype):
    bpt = 16
    K = D if method == "copy" else D // bpt
    x, w = prod_inputs(D, K, seed=D + L)
    t = loader_targets(8, 1024, bpt)
    assert (t == gi.PAD).float().mean() > 0.3   # pad-heavy, like real targets
    xin = x.to(dtype)
    got = fused(xin, w, t, method, L, bpt)
    wq = w.to(dtype).double() if dtype == torch.bfloat16 else w.double()
    ref = br.head(xin.double(), wq, t, method, bpt, L, torch.float64)
    if dtype == torch.float32:
        check_fp32(got, ref)
    else:
        check_bf16(got, ref, br.head(xin, w, t, method, bpt, L, torch.bfloat16))


@pytest.mark.parametrize("L", [0, 1])
def test_copy_fp32_over_several_chunks(L):
    # copy fp32 at D 1024 runs 8192 rows per chunk (48 MiB of scratch at 6 KB a row): 10 x 1024 tokens take a full chunk and a
    # short one, so the row offsets of the second chunk and dW summed over both are checked against float64
    B, T, D, bpt = 10, 1024, 1024, 16
    x, w = prod_inputs(D, D, seed=40 + L, B=B, T=T)
    t = torch.randint(0, 458, (B, T * bpt), device=DEV, generator=torch.Generator(device=DEV).manual_seed(41))
    check_fp32(fused(x, w, t, "copy", L, bpt), br.head(x.double(), w.double(), t, "copy", bpt, L, torch.float64))


def test_autograd_into_leaf_and_casted_linear():
    x, w, t = br.case_inputs("split", 1)
    lm = CastedLinear(w.shape[1], 512).to(DEV)
    with torch.no_grad():
        lm.weight.copy_(w)
    xl = x.to(DEV).requires_grad_(True)
    loss = fn.byte_head_loss(xl, lm.weight, t.to(DEV), method="split", bytes_per_token=br.BPT, n_layer_out=1)
    loss.backward()
    g1 = (xl.grad.clone(), lm.weight.grad.clone())
    assert lm.weight.grad.dtype == torch.float32
    xl.grad = lm.weight.grad = None
    (3 * fn.byte_head_loss(xl, lm.weight, t.to(DEV), method="split", bytes_per_token=br.BPT, n_layer_out=1)).backward()
    assert rel(xl.grad, 3 * g1[0]) < 1e-6 and rel(lm.weight.grad, 3 * g1[1]) < 1e-6


@pytest.mark.parametrize("method", ["copy", "split"])
@pytest.mark.parametrize("T", [1024, 8192])
def test_peak_memory(method, T):
    B, D, bpt = 8, 1024, 16
    K = D if method == "copy" else D // bpt
    x, w = prod_inputs(D, K, seed=3, B=B, T=T)
    t = torch.randint(0, 458, (B, T * bpt), device=DEV)
    xl, wl = x.requires_grad_(True), w.requires_grad_(True)
    fn.release_workspaces()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn.byte_head_loss(xl, wl, t, method=method, bytes_per_token=bpt, n_layer_out=1).backward()
    torch.cuda.synchronize()
    grads = xl.grad.numel() * 4 + wl.grad.numel() * 4
    extra = torch.cuda.max_memory_allocated() - base - grads
    M = B * T * bpt
    assert extra <= max(64 << 20, M * 512 * 4 // 8), f"{extra / 2**20:.1f} MiB"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("method", ["copy", "split"])
def test_deterministic(method, dtype):
    D, bpt = 1024, 16
    K = D if method == "copy" else D // bpt
    x, w = prod_inputs(D, K, seed=9)
    t = torch.randint(0, 458, (8, 1024 * bpt), device=DEV)
    a = fused(x.to(dtype), w, t, method, 1, bpt)
    b = fused(x.to(dtype), w, t, method, 1, bpt)
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["dx"], b["dx"])


@pytest.mark.parametrize("method", ["copy", "split"])
def test_hipgraph_capture_and_replay(method):
    D, bpt, L = 256, 16, 1
    K = D if method == "copy" else D // bpt
    x1, w = prod_inputs(D, K, seed=11, B=2, T=256)
    x2, _ = prod_inputs(D, K, seed=12, B=2, T=256)
    t1 = torch.randint(0, 458, (2, 256 * bpt), device=DEV)
    t2 = torch.randint(0, 458, (2, 256 * bpt), device=DEV)
    xs, ws, ts = x1.clone().requires_grad_(True), w.clone().requires_grad_(True), t1.clone()

    def step():
        fn.byte_head_loss(xs, ws, ts, method=method, bytes_per_token=bpt, n_layer_out=L).backward()

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            xs.grad = ws.grad = None
            step()
    torch.cuda.current_stream().wait_stream(s)
    xs.grad = ws.grad = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loss = fn.byte_head_loss(xs, ws, ts, method=method, bytes_per_token=bpt, n_layer_out=L)
        loss.backward()
    with torch.no_grad():
        xs.copy_(x2)
        ts.copy_(t2)
    g.replay()
    torch.cuda.synchronize()
    ref = fused(x2, w, t2, method, L, bpt)
    assert torch.equal(loss, ref["loss"]) and torch.equal(xs.grad, ref["dx"])
    assert rel(ws.grad, ref["dW"]) < 1e-6


@pytest.mark.parametrize("method", ["copy", "split"])
def test_out_of_range_target(method):
    x, w, t = br.case_inputs(method, 1)
    t = t.clone()
    t[37] = 600
    mot.check_status()
    got = fused(x.to(DEV), w.to(DEV), t.to(DEV), method, 1)
    word = mot._capi.status_word(DEV)
    assert int(word.item()) & mot._capi.STATUS_TARGET_OOR
    with pytest.raises(IndexError, match="byte target"):
        mot.check_status()
    t_ok = t.clone()
    t_ok[37] = 0
    ref = br.head(x, w, t_ok, method, br.BPT, 1, torch.float64, drop=[37])
    check_fp32(got, ref)


@pytest.mark.parametrize("method", ["copy", "split"])
def test_module_loss_matches_its_forward(method):
    D, bpt = 256, 16
    bp = ByteHyperparameters(bytes_per_token=bpt, byte_mixout_method=method, n_layer_out=1)
    m = ByteMixout(ModelDims(model_dim=D), 512, bp).to(DEV)
    K = D if method == "copy" else D // bpt
    lm = CastedLinear(K, 512).to(DEV)
    x, _ = prod_inputs(D, K, seed=21, B=2, T=512)
    t = torch.randint(0, 458, (2, 512 * bpt), device=DEV)
    fused_loss = m.loss(x, lm, t)
    h = F.rms_norm(m(x), (K,))
    z = 30 * torch.sigmoid(lm(h).float() / 7.5)
    eager = F.cross_entropy(z.view(-1, 512), t.view(-1))
    assert rel(fused_loss, eager) < FP32_LOSS * 4
    assert list(m.state_dict()) == []
