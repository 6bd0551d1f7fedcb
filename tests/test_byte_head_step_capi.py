"""CPU checks of mot_byte_head_step, the split-mode byte head's training step in one call (csrc/mot_headstep.hip): the two symbols,
every refusal before any launch (fake pointers), the workspace formula, and the Python surface byte_head_loss(one_call=True) /
ByteMixout.loss(one_call=True)."""
import ctypes as C

import pytest
import torch

import mixture_of_tokenizers_amd as mot
from mixture_of_tokenizers_amd import _capi as capi
from mixture_of_tokenizers_amd.modules import ByteHyperparameters, ByteMixout, ModelDims

NEW = ("mot_byte_head_step_workspace_bytes", "mot_byte_head_step")
PTR = 0x10000   # fake, 16-byte aligned: every call below is refused before anything reads it
MiB = 1 << 20


def _desc(n_tokens=2, **kw):
    d = capi.MotByteHeadDesc()
    d.struct_size = C.sizeof(capi.MotByteHeadDesc)
    d.method, d.dtype, d.bpt, d.n_tokens, d.model_dim, d.n_layer_out, d.vocab = capi.HEAD_SPLIT, capi.BF16, 16, n_tokens, 1024, 1, 512
    d.x, d.weight, d.targets, d.loss = PTR, PTR, PTR, PTR
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _ws(d):
    return capi.lib.mot_byte_head_step_workspace_bytes(C.byref(d))


def _rc(d, dx=PTR, dw=PTR):
    return capi.lib.mot_byte_head_step(C.byref(d), dx, dw, None)


def _err():
    return capi.lib.mot_last_error().decode()


def up256(n):
    return (n + 255) // 256 * 256


def test_new_symbols_are_exported_and_the_abi_version_stays():
    for name in NEW:
        assert name in capi.EXPORTS and hasattr(capi.lib, name)
    assert capi.lib.mot_byte_head_step.restype is C.c_int and capi.lib.mot_byte_head_step_workspace_bytes.restype is C.c_size_t
    assert len(capi.lib.mot_byte_head_step.argtypes) == 4
    assert capi.lib.mot_byte_head_desc_size() == C.sizeof(capi.MotByteHeadDesc) == 104   # as before this call
    assert capi.ABI_VERSION == 13 == capi.lib.mot_version()


REFUSALS = [
    (dict(method=capi.HEAD_COPY), capi.MOT_EUNSUPPORTED, ("copy mode", "mot_byte_head_fwd")),
    (dict(method=7), capi.MOT_EUNSUPPORTED, ("method 7",)),
    (dict(vocab=458), capi.MOT_EUNSUPPORTED, ("vocab 458",)),
    (dict(dtype=5), capi.MOT_EUNSUPPORTED, ("dtype 5",)),
    (dict(model_dim=16 * 24), capi.MOT_EUNSUPPORTED, ("row width 24", "LDS")),             # K % 16
    (dict(model_dim=16 * 144), capi.MOT_EUNSUPPORTED, ("row width 144", "at most 128", "LDS")),   # bf16: K > 128
    (dict(dtype=capi.F32, model_dim=16 * 80), capi.MOT_EUNSUPPORTED, ("row width 80", "at most 64", "LDS")),   # fp32: K > 64
    (dict(model_dim=1000), capi.MOT_ESHAPE, ("model_dim % bpt",)),
    (dict(bpt=0), capi.MOT_ESHAPE, ("bpt 0",)),
    (dict(bpt=65, model_dim=65 * 16), capi.MOT_ESHAPE, ("bpt 65",)),
    (dict(n_layer_out=-1), capi.MOT_ESHAPE, ("n_layer_out -1",)),
    (dict(n_layer_out=65), capi.MOT_ESHAPE, ("n_layer_out 65",)),
    (dict(model_dim=0), capi.MOT_ESHAPE, ("model_dim 0",)),
    (dict(x=None), capi.MOT_EINVAL, ("null x",)),
    (dict(weight=None), capi.MOT_EINVAL, ("null x / weight",)),
    (dict(targets=None), capi.MOT_EINVAL, ("targets",)),
    (dict(loss=None), capi.MOT_EINVAL, ("loss",)),
    (dict(x=PTR + 8), capi.MOT_EUNSUPPORTED, ("16-byte aligned",)),
    (dict(weight=PTR + 2), capi.MOT_EUNSUPPORTED, ("16-byte aligned",)),
]


@pytest.mark.parametrize("n_tokens", [0, 2])
@pytest.mark.parametrize("kw, want, says", REFUSALS)
def test_refusals_before_any_launch(kw, want, says, n_tokens):
    d = _desc(n_tokens, **kw)
    for dx, dw in ((PTR, PTR), (None, None)):   # the training form and the loss alone
        assert _rc(d, dx, dw) == want
        assert _err().startswith("byte_head_step") and all(s in _err() for s in says), _err()
    assert _ws(d) == 0


def test_more_refusals():
    assert _rc(_desc(n_tokens=-1)) == capi.MOT_ESHAPE and _ws(_desc(n_tokens=-1)) == 0
    big = _desc(n_tokens=(1 << 31) // 16 + 1)
    assert _rc(big) == capi.MOT_EUNSUPPORTED and "2^31" in _err() and _ws(big) == 0
    assert _ws(_desc(n_tokens=(1 << 31) // 16)) > 0          # 2^31 targets themselves pass
    none = _desc(n_tokens=0)
    assert _rc(none) == capi.MOT_ESHAPE and _err().startswith("byte_head_step") and "no targets" in _err() and _ws(none) == 0
    assert capi.lib.mot_byte_head_step(None, PTR, PTR, None) == capi.MOT_EINVAL and capi.lib.mot_byte_head_step_workspace_bytes(None) == 0
    assert _rc(_desc(struct_size=0)) == capi.MOT_EINVAL and "ABI mismatch" in _err()
    for n in (0, 2):   # what the descriptor does not show: dx and dW come together, dx is aligned
        for dx, dw in ((PTR, None), (None, PTR)):
            d = _desc(n)
            assert (_rc(d, dx, dw) == capi.MOT_EINVAL and "dx and dW" in _err()) if n else _rc(d, dx, dw) == capi.MOT_ESHAPE
    assert _rc(_desc(), PTR + 4, PTR) == capi.MOT_EUNSUPPORTED and "16-byte aligned" in _err() and _err().startswith("byte_head_step")


@pytest.mark.parametrize("dtype, K", [(capi.BF16, K) for K in (16, 48, 64, 80, 128)] + [(capi.F32, K) for K in (16, 32, 48, 64)])
@pytest.mark.parametrize("bpt", [1, 3, 16])
def test_valid_split_descriptors_reach_the_workspace_check(dtype, K, bpt):
    """Validation passes, in the training form and for the loss alone, with row_stats NULL; the call stops at its workspace."""
    d = _desc(5, dtype=dtype, bpt=bpt, model_dim=K * bpt, n_layer_out=4)
    need = _ws(d)
    assert need > 0
    for dx, dw in ((PTR, PTR), (None, None)):
        for ws, ws_bytes in ((None, 0), (PTR, 0), (PTR, need - 1)):   # refused, not run: the pointers are fake
            d.workspace, d.workspace_bytes = ws, ws_bytes
            assert _rc(d, dx, dw) == capi.MOT_EWORKSPACE
            assert _err().startswith("byte_head_step") and str(need) in _err()


def test_the_workspace_has_no_term_in_rows_times_512_times_4():
    """What the pieces add up to: 4 bytes of loss term per byte row, the loss's 512 partial sums, ONE chunk's G in dtype (at most
    131 072 rows of 512 elements), and beside it the class-ordered k-major copy of W ([K rounded up to 32][512 + 8]) in bf16, a
    chunk's rows of x / se in fp32."""
    for T, bpt, K in ((8 * 1024, 16, 64), (64 * 1024, 16, 64), (64 * 1024, 16, 48), (1000, 3, 128), (1, 1, 16)):
        rows, Kp = T * bpt, (K + 31) // 32 * 32
        chunk = min(rows, 131072)
        want = up256(rows * 4) + 512 * 8 + up256(Kp * 520 * 2) + up256(chunk * 512 * 2)
        assert _ws(_desc(T, bpt=bpt, model_dim=K * bpt)) == want, (T, bpt, K)
        if K <= 64:
            want = up256(rows * 4) + 512 * 8 + up256(chunk * K * 4) + up256(chunk * 512 * 4)
            assert _ws(_desc(T, dtype=capi.F32, bpt=bpt, model_dim=K * bpt)) == want, (T, bpt, K)
    head = _desc(64 * 1024)                       # 1 M byte rows
    assert _ws(head) <= 133 * MiB < 64 * 1024 * 16 * 512 * 4 // 15
    assert _ws(_desc(64 * 1024, dtype=capi.F32)) <= 293 * MiB < 64 * 1024 * 16 * 512 * 4 // 6
    for dt in (capi.BF16, capi.F32):              # twice the rows: only the terms grow
        assert _ws(_desc(128 * 1024, dtype=dt)) - _ws(_desc(64 * 1024, dtype=dt)) == 64 * 1024 * 16 * 4


def _cpu_inputs(K=64, bpt=16, T=4, dtype=torch.bfloat16):
    x = torch.zeros(T, K * bpt, dtype=dtype, requires_grad=True)
    w = torch.zeros(512, K, requires_grad=True)
    return x, w, torch.zeros(T * bpt, dtype=torch.int64)


def test_functional_refuses_cpu_tensors_and_what_the_call_does_not_build_at_forward_time():
    x, w, t = _cpu_inputs()
    with pytest.raises(RuntimeError, match="HIP device only"):
        mot.byte_head_loss(x, w, t, method="split", bytes_per_token=16, n_layer_out=1, one_call=True)
    with torch.no_grad(), pytest.raises(RuntimeError, match="HIP device only"):
        mot.byte_head_loss(x, w, t, method="split", bytes_per_token=16, one_call=True)
    xc = torch.zeros(4, 64, dtype=torch.bfloat16, requires_grad=True)
    for grad in (True, False):   # before anything looks at the tensors' device; no fallback to the two-call path
        with torch.set_grad_enabled(grad):
            with pytest.raises(NotImplementedError, match="byte_head_step.*copy mode.*mot_byte_head_fwd"):
                mot.byte_head_loss(xc, w, t, method="copy", bytes_per_token=16, one_call=True)
            x80, w80, t80 = _cpu_inputs(K=80, dtype=torch.float32)
            with pytest.raises(NotImplementedError, match="byte_head_step.*row width 80.*at most 64"):
                mot.byte_head_loss(x80, w80, t80, method="split", bytes_per_token=16, one_call=True)
            x24, w24, t24 = _cpu_inputs(K=24)
            with pytest.raises(NotImplementedError, match="row width 24"):
                mot.byte_head_loss(x24, w24, t24, method="split", bytes_per_token=16, one_call=True)
            x144, w144, t144 = _cpu_inputs(K=144)
            with pytest.raises(NotImplementedError, match="row width 144.*LDS"):
                mot.byte_head_loss(x144, w144, t144, method="split", bytes_per_token=16, one_call=True)
    with pytest.raises(ValueError, match="method must be"):
        mot.byte_head_loss(x, w, t, method="mean", bytes_per_token=16, one_call=True)
    with pytest.raises(RuntimeError, match="HIP device only"):   # the default is the two-call path, as before
        mot.byte_head_loss(x, w, t, method="split", bytes_per_token=16)


def test_mixout_loss_passes_one_call_through():
    x, w, t = _cpu_inputs()
    lm = torch.nn.Linear(64, 512, bias=False)
    split = ByteMixout(ModelDims(model_dim=1024), 1024, ByteHyperparameters(bytes_per_token=16, byte_mixout_method="split", n_layer_out=1))
    with pytest.raises(RuntimeError, match="HIP device only"):
        split.loss(x[None], lm, t[None], one_call=True)
    wide = ByteMixout(ModelDims(model_dim=16 * 144), 1024, ByteHyperparameters(bytes_per_token=16, byte_mixout_method="split", n_layer_out=1))
    with pytest.raises(NotImplementedError, match="byte_head_step.*row width 144"):   # the new call's own refusal: it was reached
        wide.loss(torch.zeros(1, 4, 16 * 144, dtype=torch.bfloat16), torch.nn.Linear(144, 512, bias=False), t[None], one_call=True)
    copy = ByteMixout(ModelDims(model_dim=64), 1024, ByteHyperparameters(bytes_per_token=16, byte_mixout_method="copy", n_layer_out=1))
    with pytest.raises(NotImplementedError, match="byte_head_step.*copy mode"):
        copy.loss(torch.zeros(1, 4, 64, dtype=torch.bfloat16), lm, t[None], one_call=True)
    with pytest.raises(RuntimeError, match="HIP device only"):   # the default stays the two-call path
        copy.loss(torch.zeros(1, 4, 64, dtype=torch.bfloat16), lm, t[None])
