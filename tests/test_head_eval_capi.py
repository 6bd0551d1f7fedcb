"""CPU checks of the heads' evaluation calls (mot_token_head_eval, mot_byte_head_eval): the out struct, every refusal before any
HIP call with the function's name in front of its message, the workspace rule, and the Python surface (no GPU needed)."""
import ctypes as C

import pytest
import torch

import byte_head_ref as br
import mixture_of_tokenizers_amd as mot
import token_head_ref as tr
from mixture_of_tokenizers_amd import _capi as capi
from mixture_of_tokenizers_amd.modules import ByteHyperparameters, ByteMixout, CastedLinear, ModelDims

NAMES = ("mot_head_eval_out_size", "mot_token_head_eval", "mot_byte_head_eval")


def _tok(**kw):
    d = capi.MotTokenHeadDesc()
    d.struct_size = C.sizeof(capi.MotTokenHeadDesc)
    d.dtype, d.softcap, d.norm_in, d.n_rows, d.model_dim, d.vocab = capi.F32, capi.SOFTCAP_SIGMOID30, 1, 65536, 768, 50304
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _byte(**kw):
    d = capi.MotByteHeadDesc()
    d.struct_size = C.sizeof(capi.MotByteHeadDesc)
    d.method, d.dtype, d.bpt, d.n_tokens, d.model_dim, d.n_layer_out, d.vocab = capi.HEAD_SPLIT, capi.F32, 16, 8, 1024, 1, 512
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _out(**kw):
    o = capi.MotHeadEvalOut()
    o.struct_size = C.sizeof(capi.MotHeadEvalOut)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


HEADS = {
    "token": (capi.lib.mot_token_head_eval, _tok, "mot_token_head_eval: "),
    "byte": (capi.lib.mot_byte_head_eval, _byte, "mot_byte_head_eval: "),
}


def _refused(head, d, o, want, msg):
    fn, _, name = HEADS[head]
    rc = fn(None if d is None else C.byref(d), None if o is None else C.byref(o), None)
    err = capi.lib.mot_last_error().decode()
    assert rc == want, (rc, err)
    assert err.startswith(name) and msg in err, err


def test_struct_size_exports_and_surface():
    assert capi.lib.mot_head_eval_out_size() == C.sizeof(capi.MotHeadEvalOut) == 40
    assert capi.ABI_VERSION == 13 == capi.lib.mot_version()   # new symbols only
    for name in NAMES:
        assert name in capi.EXPORTS and hasattr(capi.lib, name), name
    for name in ("token_head_eval", "byte_head_eval", "HeadEval"):
        assert getattr(mot, name) is getattr(mot.functional, name) and name in mot.__all__
    assert mot.HeadEval._fields == ("loss", "row_loss", "pred", "rank", "counts")
    assert callable(ByteMixout.evaluate)


@pytest.mark.parametrize("head", HEADS)
def test_out_struct_refusals(head):
    d = HEADS[head][1]()
    _refused(head, None, _out(), capi.MOT_EINVAL, "null descriptor")
    _refused(head, d, None, capi.MOT_EINVAL, "null out struct")
    _refused(head, d, _out(struct_size=0), capi.MOT_EINVAL, "struct_size")
    _refused(head, d, _out(struct_size=48), capi.MOT_EINVAL, "struct_size")
    _refused(head, d, _out(reserved=1), capi.MOT_EINVAL, "reserved")
    for field, addr in (("row_loss", 258), ("pred", 257), ("rank", 259), ("counts", 260)):
        _refused(head, d, _out(**{"pred": 256, field: addr}), capi.MOT_EINVAL, "aligned")
    _refused(head, d, _out(counts=256), capi.MOT_EINVAL, "counts needs pred")
    d.struct_size = 0
    _refused(head, d, _out(), capi.MOT_EINVAL, "struct_size")


def test_token_descriptor_with_gradients_is_refused():
    for kw in (dict(dx=256), dict(dW=256), dict(dx=256, dW=512)):
        _refused("token", _tok(**kw), _out(), capi.MOT_EINVAL, "forms no gradients")


@pytest.mark.parametrize("kw, want, msg", [
    (dict(vocab=50257), capi.MOT_EUNSUPPORTED, "vocab 50257 must be a multiple of 128"),
    (dict(vocab=262144 + 128), capi.MOT_EUNSUPPORTED, "at most 262144"),
    (dict(model_dim=1000), capi.MOT_EUNSUPPORTED, "model_dim 1000 must be a multiple of 16"),
    (dict(model_dim=4096), capi.MOT_EUNSUPPORTED, "at most 2048"),
    (dict(dtype=5), capi.MOT_EUNSUPPORTED, "dtype 5"),
    (dict(softcap=2), capi.MOT_EUNSUPPORTED, "softcap 2"),
    (dict(chunk_rows=100), capi.MOT_ESHAPE, "chunk_rows 100 must be 0"),
    (dict(chunk_rows=-32), capi.MOT_ESHAPE, "chunk_rows -32"),
    (dict(chunk_rows=1 << 16), capi.MOT_EUNSUPPORTED, "exceeds 2^31"),
    (dict(n_rows=-1), capi.MOT_ESHAPE, "n_rows -1"),
])
def test_token_head_refusals_of_the_forward(kw, want, msg):
    """The cases of test_token_head_capi.py: the evaluation refuses them with the forward's codes."""
    d = _tok(**kw)
    assert capi.lib.mot_token_head_fwd(C.byref(d), None) == want
    _refused("token", d, _out(), want, msg)


@pytest.mark.parametrize("kw, want", [
    (dict(method=7), capi.MOT_EUNSUPPORTED),
    (dict(vocab=458), capi.MOT_EUNSUPPORTED),
    (dict(method=capi.HEAD_COPY, model_dim=1000), capi.MOT_EUNSUPPORTED),   # K % 16
    (dict(method=capi.HEAD_COPY, model_dim=4096), capi.MOT_EUNSUPPORTED),   # K > 2048
    (dict(model_dim=1000), capi.MOT_ESHAPE),                                # split, D % bpt
    (dict(model_dim=16 * 24), capi.MOT_EUNSUPPORTED),                       # split, K = 24
    (dict(dtype=5), capi.MOT_EUNSUPPORTED),
    (dict(bpt=0), capi.MOT_ESHAPE),
])
def test_byte_head_refusals_of_the_forward(kw, want):
    """The cases of test_byte_head_capi.py."""
    d = _byte(**kw)
    assert capi.lib.mot_byte_head_fwd(C.byref(d), None) == want
    _refused("byte", d, _out(), want, "")


def test_pointers_rows_and_workspace_are_refused_before_any_launch():
    d = _tok()
    _refused("token", d, _out(), capi.MOT_EINVAL, "null x")
    d.x = d.weight = d.targets = d.loss = 256   # never dereferenced: the workspace check fails first
    _refused("token", d, _out(), capi.MOT_EWORKSPACE, "workspace 0 bytes")
    d.workspace, d.workspace_bytes = 256, 1 << 40
    d.x = 264
    _refused("token", d, _out(), capi.MOT_EUNSUPPORTED, "16-byte aligned")
    _refused("token", _tok(n_rows=0, x=256, weight=256, targets=256, loss=256), _out(), capi.MOT_ESHAPE, "no rows")
    b = _byte()
    _refused("byte", b, _out(), capi.MOT_EINVAL, "null loss")
    b.loss = 256
    _refused("byte", b, _out(), capi.MOT_EINVAL, "null x")
    b.x = b.weight = b.targets = 256             # row_stats stays NULL: the evaluation does not need it
    _refused("byte", b, _out(), capi.MOT_EWORKSPACE, "workspace 0 bytes")
    _refused("byte", _byte(n_tokens=0, loss=256), _out(), capi.MOT_ESHAPE, "no targets")


def test_evaluation_needs_no_more_workspace_than_the_forward_without_gradients():
    """The call takes the workspace of the gradient-free forward (mot.h names the query): one byte less is refused with that size in
    the message, and the refusal names no larger one."""
    for kw in (dict(), dict(dtype=capi.BF16), dict(chunk_rows=128), dict(n_rows=40, vocab=384, model_dim=64)):
        d = _tok(x=256, weight=256, targets=256, loss=256, **kw)
        need = capi.lib.mot_token_head_workspace_bytes(C.byref(d))
        assert 0 < need < capi.lib.mot_token_head_workspace_bytes(C.byref(_tok(dx=256, **kw)))
        d.workspace, d.workspace_bytes = 256, need - 1
        _refused("token", d, _out(pred=256, counts=512), capi.MOT_EWORKSPACE, f"workspace {need - 1} bytes < {need}")
    for kw in (dict(), dict(method=capi.HEAD_COPY, dtype=capi.BF16, n_tokens=1000)):
        b = _byte(x=256, weight=256, targets=256, loss=256, **kw)
        need = capi.lib.mot_byte_head_workspace_bytes(C.byref(b))
        assert need > 0
        b.workspace, b.workspace_bytes = 256, need - 1
        _refused("byte", b, _out(pred=256, counts=512), capi.MOT_EWORKSPACE, f"workspace {need - 1} bytes < {need}")


def test_cpu_tensors_are_refused():
    x, w, t = tr.case_inputs("sigmoid30", True)
    with pytest.raises(RuntimeError, match="HIP device only"):
        mot.token_head_eval(x, w, t)
    with torch.enable_grad(), pytest.raises(RuntimeError, match="HIP device only"):
        mot.token_head_eval(x.requires_grad_(True), w, t.int(), softcap="rsqrt15", norm_in=False, chunk_rows=32)
    for method in ("copy", "split"):
        xb, wb, tb = br.case_inputs(method, 1)
        with pytest.raises(RuntimeError, match="HIP device only"):
            mot.byte_head_eval(xb, wb, tb, method=method, bytes_per_token=br.BPT, n_layer_out=1)


def test_arguments_are_checked_as_in_the_loss_calls():
    x, w, t = tr.case_inputs("sigmoid30", True)
    with pytest.raises(TypeError, match="x must be float32 or bfloat16"):
        mot.token_head_eval(x.half(), w, t)
    with pytest.raises(ValueError, match="softcap must be 'sigmoid30' or 'rsqrt15'"):
        mot.token_head_eval(x, w, t, softcap="tanh")
    with pytest.raises(TypeError, match="targets must be int64 or int32"):
        mot.token_head_eval(x, w, t.float())
    xb, wb, tb = br.case_inputs("copy", 0)
    with pytest.raises(TypeError, match="x must be float32 or bfloat16"):
        mot.byte_head_eval(xb.half(), wb, tb, method="copy", bytes_per_token=br.BPT)
    with pytest.raises(ValueError, match="method must be 'copy' or 'split'"):
        mot.byte_head_eval(xb, wb, tb, method="noop", bytes_per_token=br.BPT)


@pytest.mark.parametrize("method", ["noop", "copy", "split"])
def test_mixout_evaluate_reaches_the_fused_call(method):
    bp = ByteHyperparameters(bytes_per_token=br.BPT, byte_mixout_method=method, n_layer_out=1)
    if method == "noop":
        x, w, t = tr.case_inputs("sigmoid30", True)
    else:
        x, w, t = br.case_inputs(method, 1)
    m = ByteMixout(ModelDims(model_dim=x.shape[1]), 1024, bp)
    lm = CastedLinear(w.shape[1], w.shape[0])
    with pytest.raises(RuntimeError, match="HIP device only"):
        m.evaluate(x[None], lm, t[None])
