"""CPU checks of the byte output head: the C ABI's struct and validation (no GPU needed), ByteMixout's module surface, and the float64
restatement (tests/byte_head_ref.py) against the reference's own outputs in tests/golden/byte_head.npz."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

import byte_head_ref as br
import mixture_of_tokenizers_amd as mot
from mixture_of_tokenizers_amd import _capi as capi
from mixture_of_tokenizers_amd.modules import ByteHyperparameters, ByteMixout, ModelDims

GOLDEN = np.load(Path(__file__).parent / "golden" / "byte_head.npz")


def _desc(**kw):
    d = capi.MotByteHeadDesc()
    d.struct_size = C.sizeof(capi.MotByteHeadDesc)
    d.method, d.dtype, d.bpt, d.n_tokens, d.model_dim, d.n_layer_out, d.vocab = capi.HEAD_SPLIT, capi.F32, 16, 8, 1024, 1, 512
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _rc(d):
    return capi.lib.mot_byte_head_fwd(C.byref(d), None), capi.lib.mot_byte_head_bwd(C.byref(d), None, None, None, None)


def test_struct_size_matches_library():
    assert capi.lib.mot_byte_head_desc_size() == C.sizeof(capi.MotByteHeadDesc)
    assert capi.ABI_VERSION == 13 == capi.lib.mot_version()


@pytest.mark.parametrize("kw, want", [
    (dict(struct_size=0), capi.MOT_EINVAL),
    (dict(method=7), capi.MOT_EUNSUPPORTED),
    (dict(vocab=458), capi.MOT_EUNSUPPORTED),
    (dict(method=capi.HEAD_COPY, model_dim=1000), capi.MOT_EUNSUPPORTED),   # K % 16
    (dict(method=capi.HEAD_COPY, model_dim=4096), capi.MOT_EUNSUPPORTED),   # K > 2048
    (dict(model_dim=1000), capi.MOT_ESHAPE),                                # split, D % bpt
    (dict(model_dim=16 * 24), capi.MOT_EUNSUPPORTED),                       # split, K = 24
    (dict(dtype=5), capi.MOT_EUNSUPPORTED),
    (dict(bpt=0), capi.MOT_ESHAPE),
])
def test_validation_without_gpu(kw, want):
    d = _desc(**kw)
    assert _rc(d) == (want, want)
    assert capi.lib.mot_byte_head_workspace_bytes(C.byref(d)) == 0


def test_null_pointers_are_refused_before_any_launch():
    d = _desc()
    assert capi.lib.mot_byte_head_workspace_bytes(C.byref(d)) > 0
    assert _rc(d) == (capi.MOT_EINVAL, capi.MOT_EINVAL)


def test_x_dtype_is_named_in_the_error():
    x = torch.zeros(4, 16, dtype=torch.float16)
    with pytest.raises(TypeError, match="byte_head_loss: x must be float32 or bfloat16"):
        mot.byte_head_loss(x, torch.zeros(512, 16), torch.zeros(64, dtype=torch.int64), method="copy", bytes_per_token=16)


def test_target_status_bit_is_named():
    assert capi.STATUS_TARGET_OOR == 4
    assert "mot_byte_head_fwd" in capi.EXPORTS and "mot_byte_head_bwd" in capi.EXPORTS
    assert mot.byte_head_loss is mot.functional.byte_head_loss


def test_mixout_refuses_self_attention():
    bp = ByteHyperparameters(bytes_per_token=16, byte_mixout_method="copy", use_byte_self_attn=True)
    with pytest.raises(NotImplementedError, match="train_gpt.py:382-419"):
        ByteMixout(ModelDims(model_dim=1024), 1024, bp)


@pytest.mark.parametrize("method", ["copy", "split", "noop"])
def test_mixout_module_surface(method):
    bp = ByteHyperparameters(bytes_per_token=16, byte_mixout_method=method, n_layer_out=2)
    m = ByteMixout(ModelDims(model_dim=1024), 1024, bp)
    assert list(m.state_dict()) == [] and list(m.parameters()) == []
    if method != "noop":
        assert len(m.mixout.attention_layers) == 2


@pytest.mark.parametrize("method", ["copy", "split"])
@pytest.mark.parametrize("L", br.LAYERS)
def test_restatement_reproduces_reference_float64(method, L):
    x, w, t = br.case_inputs(method, L)
    r = br.head(x, w, t, method, br.BPT, L, torch.float64)
    for what in ("loss", "dx", "dW", "states"):
        ref = GOLDEN[br.case_key(method, L, "f64", what)]
        got = r[what].numpy()
        assert got.shape == ref.shape, what
        assert np.abs(got - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1e-300), what


@pytest.mark.parametrize("method", ["copy", "split"])
@pytest.mark.parametrize("L", br.LAYERS)
def test_mixout_forward_matches_reference_states(method, L):
    x, _, _ = br.case_inputs(method, L)
    bp = ByteHyperparameters(bytes_per_token=br.BPT, byte_mixout_method=method, n_layer_out=L)
    m = ByteMixout(ModelDims(model_dim=x.shape[1]), br.N_TOKENS, bp)
    h = m(x.double()[None])[0].numpy()
    ref = GOLDEN[br.case_key(method, L, "f64", "states")]
    assert np.abs(h - ref).max() <= 1e-12 * np.abs(ref).max()


def test_fixture_records_torch_version():
    assert str(GOLDEN["torch_version"])
