"""CPU checks of the token-level output head: the C ABI's struct, validation and workspace query (no GPU needed), the module and
package surface, and the float64 restatement (tests/token_head_ref.py) against the reference's own outputs in
tests/golden/token_head.npz."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

import mixture_of_tokenizers_amd as mot
import token_head_ref as tr
from mixture_of_tokenizers_amd import _capi as capi
from mixture_of_tokenizers_amd.modules import ByteHyperparameters, ByteMixout, CastedLinear, ModelDims

GOLDEN = np.load(Path(__file__).parent / "golden" / "token_head.npz")
NAMES = ("mot_token_head_desc_size", "mot_token_head_workspace_bytes", "mot_token_head_fwd")


def _desc(**kw):
    d = capi.MotTokenHeadDesc()
    d.struct_size = C.sizeof(capi.MotTokenHeadDesc)
    d.dtype, d.softcap, d.norm_in, d.n_rows, d.model_dim, d.vocab = capi.F32, capi.SOFTCAP_SIGMOID30, 1, 65536, 768, 50304
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _err():
    return capi.lib.mot_last_error().decode()


def test_struct_size_and_exports():
    assert capi.lib.mot_token_head_desc_size() == C.sizeof(capi.MotTokenHeadDesc)
    assert capi.ABI_VERSION == 13 == capi.lib.mot_version()
    for name in NAMES:
        assert name in capi.EXPORTS and hasattr(capi.lib, name), name
    assert (capi.SOFTCAP_SIGMOID30, capi.SOFTCAP_RSQRT15) == (0, 1)
    assert mot.token_head_loss is mot.functional.token_head_loss and "token_head_loss" in mot.__all__


@pytest.mark.parametrize("kw, want, msg", [
    (dict(struct_size=0), capi.MOT_EINVAL, "struct_size"),
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
def test_refusals_before_any_hip_call(kw, want, msg):
    d = _desc(**kw)
    assert capi.lib.mot_token_head_fwd(C.byref(d), None) == want
    assert msg in _err(), _err()
    assert capi.lib.mot_token_head_workspace_bytes(C.byref(d)) == 0


def test_null_pointers_and_workspace_are_refused_before_any_launch():
    d = _desc()
    assert capi.lib.mot_token_head_workspace_bytes(C.byref(d)) > 0
    assert capi.lib.mot_token_head_fwd(C.byref(d), None) == capi.MOT_EINVAL and "null x" in _err()
    d.x = d.weight = d.targets = d.loss = 256   # never dereferenced: the workspace check fails first
    assert capi.lib.mot_token_head_fwd(C.byref(d), None) == capi.MOT_EWORKSPACE
    d.n_rows = 0
    assert capi.lib.mot_token_head_fwd(C.byref(d), None) == capi.MOT_ESHAPE and "no rows" in _err()


def test_workspace_query():
    ws = lambda **kw: capi.lib.mot_token_head_workspace_bytes(C.byref(_desc(**kw)))
    V, D = 50304, 768
    # the loss alone: the chunk's logits and the per-row terms
    assert V * 4 * 128 <= ws(chunk_rows=128) < V * 4 * 128 + (1 << 20)
    assert ws(chunk_rows=128) < ws(chunk_rows=256) < ws(chunk_rows=1024)
    assert ws(chunk_rows=256) - ws(chunk_rows=128) == V * 4 * 128
    # with dx: u of the chunk in fp32; in bf16 the logits halve and the k-major copy of W joins
    assert ws(chunk_rows=128, dx=256) - ws(chunk_rows=128) == 128 * D * 4
    assert ws(chunk_rows=128, dx=256, dtype=capi.BF16) - ws(chunk_rows=128, dtype=capi.BF16) == 128 * D * 4 + V * D * 2
    assert V * 2 * 128 <= ws(chunk_rows=128, dtype=capi.BF16) < V * 2 * 128 + (1 << 20)
    # the library's choice (mot.h): the largest multiple of 256 rows whose logits and u stay below 512 MiB
    for dt, e in ((capi.F32, 4), (capi.BF16, 2)):
        rows = (512 << 20) // (V * e + D * 4) // 256 * 256
        assert rows == (2560 if e == 4 else 5120)
        assert ws(dtype=dt, dx=256) == ws(dtype=dt, dx=256, chunk_rows=rows)
    # a chunk never exceeds the rows there are
    assert ws(n_rows=40, vocab=384, model_dim=64) == ws(n_rows=40, vocab=384, model_dim=64, chunk_rows=64) < 40 * 384 * 4 + 8192
    assert ws(n_rows=0) == 0


def test_cpu_tensors_are_refused():
    x, w, t = tr.case_inputs("sigmoid30", True)
    with pytest.raises(RuntimeError, match="HIP device only"):
        mot.token_head_loss(x, w, t)
    with pytest.raises(RuntimeError, match="HIP device only"):
        mot.token_head_loss(x.requires_grad_(True), w, t.int(), softcap="rsqrt15", norm_in=False)


def test_arguments_are_named_in_the_errors():
    x, w, t = tr.case_inputs("sigmoid30", True)
    with pytest.raises(TypeError, match="token_head_loss: x must be float32 or bfloat16"):
        mot.token_head_loss(x.half(), w, t)
    with pytest.raises(ValueError, match="softcap must be 'sigmoid30' or 'rsqrt15'"):
        mot.token_head_loss(x, w, t, softcap="tanh")
    with pytest.raises(ValueError, match="weight must be"):
        mot.token_head_loss(x, w[:, :32], t)
    with pytest.raises(TypeError, match="targets must be int64 or int32"):
        mot.token_head_loss(x, w, t.float())


def test_noop_mixout_exposes_the_token_head():
    bp = ByteHyperparameters(bytes_per_token=16, byte_mixout_method="noop")
    m = ByteMixout(ModelDims(model_dim=64), 1024, bp)
    x, w, t = tr.case_inputs("sigmoid30", True)
    lm = CastedLinear(64, 384)
    with pytest.raises(RuntimeError, match="HIP device only"):   # the fused call is reached: no NotImplementedError any more
        m.loss(x[None], lm, t[None])


@pytest.mark.parametrize("kind", tr.SOFTCAPS)
@pytest.mark.parametrize("norm_in", [True, False])
def test_restatement_reproduces_reference_float64(kind, norm_in):
    x, w, t = tr.case_inputs(kind, norm_in)
    r = tr.head(x, w, t, kind, norm_in, torch.float64)
    for what in ("loss", "dx", "dW"):
        ref = GOLDEN[tr.case_key(kind, norm_in, "f64", what)]
        got = r[what].numpy()
        assert got.shape == ref.shape, what
        assert np.abs(got - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1e-300), what


@pytest.mark.parametrize("kind", tr.SOFTCAPS)
def test_restatement_reproduces_reference_bf16(kind):
    """The eager bf16 path of the restatement is the reference's: the same ops in the same order.  Under the torch that wrote the
    fixture that means the same bits; another torch may order a reduction differently, which moves a bf16 result by one step of
    its own (2^-8 relative) at the most, a gradient element being one rounding of an fp32 sum."""
    x, w, t = tr.case_inputs(kind, True)
    r = tr.head(x, w, t, kind, True, torch.bfloat16)
    same_torch = str(GOLDEN["torch_version"]) == torch.__version__
    for what in ("loss", "dx", "dW"):
        ref = GOLDEN[tr.case_key(kind, True, "bf16", what)].astype(np.float64)
        got = r[what].numpy()
        if same_torch:
            assert np.array_equal(got, ref), what
        else:
            assert (np.abs(got - ref) <= 2.0 ** -8 * np.abs(ref) + 2.0 ** -16 * np.abs(ref).max()).all(), what


def test_fixture_inputs_cover_the_target_edges_and_the_curved_part():
    for kind in tr.SOFTCAPS:
        x, w, t = tr.case_inputs(kind, True)
        assert (x.shape, w.shape, t.shape) == ((40, 64), (384, 64), (40,))
        assert {0, 299, 383} <= set(t.tolist())
        l = torch.nn.functional.rms_norm(x.double(), (64,)) @ w.double().T
        assert 8 < l.std().item() < 16
    assert str(GOLDEN["torch_version"])
