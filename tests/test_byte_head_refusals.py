"""CPU checks of the byte output head's C entry points that need no GPU: every refusal with its code and message, the order of the
pointer checks in mot_byte_head_fwd / _bwd, and the workspace query against the carve of csrc/mot_head.hip written out here."""
import ctypes as C

import pytest

from mixture_of_tokenizers_amd import _capi as capi


def _desc(**kw):
    d = capi.MotByteHeadDesc()
    d.struct_size = C.sizeof(capi.MotByteHeadDesc)
    d.method, d.dtype, d.bpt, d.n_tokens, d.model_dim, d.n_layer_out, d.vocab = capi.HEAD_SPLIT, capi.F32, 16, 8, 1024, 1, 512
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _err():
    return capi.lib.mot_last_error().decode()


@pytest.mark.parametrize("kw, want, msg", [
    (dict(struct_size=0), capi.MOT_EINVAL, "struct_size"),
    (dict(method=2), capi.MOT_EUNSUPPORTED, "method 2"),
    (dict(dtype=5), capi.MOT_EUNSUPPORTED, "dtype 5"),
    (dict(n_tokens=-1), capi.MOT_ESHAPE, ""),
    (dict(model_dim=0), capi.MOT_ESHAPE, ""),
    (dict(n_layer_out=65), capi.MOT_ESHAPE, ""),
    (dict(bpt=0), capi.MOT_ESHAPE, "bpt"),
    (dict(bpt=capi.MAX_BPT + 1), capi.MOT_ESHAPE, "bpt"),
    (dict(vocab=458), capi.MOT_EUNSUPPORTED, "only the 512-row head"),
    (dict(method=capi.HEAD_SPLIT, model_dim=1000, bpt=16), capi.MOT_ESHAPE, "split needs"),
    (dict(method=capi.HEAD_COPY, model_dim=1000), capi.MOT_EUNSUPPORTED, "row width 1000"),
    (dict(method=capi.HEAD_COPY, model_dim=4096), capi.MOT_EUNSUPPORTED, "at most 2048"),
    (dict(n_tokens=1 << 27, bpt=16), capi.MOT_EUNSUPPORTED, "exceeds 2^31"),
])
def test_refusals_before_any_hip_call(kw, want, msg):
    d = _desc(**kw)
    assert capi.lib.mot_byte_head_fwd(C.byref(d), None) == want
    assert msg in _err(), _err()
    assert capi.lib.mot_byte_head_bwd(C.byref(d), None, None, None, None) == want
    assert msg in _err(), _err()
    assert capi.lib.mot_byte_head_workspace_bytes(C.byref(d)) == 0


def test_order_of_the_forward_pointer_checks():
    fwd = lambda d: capi.lib.mot_byte_head_fwd(C.byref(d), None)
    d = _desc(x=256, weight=256, targets=256, row_stats=256)
    assert fwd(d) == capi.MOT_EINVAL and "null loss" in _err()
    d.loss, d.n_tokens = 256, 0
    assert fwd(d) == capi.MOT_ESHAPE and "no targets" in _err()
    d.n_tokens = 8
    for name in ("x", "weight", "targets", "row_stats"):
        setattr(d, name, None)
        assert fwd(d) == capi.MOT_EINVAL and "null x / weight / targets / row_stats" in _err(), name
        setattr(d, name, 256)
    assert fwd(d) == capi.MOT_EWORKSPACE   # the dummy pointers are never dereferenced: the workspace check fails first
    d.workspace, d.workspace_bytes = 256, capi.lib.mot_byte_head_workspace_bytes(C.byref(d)) - 1
    assert fwd(d) == capi.MOT_EWORKSPACE and "workspace" in _err()
    d.workspace_bytes, d.x = 1 << 40, 256 + 8
    assert fwd(d) == capi.MOT_EUNSUPPORTED and "16-byte aligned" in _err()


def test_order_of_the_backward_pointer_checks():
    d = _desc(x=256, weight=256, targets=256, row_stats=256, workspace=256, workspace_bytes=1 << 40)
    bwd = lambda go, dx, dw: capi.lib.mot_byte_head_bwd(C.byref(d), go, dx, dw, None)
    for args in ((None, 256, 256), (256, None, 256), (256, 256, None)):
        assert bwd(*args) == capi.MOT_EINVAL and "null grad_loss / dx / dW" in _err(), args
    assert bwd(256, 256 + 8, 256) == capi.MOT_EUNSUPPORTED and "dx must be 16-byte aligned" in _err()
    d.workspace_bytes = 0   # the operands' checks come before dx's alignment
    assert bwd(256, 256 + 8, 256) == capi.MOT_EWORKSPACE
    d.n_tokens = 0
    assert bwd(256, 256, 256) == capi.MOT_ESHAPE and "no targets" in _err()


@pytest.mark.parametrize("method, dtype, D, bpt, n_tokens, rows, chunk", [pytest.param(*c, id="-".join(map(str, c[:2] + c[4:]))) for c in [
    (capi.HEAD_COPY, capi.F32, 256, 16, 20000, 20000, 16384),
    (capi.HEAD_COPY, capi.BF16, 256, 16, 20000, 20000, 12288),
    (capi.HEAD_SPLIT, capi.F32, 256, 16, 1536, 24576, 23808),
    (capi.HEAD_SPLIT, capi.BF16, 256, 16, 1536, 24576, 15872),
    (capi.HEAD_SPLIT, capi.BF16, 256, 16, 40, 640, 640),   # a chunk never exceeds the rows there are
    # the widest row, K 2048, has the shortest chunk: the seams of tests/test_gpu_byte_head_edges.py, a full chunk and 37 or 38 rows
    (capi.HEAD_COPY, capi.F32, 2048, 2, 4901, 4901, 4864),
    (capi.HEAD_COPY, capi.BF16, 2048, 2, 4389, 4389, 4352),
    (capi.HEAD_SPLIT, capi.F32, 4096, 2, 2451, 4902, 4864),
    (capi.HEAD_SPLIT, capi.BF16, 4096, 2, 2195, 4390, 4352),
]])   # the ids name method, dtype and the rows, as they did before D and bpt became parameters
def test_workspace_query(method, dtype, D, bpt, n_tokens, rows, chunk):
    """The carve of mot_head.hip written out: per-row terms, the loss partials, a chunk's fp32 logits, its bf16 gradient (bf16), u,
    and the k-major bf16 weight (bf16), each rounded up to 256 bytes.  A chunk is the largest multiple of 256 rows whose pieces
    stay below 48 MiB, at least 256 and at most the rows."""
    bf = dtype == capi.BF16
    K = D if method == capi.HEAD_COPY else D // bpt
    assert rows == (n_tokens if method == capi.HEAD_COPY else n_tokens * bpt)
    per_row = 512 * 4 + (512 * 2 if bf else 0) + K * 4
    assert chunk == min(rows, max(256, (48 << 20) // per_row // 256 * 256))
    assert K < 2048 or chunk < rows < 2 * chunk   # the seam cases: two chunks, the second a short one
    up = lambda b: (b + 255) // 256 * 256
    want = up(4 * rows) + up(512 * 8) + up(chunk * 512 * 4) + up(chunk * K * 4)
    if bf:
        want += up(chunk * 512 * 2) + up(512 * K * 2)
    d = _desc(method=method, dtype=dtype, bpt=bpt, n_tokens=n_tokens, model_dim=D)
    assert capi.lib.mot_byte_head_workspace_bytes(C.byref(d)) == want
    assert capi.lib.mot_byte_head_workspace_bytes(C.byref(_desc(n_tokens=0))) == 0
