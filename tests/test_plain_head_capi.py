"""CPU checks of the plain cross-entropy head: the C ABI's struct, every refusal and the workspace query (no GPU needed), the
package surface, window_targets against the reference's slicing, and the float64 restatement (tests/plain_head_ref.py) against the
reference's own outputs in tests/golden/plain_head.npz."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mixture_of_tokenizers_amd as mot
import plain_head_ref as pr
from mixture_of_tokenizers_amd import _capi as capi
from mixture_of_tokenizers_amd.modules import PlainLMHead

GOLDEN = np.load(Path(__file__).parent / "golden" / "plain_head.npz")
NAMES = ("mot_plain_head_desc_size", "mot_plain_head_workspace_bytes", "mot_plain_head_fwd", "mot_plain_head_eval")
CASES = [(k, v) for k in pr.KINDS for v in pr.VOCABS]


def _desc(**kw):
    d = capi.MotPlainHeadDesc()
    d.struct_size = C.sizeof(capi.MotPlainHeadDesc)
    d.dtype, d.norm_in, d.n_rows, d.model_dim, d.vocab, d.ignore_index = capi.F32, 1, 65536, 768, 50304, -100
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _out(**kw):
    o = capi.MotHeadEvalOut()
    o.struct_size = C.sizeof(capi.MotHeadEvalOut)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _err():
    return capi.lib.mot_last_error().decode()


def test_struct_size_and_exports():
    assert capi.lib.mot_plain_head_desc_size() == C.sizeof(capi.MotPlainHeadDesc)
    assert capi.ABI_VERSION == 13 == capi.lib.mot_version()   # new symbols only
    for name in NAMES:
        assert name in capi.EXPORTS and hasattr(capi.lib, name), name
    for name in ("plain_head_loss", "plain_head_eval", "window_targets"):
        assert getattr(mot, name) is getattr(mot.functional, name) and name in mot.__all__
    assert mot.PlainLMHead is PlainLMHead and "PlainLMHead" in mot.__all__


REFUSALS = [
    (dict(struct_size=0), capi.MOT_EINVAL, "struct_size"),
    (dict(vocab=50257), capi.MOT_EUNSUPPORTED, "vocab 50257 must be a multiple of 128"),
    (dict(vocab=14), capi.MOT_EUNSUPPORTED, "vocab 14 must be a multiple of 128"),   # the digit head stays out of scope
    (dict(vocab=262144 + 128), capi.MOT_EUNSUPPORTED, "at most 262144"),
    (dict(model_dim=1000), capi.MOT_EUNSUPPORTED, "model_dim 1000 must be a multiple of 16"),
    (dict(model_dim=4096), capi.MOT_EUNSUPPORTED, "at most 2048"),
    (dict(model_dim=0), capi.MOT_ESHAPE, "model_dim 0"),
    (dict(dtype=5), capi.MOT_EUNSUPPORTED, "dtype 5"),
    (dict(chunk_rows=100), capi.MOT_ESHAPE, "chunk_rows 100 must be 0"),
    (dict(chunk_rows=-32), capi.MOT_ESHAPE, "chunk_rows -32"),
    (dict(chunk_rows=1 << 16), capi.MOT_EUNSUPPORTED, "exceeds 2^31"),
    (dict(n_rows=-1), capi.MOT_ESHAPE, "n_rows -1"),
    (dict(group_rows=-1), capi.MOT_ESHAPE, "group_rows -1"),
    (dict(group_rows=1000), capi.MOT_ESHAPE, "group_rows 1000 must be 0 (no groups) or divide n_rows 65536"),
]


@pytest.mark.parametrize("kw, want, msg", REFUSALS)
def test_refusals_before_any_hip_call(kw, want, msg):
    d = _desc(**kw)
    assert capi.lib.mot_plain_head_fwd(C.byref(d), None) == want
    assert _err().startswith("mot_plain_head_fwd: ") and msg in _err(), _err()
    assert capi.lib.mot_plain_head_eval(C.byref(d), C.byref(_out()), None) == want
    assert _err().startswith("mot_plain_head_eval: ") and msg in _err(), _err()
    assert capi.lib.mot_plain_head_workspace_bytes(C.byref(d)) == 0


def test_null_pointers_and_workspace_are_refused_before_any_launch():
    assert capi.lib.mot_plain_head_fwd(None, None) == capi.MOT_EINVAL and "null descriptor" in _err()
    assert capi.lib.mot_plain_head_workspace_bytes(None) == 0
    d = _desc()
    need = capi.lib.mot_plain_head_workspace_bytes(C.byref(d))
    assert need > 0
    assert capi.lib.mot_plain_head_fwd(C.byref(d), None) == capi.MOT_EINVAL and "null x" in _err()
    d.x = d.weight = d.targets = d.loss = 256   # never dereferenced: the workspace check fails first
    assert capi.lib.mot_plain_head_fwd(C.byref(d), None) == capi.MOT_EWORKSPACE and str(need) in _err()
    d.workspace, d.workspace_bytes = 256, need - 1
    assert capi.lib.mot_plain_head_fwd(C.byref(d), None) == capi.MOT_EWORKSPACE and str(need) in _err()
    d.workspace, d.workspace_bytes = 264, need
    assert capi.lib.mot_plain_head_fwd(C.byref(d), None) == capi.MOT_EUNSUPPORTED and "16-byte aligned" in _err()
    d.n_rows = 0
    assert capi.lib.mot_plain_head_fwd(C.byref(d), None) == capi.MOT_ESHAPE and "no rows" in _err()
    assert capi.lib.mot_plain_head_workspace_bytes(C.byref(d)) == 0


def test_evaluation_refusals():
    d = _desc()
    fn = capi.lib.mot_plain_head_eval
    assert fn(C.byref(d), None, None) == capi.MOT_EINVAL and _err().startswith("mot_plain_head_eval: null out struct")
    assert fn(C.byref(d), C.byref(_out(struct_size=4)), None) == capi.MOT_EINVAL and "out struct_size" in _err()
    assert fn(C.byref(d), C.byref(_out(reserved=1)), None) == capi.MOT_EINVAL and "reserved" in _err()
    assert fn(C.byref(d), C.byref(_out(counts=256)), None) == capi.MOT_EINVAL and "counts needs pred" in _err()
    assert fn(C.byref(d), C.byref(_out(pred=258)), None) == capi.MOT_EINVAL and "aligned" in _err()
    d.dx = 256
    assert fn(C.byref(d), C.byref(_out()), None) == capi.MOT_EINVAL and "forms no gradients" in _err()


def test_workspace_query_and_the_chunk_rule():
    ws = lambda **kw: capi.lib.mot_plain_head_workspace_bytes(C.byref(_desc(**kw)))
    V, D = 50304, 768
    assert V * 4 * 128 <= ws(chunk_rows=128) < V * 4 * 128 + (1 << 20)
    assert ws(chunk_rows=256) - ws(chunk_rows=128) == V * 4 * 128
    # with dx: u of the chunk in fp32; in bf16 the logits halve and the k-major copy of W joins
    assert ws(chunk_rows=128, dx=256) - ws(chunk_rows=128) == 128 * D * 4
    assert ws(chunk_rows=128, dx=256, dtype=capi.BF16) - ws(chunk_rows=128, dtype=capi.BF16) == 128 * D * 4 + V * D * 2
    assert V * 2 * 128 <= ws(chunk_rows=128, dtype=capi.BF16) < V * 2 * 128 + (1 << 20)
    # the library's choice: the largest multiple of 256 rows whose logits and u stay below 512 MiB, at both real widths
    for V, D, want in ((50304, 768, {4: 2560, 2: 5120}), (128256, 2048, {4: 1024, 2: 1792})):
        for dt, e in ((capi.F32, 4), (capi.BF16, 2)):
            rows = (512 << 20) // (V * e + D * 4) // 256 * 256
            assert rows == want[e]
            kw = dict(vocab=V, model_dim=D, dtype=dt, dx=256)
            assert ws(**kw) == ws(chunk_rows=rows, **kw) < ws(chunk_rows=rows + 256, **kw)
            assert ws(**kw) < (512 << 20) + V * D * 2 + (1 << 20)
    # a chunk never exceeds the rows there are; group_rows and ignore_index do not change the size
    assert ws(n_rows=40, vocab=384, model_dim=64) == ws(n_rows=40, vocab=384, model_dim=64, chunk_rows=64) < 40 * 384 * 4 + 8192
    assert ws(group_rows=1024, ignore_index=7) == ws()
    assert ws(n_rows=0) == 0


def test_cpu_tensors_are_refused_and_arguments_named():
    x, w, y, idx = pr.case_inputs("math", 128)
    with pytest.raises(RuntimeError, match="HIP device only"):
        mot.plain_head_loss(x, w, y)
    with pytest.raises(RuntimeError, match="HIP device only"):
        mot.plain_head_eval(x, w, y, group_rows=pr.T)
    with pytest.raises(RuntimeError, match="HIP device only"):
        PlainLMHead(torch.nn.Linear(pr.DIM, 128, bias=False)).loss(x, y)
    with pytest.raises(TypeError, match="plain_head_loss: x must be float32 or bfloat16"):
        mot.plain_head_loss(x.half(), w, y)
    with pytest.raises(ValueError, match="weight must be"):
        mot.plain_head_loss(x, w[:, :16], y)
    with pytest.raises(TypeError, match="targets must be int64 or int32"):
        mot.plain_head_loss(x, w, y.float())
    with pytest.raises(ValueError, match="no bias"):
        PlainLMHead(torch.nn.Linear(pr.DIM, 128))


@pytest.mark.parametrize("vocab", pr.VOCABS)
def test_window_targets_is_the_reference_slicing(vocab):
    """Marking everything outside [start, end) ignored keeps exactly the rows slice_logits_and_targets cuts out, in its order, and
    the mean over them is the fixture's loss of the reference's sliced call."""
    x, w, y, idx = pr.case_inputs("math", vocab)
    wt = mot.window_targets(y, idx)
    assert wt.shape == y.shape and wt.dtype == y.dtype and wt.device == y.device
    for form in (idx.tolist(), [tuple(r) for r in idx.tolist()], idx.int()):
        assert torch.equal(mot.window_targets(y, form), wt)
    sliced = torch.cat([y[i, s:e] for i, (s, e) in enumerate(idx.tolist())])
    assert torch.equal(wt[wt != -100], sliced)
    for i, (s, e) in enumerate(idx.tolist()):
        assert (wt[i, :s] == -100).all() and (wt[i, e:] == -100).all() and torch.equal(wt[i, s:e], y[i, s:e])
    assert torch.equal(mot.window_targets(y, idx, ignore_index=-7) == -7, wt == -100)
    counts = GOLDEN[pr.case_key("math", vocab, "f64", "counts")]
    assert int((wt != -100).sum()) == counts[0] == sliced.numel()
    logits = F.linear(F.rms_norm(x.double(), (pr.DIM,)), w.double())
    loss = F.cross_entropy(logits.reshape(-1, vocab), wt.reshape(-1))
    ref = float(GOLDEN[pr.case_key("math", vocab, "f64", "loss")])
    assert abs(loss.item() - ref) <= 1e-12 * abs(ref)
    with pytest.raises(ValueError, match=r"\(B, T\)"):
        mot.window_targets(y.reshape(-1), idx)


def _fused_operands(kind, vocab):
    """What the fused call is given for a fixture case, and the float64 gradient of the reference laid out as the call's dx."""
    x, w, y, idx = pr.case_inputs(kind, vocab)
    if kind == "math":
        return x, w, mot.window_targets(y, idx), True, slice(None)
    return x[:, :-1], w, y[:, 1:], False, slice(0, -1)   # the shift of inference.py:354-355


@pytest.mark.parametrize("kind, vocab", CASES)
def test_restatement_reproduces_reference_float64(kind, vocab):
    xs, w, t, norm_in, cut = _fused_operands(kind, vocab)
    r = pr.head(xs, w, t, norm_in, torch.float64, eps=None)   # the reference's own call
    ref = {k: GOLDEN[pr.case_key(kind, vocab, "f64", k)] for k in ("loss", "dx", "dW")}
    full_dx = torch.from_numpy(ref["dx"])
    if kind == "infer":
        assert (full_dx[:, -1] == 0).all()   # the last position predicts nothing
    got = {"loss": r["loss"].numpy(), "dx": r["dx"].numpy(), "dW": r["dW"].numpy()}
    want = {"loss": ref["loss"], "dx": full_dx[:, cut].numpy(), "dW": ref["dW"]}
    for what in ("loss", "dx", "dW"):
        assert got[what].shape == want[what].shape, what
        assert np.abs(got[what] - want[what]).max() <= 1e-12 * max(np.abs(want[what]).max(), 1e-300), what


@pytest.mark.parametrize("kind, vocab", CASES)
def test_restatement_float32_is_as_close_as_the_reference_float32(kind, vocab):
    """The fixture records the reference's own float32 error against its float64 run; the restatement's float32 path is the same
    expression, so it stays within twice that (another torch may order a reduction differently) and inside the project's fixed
    fp32 bars (loss 2e-6, gradients 2e-5), which is what lets the GPU tests hold the fused call to them on these inputs."""
    xs, w, t, norm_in, cut = _fused_operands(kind, vocab)
    r64, r32 = pr.head(xs, w, t, norm_in, torch.float64, eps=None), pr.head(xs, w, t, norm_in, torch.float32, eps=None)
    own = GOLDEN[pr.case_key(kind, vocab, "f32", "err")]
    for i, (what, bar) in enumerate((("loss", 2e-6), ("dx", 2e-5), ("dW", 2e-5))):
        err = float((r32[what] - r64[what]).abs().max() / r64[what].abs().max())
        assert own[i] < bar and err <= 2 * own[i] + 1e-7, (what, err, own[i])


@pytest.mark.parametrize("vocab", pr.VOCABS)
def test_restatement_rows_and_counts_reproduce_the_reference_accuracies(vocab):
    x, w, y, idx = pr.case_inputs("math", vocab)
    wt = mot.window_targets(y, idx)
    h = x.double().reshape(-1, pr.DIM)
    c = (h.square().mean(-1) + torch.finfo(torch.float64).eps).rsqrt()   # F.rms_norm(eps=None) on float64, as the fixture's run
    row_loss, pred, rank = pr.rows(h @ w.double().T, c, wt)
    got = pr.counts(pred, wt, vocab, group_rows=pr.T)
    assert got == GOLDEN[pr.case_key("math", vocab, "f64", "counts")].tolist()
    assert 0 < got[2] < pr.B and got[1] < got[0]   # right and wrong sequences, right and wrong rows
    keep = wt.reshape(-1) != -100
    assert (rank[~keep] == -1).all() and (row_loss[~keep] == 0).all() and ((rank[keep] == 0) == (pred[keep] == wt.reshape(-1)[keep])).all()
    ref = float(GOLDEN[pr.case_key("math", vocab, "f64", "loss")])
    assert abs(float(row_loss.sum() / keep.sum()) - ref) <= 1e-12 * abs(ref)


def test_restatement_edge_semantics():
    x, w, y, _ = pr.case_inputs("infer", 128)
    xs, t = x[:, :-1].reshape(-1, pr.DIM), y[:, 1:].reshape(-1)
    none = pr.head(xs, w, torch.full_like(t, -100), False)
    assert torch.isnan(none["loss"]) and (none["dx"] == 0).all() and (none["dW"] == 0).all()
    # other out-of-range targets are dropped like ignored ones; a non-default ignore_index drops its class
    t2 = t.clone()
    t2[t == -100] = 128
    a, b = pr.head(xs, w, t, False), pr.head(xs, w, t2, False)
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["dx"], b["dx"])
    t3 = torch.where(t == -100, torch.full_like(t, 5), t)
    c = pr.head(xs, w, t3, False, ignore_index=5)
    keep = (t != -100) & (t != 5)
    ref = F.cross_entropy(xs.double() @ w.double().T, torch.where(keep, t, torch.full_like(t, -100)))
    assert abs(float(c["loss"]) - float(ref)) < 1e-12
    assert pr.counts(torch.zeros_like(t), t3, 128, ignore_index=5)[0] == int(keep.sum())
    # groups: no kept row -> not counted; all kept rows right -> counted; one wrong kept row -> not counted
    tg = torch.tensor([-100, -100, 3, -100, 3, 4, -100, 9])
    pg = torch.tensor([0, 0, 3, 7, 3, 5, 1, 9])
    assert pr.counts(pg, tg, 128, group_rows=2) == [4, 3, 2]
