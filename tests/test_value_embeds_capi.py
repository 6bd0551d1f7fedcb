"""CPU checks of the token value embeddings (mot_value_embeds_fwd / _bwd; scaled-pre-train/train_gpt.py:566, 600 and
modded-nanogpt/runs/71_*_toks-valemb.py:247, 303): the new symbols and structs, the C ABI's validation table (argument checks run
before any HIP call, so no GPU is needed), the module surface of ValueEmbeds, and the plain-torch restatement
(tests/value_embeds_ref.py) against the reference's own float64 gradients in tests/golden/value_embeds.npz."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch
from torch import nn

import value_embeds_ref as vr
import mixture_of_tokenizers_amd as mot
from mixture_of_tokenizers_amd import _capi as capi
from mixture_of_tokenizers_amd import functional as Fm
from mixture_of_tokenizers_amd import modules as M

GOLDEN = vr.load_golden()
PTR = 64   # never dereferenced: validation fails first
SYMBOLS = ("mot_value_embeds_desc_size", "mot_value_embeds_bwd_workspace_bytes", "mot_value_embeds_fwd", "mot_value_embeds_bwd")
HEADER = Path(__file__).resolve().parents[1] / "include" / "mot.h"


def _desc(tables=None, outs=None, **kw):
    """A valid descriptor of the training scripts' shape (three 50 257 x 1024 tables) with fake pointers and an empty batch, which a
    valid descriptor answers with MOT_OK without a launch; tables / outs = {index: pointer}."""
    d = capi.MotValueEmbedsDesc()
    d.struct_size = C.sizeof(capi.MotValueEmbedsDesc)
    d.dtype = capi.F32
    d.n_tokens, d.tokens, d.tok_rows, d.dim, d.n_tables = 0, PTR, 50257, 1024, 3
    for j in range(4):
        d.tables[j] = d.outs[j] = PTR
    for k, v in kw.items():
        setattr(d, k, v)
    for j, v in (tables or {}).items():
        d.tables[j] = v
    for j, v in (outs or {}).items():
        d.outs[j] = v
    return d


def _grads(d, **kw):
    g = capi.MotValueEmbedsGrads()
    g.struct_size = C.sizeof(capi.MotValueEmbedsGrads)
    for j in range(4):
        g.grad_outs[j] = g.d_tables[j] = PTR
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def _rc(d):
    return capi.lib.mot_value_embeds_fwd(C.byref(d), None), capi.lib.mot_value_embeds_bwd(C.byref(d), C.byref(_grads(d)), None)


def test_abi_version_and_new_symbols():
    assert capi.ABI_VERSION == 13 == capi.lib.mot_version()
    header = HEADER.read_text()
    for s in SYMBOLS:
        assert s in capi.EXPORTS and getattr(capi.lib, s) is not None
        assert re.search(rf"\b{s}\(", header), s
    assert capi.lib.mot_value_embeds_desc_size() == C.sizeof(capi.MotValueEmbedsDesc)
    assert "MotValueEmbedsDesc" in header and "MotValueEmbedsGrads" in header
    assert sorted(Fm._MODES) == ["concat", "concat_linear", "mean", "noop", "sum"]            # no new mode: new symbols instead
    assert mot.value_embeds is Fm.value_embeds and mot.ValueEmbeds is M.ValueEmbeds
    assert "value_embeds" in mot.__all__ and "ValueEmbeds" in mot.__all__ and callable(Fm.value_embeds_backward)


def test_valid_descriptors_pass_validation():
    for kw in (dict(), dict(dtype=capi.BF16), dict(n_tables=1), dict(n_tables=4), dict(dim=4), dict(dtype=capi.BF16, dim=8), dict(dim=2048),
               dict(tok_rows=(1 << 21) - 2), dict(tok_rows=1)):
        assert _rc(_desc(**kw)) == (capi.MOT_OK, capi.MOT_OK), (kw, capi.lib.mot_last_error())


@pytest.mark.parametrize("kw, want, says", [
    (dict(struct_size=0), capi.MOT_EINVAL, b"struct_size 0"),
    (dict(n_tables=0), capi.MOT_EUNSUPPORTED, b"n_tables 0"),
    (dict(n_tables=5), capi.MOT_EUNSUPPORTED, b"n_tables 5"),
    (dict(dim=6), capi.MOT_EUNSUPPORTED, b"dim 6"),                                 # no multiple of the 16-byte vector
    (dict(dtype=capi.BF16, dim=12), capi.MOT_EUNSUPPORTED, b"multiple of 8"),       # 12 fp32 elements are 48 bytes, 12 bf16 are 24
    (dict(dim=2052), capi.MOT_EUNSUPPORTED, b"dim 2052"),
    (dict(dtype=5), capi.MOT_EINVAL, b"bad dtype 5"),
    (dict(tok_rows=1 << 21), capi.MOT_EUNSUPPORTED, b"2097152 rows"),                # the token order's limit
    (dict(tok_rows=(1 << 21) - 1), capi.MOT_EUNSUPPORTED, b"2097151 rows"),
])
def test_refusals_without_gpu(kw, want, says):
    """Every refusal comes back before any launch -- with a non-empty batch too (the pointers are fake) -- its message starts with
    the call's name, and the workspace query returns 0 for a descriptor that the shape rules refuse."""
    for n_tokens in (0, 128):
        d = _desc(n_tokens=n_tokens, **kw)
        assert _rc(d) == (want, want), capi.lib.mot_last_error()
        msg = capi.lib.mot_last_error()
        assert says in msg and msg.startswith(b"value_embeds"), msg
        assert capi.lib.mot_value_embeds_bwd_workspace_bytes(C.byref(d)) == 0


def test_null_pointers_are_invalid_arguments():
    fwd, bwd = capi.lib.mot_value_embeds_fwd, capi.lib.mot_value_embeds_bwd
    assert fwd(None, None) == capi.MOT_EINVAL and capi.lib.mot_last_error().startswith(b"value_embeds")
    assert bwd(None, None, None) == capi.MOT_EINVAL
    assert capi.lib.mot_value_embeds_bwd_workspace_bytes(None) == 0
    for n_tokens in (0, 128):
        d = _desc(n_tokens=n_tokens)
        assert bwd(C.byref(d), None, None) == capi.MOT_EINVAL and b"grads" in capi.lib.mot_last_error()
        assert bwd(C.byref(d), C.byref(_grads(d, struct_size=4)), None) == capi.MOT_EINVAL
        assert fwd(C.byref(_desc(n_tokens=n_tokens, tokens=None)), None) == capi.MOT_EINVAL and b"null tokens" in capi.lib.mot_last_error()
        assert fwd(C.byref(_desc(n_tokens=n_tokens, tables={1: None})), None) == capi.MOT_EINVAL and b"table 1" in capi.lib.mot_last_error()
        assert fwd(C.byref(_desc(n_tokens=n_tokens, outs={2: None})), None) == capi.MOT_EINVAL and b"table 2" in capi.lib.mot_last_error()
        g = _grads(d)
        g.d_tables[0] = None                                                      # a gradient is asked for and has nowhere to go
        assert bwd(C.byref(d), C.byref(g), None) == capi.MOT_EINVAL and b"null d_table" in capi.lib.mot_last_error()
    d = _desc(n_tokens=128)
    assert bwd(C.byref(d), C.byref(_grads(d)), None) == capi.MOT_EWORKSPACE      # a backward without its workspace is refused, not run
    d = _desc(n_tokens=128, n_tables=3, tables={3: None}, outs={3: None})         # an unused entry is not looked at
    assert capi.lib.mot_value_embeds_fwd(C.byref(_desc(n_tables=3, tables={3: None}, outs={3: None})), None) == capi.MOT_OK
    g = _grads(d)
    g.grad_outs[1] = g.d_tables[1] = None                                         # a skipped table needs no buffer
    assert bwd(C.byref(_desc()), C.byref(g), None) == capi.MOT_OK


def test_empty_batch_is_a_no_op_and_workspace_query():
    d = _desc()
    assert _rc(d) == (capi.MOT_OK, capi.MOT_OK)
    assert capi.lib.mot_value_embeds_bwd_workspace_bytes(C.byref(d)) == 0
    d = _desc(n_tokens=65536)
    need = capi.lib.mot_value_embeds_bwd_workspace_bytes(C.byref(d))
    # the token order, the positions again, and two fp32 pieces per 64 sorted positions and table
    assert need >= 4 * capi.lib.mot_token_order_ints(65536, 50257) + 4 * 65536 + (65536 // 64) * 2 * 3 * 1024 * 4
    assert need <= 64 << 20
    assert capi.lib.mot_value_embeds_bwd_workspace_bytes(C.byref(_desc(n_tokens=65536, tables={0: None}, outs={0: None}))) == need   # not read by the backward


def test_functional_refuses_cpu_tensors_and_bad_arguments():
    T3 = [torch.zeros(50, 8) for _ in range(3)]
    tok = torch.zeros(2, 6, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="HIP device only"):
        mot.value_embeds(tok, T3)
    with pytest.raises(RuntimeError, match="HIP device only"):
        Fm.value_embeds_backward([torch.zeros(2, 6, 8)] * 3, tok, T3)
    with pytest.raises(RuntimeError, match="HIP device only"):
        M.ValueEmbeds(50, 8)(tok)


def test_value_embeds_module_surface():
    class Model(nn.Module):
        def __init__(self):
            super().__init__()
            self.value_embeds = M.ValueEmbeds(50, 16)

    m = Model()
    sd = m.state_dict()
    assert list(sd) == [f"value_embeds.{j}.weight" for j in range(3)]                       # train_gpt.py:566's keys
    assert all(tuple(v.shape) == (50, 16) and v.dtype == torch.float32 for v in sd.values())
    assert isinstance(m.value_embeds, nn.ModuleList) and len(m.value_embeds) == 3
    assert all(type(e) is nn.Embedding for e in m.value_embeds)
    assert sum(p.numel() for p in m.value_embeds.parameters()) == 3 * 50 * 16                # train_gpt.py:1135
    ref = nn.ModuleList([nn.Embedding(50, 16) for _ in range(3)])
    m.value_embeds.load_state_dict(ref.state_dict())                                         # a reference checkpoint loads
    assert torch.equal(m.value_embeds[1].weight, ref[1].weight)
    for sub in m.modules():                                                                   # the training scripts' cast loop
        if isinstance(sub, nn.Embedding):
            sub.bfloat16()
    assert all(e.weight.dtype == torch.bfloat16 for e in m.value_embeds)
    assert len(M.ValueEmbeds(50, 16, n=1)) == 1 and len(M.ValueEmbeds(50, 16, n=4)) == 4
    for n in (0, 5):
        with pytest.raises(ValueError, match="1..4"):
            M.ValueEmbeds(50, 16, n=n)


@pytest.mark.parametrize("name", list(vr.CASES))
def test_restatement_reproduces_reference(name):
    vocab, dim, shape, n, kind, seed = vr.CASES[name]
    toks = GOLDEN[vr.key(name, "tokens")]
    np.testing.assert_array_equal(toks, vr.case_tokens(name))
    assert toks.shape == tuple(shape) and toks.min() >= 0 and toks.max() < vocab
    tables, gs = vr.case_inputs(name)
    r64 = vr.run(toks, tables, gs, dtype=torch.float64)
    for j in range(n):
        ref = GOLDEN[vr.key(name, f"f64/d_table{j}")]
        assert r64["d_table"][j].shape == ref.shape == (vocab, dim)
        err = vr.rel_err(r64["d_table"][j], ref)
        print(f"{name} d_table{j}: restatement vs reference float64 {err:.2e}")
        assert err <= 1e-15, (j, err)
        np.testing.assert_array_equal(r64["out"][j], tables[j][toks])                        # the forward is a copy
        absent = np.setdiff1d(np.arange(vocab), toks)
        assert not ref[absent].any()
        assert float(GOLDEN[vr.key(name, f"f32err/d_table{j}")]) <= 2e-6                     # the reference's own float32 run, a factor ten inside the bar
        assert float(GOLDEN[vr.key(name, f"bf16err/d_table{j}")]) < 0.05


def test_fixture_covers_the_listed_kinds_and_stays_small():
    kinds = {c[4] for c in vr.CASES.values()}
    assert {"uniform", "skewed", "hot", "ends"} <= kinds
    hot = GOLDEN[vr.key("v10_d8_hot", "tokens")]
    assert (hot == 3).sum() >= hot.size - 10
    ends = GOLDEN[vr.key("v100_d32_ends", "tokens")]
    assert ends.shape == (3, 50) and set(np.unique(ends)) == {0, 99}
    assert vr.GOLDEN.stat().st_size <= 64 << 10
    assert str(GOLDEN["torch_version"])
