"""CPU checks of run 71081's three streams in one call (modded-nanogpt/runs/71081_mot-in_toks-valemb.py:302-304, 315): the new C
symbols and the ctypes mirror of MotSplitX0Desc, the C ABI's validation table (argument checks run before any HIP call, so no GPU is
needed), and the surface of functional.split_x0 and SplitX0FrontEnd."""
import ctypes as C

import pytest
import torch

import mixture_of_tokenizers_amd as mot
from mixture_of_tokenizers_amd import _capi as capi
from mixture_of_tokenizers_amd import functional as Fm
from mixture_of_tokenizers_amd import modules as M

PTR = 64   # never dereferenced: validation fails first
NEW = ("mot_splitx_desc_size", "mot_splitx_workspace_bytes", "mot_splitx_fwd", "mot_splitx_bwd")


def _desc(**kw):
    """A valid descriptor of the run (1024 / 64 / 16, ids given) with fake pointers and an empty batch."""
    d = capi.MotSplitX0Desc()
    d.struct_size = C.sizeof(capi.MotSplitX0Desc)
    d.dtype = capi.F32
    d.n_rows, d.tokens_per_row, d.bpt = 0, 4, 16          # an empty batch: a valid descriptor returns MOT_OK without a launch
    d.tokens = d.ids = d.tok_table = d.byte_table = d.scale_tok = d.scale_byte = PTR
    d.out_x0t = d.out_x0b = d.out_x = PTR
    d.tok_rows, d.byte_rows, d.model_dim, d.byte_dim = 100, 458, 1024, 64
    d.id_source = capi.IDS_GIVEN
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _grads(**kw):
    g = capi.MotSplitX0Grads()
    g.struct_size = C.sizeof(capi.MotSplitX0Grads)
    g.grad_x0t = g.grad_x0b = g.grad_x = g.d_tok_table = g.d_byte_table = g.d_scale_tok = g.d_scale_byte = PTR
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def _rc(d, g=None):
    return capi.lib.mot_splitx_fwd(C.byref(d), None), capi.lib.mot_splitx_bwd(C.byref(d), C.byref(g or _grads()), None)


def test_new_symbols_are_exported_and_the_abi_version_stays():
    for name in NEW:
        assert name in capi.EXPORTS and hasattr(capi.lib, name), name
    assert capi.ABI_VERSION == 13 == capi.lib.mot_version()
    assert capi.lib.mot_splitx_desc_size() == C.sizeof(capi.MotSplitX0Desc)
    assert mot.split_x0 is Fm.split_x0 and mot.SplitX0FrontEnd is M.SplitX0FrontEnd
    assert "split_x0" in mot.__all__ and "SplitX0FrontEnd" in mot.__all__


def test_valid_descriptors_pass_validation():
    for kw in (dict(), dict(dtype=capi.BF16), dict(out_x0t=None), dict(out_x0t=None, out_x0b=None), dict(out_x=None, out_x0b=None),
               dict(model_dim=64, byte_dim=4), dict(model_dim=96, byte_dim=24, bpt=4), dict(model_dim=2048, byte_dim=128),
               dict(dtype=capi.BF16, model_dim=768, byte_dim=48), dict(tok_rows=1 << 21),
               dict(id_source=capi.IDS_FROM_TTB, ids=None, ttb=PTR, ttb_rows=100, ttb_elem_bytes=2, pull_dir=capi.PULL_LEFT)):
        d = _desc(**kw)
        assert capi.lib.mot_splitx_fwd(C.byref(d), None) == capi.MOT_OK, (kw, capi.lib.mot_last_error())
        if d.id_source == capi.IDS_GIVEN and d.tok_rows < (1 << 21) - 1:
            assert capi.lib.mot_splitx_bwd(C.byref(d), C.byref(_grads()), None) == capi.MOT_OK, (kw, capi.lib.mot_last_error())


@pytest.mark.parametrize("kw, want, says", [
    (dict(model_dim=1000), capi.MOT_EUNSUPPORTED, b"model_dim 1000 != bpt*byte_dim = 16*64"),
    (dict(bpt=8), capi.MOT_EUNSUPPORTED, b"model_dim 1024 != bpt*byte_dim = 8*64"),
    (dict(model_dim=96, byte_dim=6), capi.MOT_EUNSUPPORTED, b"byte_dim 6 must be a multiple of 4"),
    (dict(dtype=capi.BF16, model_dim=64, byte_dim=4), capi.MOT_EUNSUPPORTED, b"byte_dim 4 must be a multiple of 8"),
    (dict(model_dim=2112, byte_dim=132), capi.MOT_EUNSUPPORTED, b"model_dim 2112 above 2048"),
    (dict(bpt=0), capi.MOT_EUNSUPPORTED, b"bytes_per_token 0 outside [1, 64]"),
    (dict(bpt=65, model_dim=260, byte_dim=4), capi.MOT_EUNSUPPORTED, b"bytes_per_token 65 outside [1, 64]"),
    (dict(dtype=2), capi.MOT_EUNSUPPORTED, b"dtype 2 is not built"),
    (dict(id_source=capi.IDS_NONE), capi.MOT_EINVAL, b"bad id_source 0"),
    (dict(struct_size=8), capi.MOT_EINVAL, b"struct_size"),
    (dict(ids=None), capi.MOT_EINVAL, b"ids missing"),
    (dict(tokens=None), capi.MOT_EINVAL, b"tokens"),
    (dict(tok_table=None), capi.MOT_EINVAL, b"null tok_table or byte_table"),
    (dict(byte_table=None), capi.MOT_EINVAL, b"null tok_table or byte_table"),
    (dict(scale_tok=None), capi.MOT_EINVAL, b"null scale_tok or scale_byte"),
    (dict(scale_byte=None), capi.MOT_EINVAL, b"null scale_tok or scale_byte"),
    (dict(out_ids_pulled=PTR), capi.MOT_EINVAL, b"MOT_IDS_FROM_TTB"),
    (dict(tok_table=PTR + 4), capi.MOT_EINVAL, b"16-byte aligned"),
])
def test_refusals_come_back_before_any_launch(kw, want, says):
    """With a non-empty batch too: the pointers are fake, so a launch would fault."""
    for n_rows in (0, 2):
        d = _desc(n_rows=n_rows, **dict(kw))
        assert _rc(d) == (want, want), capi.lib.mot_last_error()
        assert says in capi.lib.mot_last_error(), capi.lib.mot_last_error()
        if kw.keys() & {"model_dim", "byte_dim", "dtype", "id_source", "bpt", "struct_size"}:   # what a size query can see
            assert capi.lib.mot_splitx_workspace_bytes(C.byref(d), 0) == 0
            assert capi.lib.mot_splitx_workspace_bytes(C.byref(d), 1) == 0


def test_all_outputs_or_all_gradients_null():
    for n_rows in (0, 2):
        d = _desc(n_rows=n_rows, out_x0t=None, out_x0b=None, out_x=None)
        assert capi.lib.mot_splitx_fwd(C.byref(d), None) == capi.MOT_EUNSUPPORTED
        assert b"all null" in capi.lib.mot_last_error()
        assert capi.lib.mot_splitx_bwd(C.byref(_desc(n_rows=n_rows)), C.byref(_grads(grad_x0t=None, grad_x0b=None, grad_x=None)), None) == capi.MOT_EUNSUPPORTED
        assert b"all null" in capi.lib.mot_last_error()
    # the backward reads no output, and any one gradient will do; any result may be unwanted
    d = _desc(out_x0t=None, out_x0b=None, out_x=None)
    for g in (_grads(grad_x0t=None, grad_x=None), _grads(grad_x0b=None), _grads(d_tok_table=None, d_scale_byte=None),
              _grads(d_tok_table=None, d_byte_table=None, d_scale_tok=None, d_scale_byte=None)):
        assert capi.lib.mot_splitx_bwd(C.byref(d), C.byref(g), None) == capi.MOT_OK, capi.lib.mot_last_error()


def test_bad_pull_direction_and_table_source():
    ttb = dict(id_source=capi.IDS_FROM_TTB, ids=None, ttb=PTR, ttb_rows=100, ttb_elem_bytes=2, pull_dir=capi.PULL_LEFT)
    for n_rows in (0, 2):
        for kw, says in ((dict(pull_dir=3), b"bad pull_dir 3"), (dict(pull_dir=-1), b"bad pull_dir -1"), (dict(ttb_elem_bytes=8), b"ttb_elem_bytes"),
                         (dict(ttb=None), b"ttb missing")):
            d = _desc(n_rows=n_rows, **{**ttb, **kw})
            assert capi.lib.mot_splitx_fwd(C.byref(d), None) == capi.MOT_EINVAL
            assert says in capi.lib.mot_last_error(), capi.lib.mot_last_error()
    d = _desc(**ttb)   # the backward takes the ids the forward used
    assert capi.lib.mot_splitx_bwd(C.byref(d), C.byref(_grads()), None) == capi.MOT_EUNSUPPORTED
    assert capi.lib.mot_splitx_workspace_bytes(C.byref(d), 1) == 0


def test_the_token_orders_limit_counts_only_where_a_token_gradient_is_asked_for():
    for n_rows in (0, 2):
        d = _desc(n_rows=n_rows, tok_rows=(1 << 21) - 1)
        assert capi.lib.mot_splitx_bwd(C.byref(d), C.byref(_grads()), None) == capi.MOT_EUNSUPPORTED
        assert b"token order's limit" in capi.lib.mot_last_error()
    assert capi.lib.mot_splitx_bwd(C.byref(_desc(tok_rows=(1 << 21) - 1)), C.byref(_grads(d_tok_table=None)), None) == capi.MOT_OK
    assert capi.lib.mot_splitx_bwd(C.byref(_desc(tok_rows=(1 << 21) - 2)), C.byref(_grads()), None) == capi.MOT_OK


def test_backward_wants_its_grads_struct():
    d = _desc(n_rows=2)
    assert capi.lib.mot_splitx_bwd(C.byref(d), None, None) == capi.MOT_EINVAL
    g = _grads()
    g.struct_size = 8
    assert capi.lib.mot_splitx_bwd(C.byref(d), C.byref(g), None) == capi.MOT_EINVAL
    assert capi.lib.mot_splitx_bwd(C.byref(d), C.byref(_grads(grad_x=PTR + 8)), None) == capi.MOT_EINVAL
    assert b"16-byte aligned" in capi.lib.mot_last_error()


def test_workspace_queries_and_a_call_without_its_workspace():
    d = _desc(n_rows=2, tokens_per_row=64)
    fwd, bwd = capi.lib.mot_splitx_workspace_bytes(C.byref(d), 0), capi.lib.mot_splitx_workspace_bytes(C.byref(d), 1)
    assert 458 * 4 <= fwd < 458 * 4 + 256                                             # the byte rows' rms factors, nothing else
    assert bwd >= fwd + 128 * 1024 * 4 + 128 * 1024 * 4                               # d a of the batch, d u of the slab
    assert capi.lib.mot_splitx_workspace_bytes(C.byref(_desc()), 0) == 0 == capi.lib.mot_splitx_workspace_bytes(C.byref(_desc()), 1)   # an empty batch
    # refused, not run: the pointers are fake
    for ws, ws_bytes in ((None, 0), (PTR, 0), (PTR, fwd - 1), (PTR + 4, fwd)):
        d.workspace, d.workspace_bytes = ws, ws_bytes
        assert capi.lib.mot_splitx_fwd(C.byref(d), None) == capi.MOT_EWORKSPACE
        assert str(fwd).encode() in capi.lib.mot_last_error()
    for ws, ws_bytes in ((None, 0), (PTR, fwd), (PTR, bwd - 1)):
        d.workspace, d.workspace_bytes = ws, ws_bytes
        assert capi.lib.mot_splitx_bwd(C.byref(d), C.byref(_grads()), None) == capi.MOT_EWORKSPACE
        assert str(bwd).encode() in capi.lib.mot_last_error()
    # the run's step: d u stays one slab of 16 384 positions; d a is the whole batch in fp32
    step = _desc(n_rows=1, tokens_per_row=65536, dtype=capi.BF16, tok_rows=50257)
    b = capi.lib.mot_splitx_workspace_bytes(C.byref(step), 1)
    assert 65536 * 1024 * 4 + 16384 * 1024 * 4 < b < 65536 * 1024 * 4 + 16384 * 1024 * 4 + (16 << 20)
    assert capi.lib.mot_splitx_workspace_bytes(C.byref(step), 0) < 4096


def test_module_surface():
    torch.manual_seed(0)
    m = M.SplitX0FrontEnd(token_vocab_size=50257, byte_vocab_size=458, model_dim=1024, byte_dim=64)
    sd = m.state_dict()
    assert sorted(sd) == ["embed_bytes.weight", "embed_tokens.weight", "scalars"]     # SumFrontEnd's keys; the ttb is no state
    assert sorted(sd) == sorted(M.SumFrontEnd(100, 458, 64, 4, variant="71081").state_dict())
    assert tuple(sd["embed_tokens.weight"].shape) == (50257, 1024) and tuple(sd["embed_bytes.weight"].shape) == (458, 64)
    assert isinstance(m.scalars, torch.nn.Parameter) and m.scalars.dtype == torch.float32 and m.scalars.tolist() == [0.5, 0.5]   # runs/71081_*.py:247
    assert m.bpt == 16 and (m.pad_byte, m.eot_byte) == (456, 457) and m.ttb is None
    M.SplitX0FrontEnd(50257, 458, 1024, 64).load_state_dict(sd)
    with pytest.raises(AssertionError):
        M.SplitX0FrontEnd(100, 458, 1000, 64)
    with pytest.raises(ValueError, match="byte_inputs"):
        m(torch.zeros(8, dtype=torch.int32))                                    # no ttb attached, no ids given
    with pytest.raises(ValueError, match="two elements"):
        m(torch.zeros(8, dtype=torch.int32), torch.zeros(128, dtype=torch.int64), scalars=torch.zeros(3))
    with pytest.raises(RuntimeError, match="HIP device only"):
        m(torch.zeros(8, dtype=torch.int32), torch.zeros(128, dtype=torch.int64))


def test_functional_refuses_cpu_and_mismatched_inputs():
    Et, Eb, s = torch.zeros(10, 64), torch.zeros(458, 8), torch.tensor([0.5, 0.5])
    toks, ids = torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, 32, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="HIP device only"):
        mot.split_x0(toks, Et, Eb, s[1:], s[:1], bpt=8, ids=ids)
    with pytest.raises(RuntimeError, match="HIP device only"):
        Fm.split_x0_backward(torch.zeros(1, 4, 64), None, None, toks, Et, Eb, s[1:], s[:1], bpt=8, ids=ids)
    # (shape and dtype checks: the descriptor builder runs them before anything touches a device)
    with pytest.raises(TypeError, match="share one dtype"):
        Fm._split_x0_desc(toks, Et, Eb.bfloat16(), s[1:], s[:1], 8, None, "split_x0")
    with pytest.raises(TypeError, match="float32 or bfloat16"):
        Fm._split_x0_desc(toks, Et.double(), Eb.double(), s[1:], s[:1], 8, None, "split_x0")
    with pytest.raises(TypeError, match="expected torch.float32"):
        Fm._split_x0_desc(toks, Et, Eb, s[1:].bfloat16(), s[:1], 8, None, "split_x0")
    with pytest.raises(ValueError, match="one-element tensor"):
        Fm._split_x0_desc(toks, Et, Eb, s, s[:1], 8, None, "split_x0")
    with pytest.raises(ValueError, match="one-element tensor"):
        Fm._split_x0_desc(toks, Et, Eb, 0.5, s[:1], 8, None, "split_x0")
    with pytest.raises(ValueError, match="2-D"):
        Fm._split_x0_desc(toks, Et[0], Eb, s[1:], s[:1], 8, None, "split_x0")
    with pytest.raises(ValueError, match="want must name"):
        Fm._split_x0_want(("x", "y"))
    with pytest.raises(ValueError, match="want must name"):
        Fm._split_x0_want(())
    assert Fm._split_x0_want(["x", "x0t"]) == ("x", "x0t")
