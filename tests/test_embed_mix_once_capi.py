"""CPU checks of the write-once backward of the fused front-end (mot_embed_mix_bwd_once, include/mot.h): the new C symbols and the
ctypes mirror of MotEmbedMixGradsOnce, the C ABI's refusals (argument checks run before any HIP call, so no GPU is needed), the two
workspace caps, and the surface of functional.embed_mix(write_once=), SumFrontEnd and ConcatFrontEnd (write_once_grads=)."""
import ctypes as C

import pytest
import torch

import mixture_of_tokenizers_amd as mot
from mixture_of_tokenizers_amd import _capi as capi
from mixture_of_tokenizers_amd import functional as Fm
from mixture_of_tokenizers_amd import modules as M

PTR = 64   # never dereferenced: validation fails first
NEW = ("mot_embed_mix_grads_once_size", "mot_embed_mix_bwd_once_workspace_bytes", "mot_embed_mix_bwd_once")
MiB = 1 << 20


def _desc(**kw):
    """A valid SUM descriptor (1024 / 64 / 16, ids given) with fake pointers and an empty batch."""
    d = capi.MotEmbedMixDesc()
    d.struct_size = C.sizeof(capi.MotEmbedMixDesc)
    d.dtype, d.mode = capi.F32, capi.MIX_SUM
    d.n_rows, d.tokens_per_row, d.bpt = 0, 4, 16          # an empty batch: a valid descriptor returns MOT_OK without a launch
    d.tokens = d.ids_a = d.tok_table = d.byte_table = PTR
    d.tok_rows, d.byte_rows, d.tok_dim, d.model_dim, d.byte_dim = 100, 458, 1024, 1024, 64
    d.id_source = capi.IDS_GIVEN
    d.norm_out = 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _grads(**kw):
    g = capi.MotEmbedMixGradsOnce()
    g.struct_size = C.sizeof(capi.MotEmbedMixGradsOnce)
    g.grad_out = g.d_tok_table = g.d_byte_table = g.d_scale_tok = g.d_scale_byte = PTR
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def _rc(d, g=None):
    g = g or (_grads(d_byte_table=None, d_scale_byte=None) if d.mode == capi.MIX_NOOP else _grads())   # NOOP has no byte table to give a gradient
    return capi.lib.mot_embed_mix_bwd_once(C.byref(d), C.byref(g), None)


def _ws(d):
    return capi.lib.mot_embed_mix_bwd_once_workspace_bytes(C.byref(d))


NOOP = dict(mode=capi.MIX_NOOP, bpt=0, byte_dim=0, byte_rows=0, byte_table=None, ids_a=None, id_source=capi.IDS_NONE)
CONCAT = dict(mode=capi.MIX_CONCAT, tok_dim=512, byte_dim=32, model_dim=1024)


def test_new_symbols_are_exported_and_the_abi_version_stays():
    for name in NEW:
        assert name in capi.EXPORTS and hasattr(capi.lib, name), name
    assert capi.ABI_VERSION == 13 == capi.lib.mot_version()
    assert capi.lib.mot_embed_mix_grads_once_size() == C.sizeof(capi.MotEmbedMixGradsOnce) == 56
    assert callable(Fm.embed_mix_backward_once)


def test_valid_descriptors_pass_validation():
    for kw in (dict(), dict(dtype=capi.BF16), dict(norm_tok=1, norm_byte=1, scale_tok=PTR, scale_byte=PTR), dict(norm_out=0), NOOP,
               dict(NOOP, norm_tok=1, dtype=capi.BF16, tok_dim=16, model_dim=16), CONCAT, dict(CONCAT, dtype=capi.BF16),
               dict(tok_dim=2048, model_dim=2048, byte_dim=128), dict(tok_dim=32, model_dim=32, byte_dim=8, bpt=4),
               dict(tok_rows=(1 << 21) - 2)):
        assert _rc(_desc(**kw)) == capi.MOT_OK, (kw, capi.lib.mot_last_error())
    for g in (_grads(d_tok_table=None), _grads(d_byte_table=None, d_scale_tok=None), _grads(d_tok_table=None, d_byte_table=None, d_scale_tok=None, d_scale_byte=None)):
        assert _rc(_desc(), g) == capi.MOT_OK, capi.lib.mot_last_error()


@pytest.mark.parametrize("kw, follow_up", [
    (dict(mode=capi.MIX_CONCAT_LINEAR, weight=PTR), b"MOT_MIX_CONCAT_LINEAR"),
    (dict(mode=capi.MIX_CONCAT_LINEAR), b"MOT_MIX_CONCAT_LINEAR"),
    (dict(mode=capi.MIX_MEAN, byte_dim=1024, norm_out=0), b"MOT_MIX_MEAN"),
    (dict(ids_b=PTR), b"ids_b"),
    (dict(CONCAT, ids_b=PTR), b"ids_b"),
    (dict(id_source=capi.IDS_FROM_TTB, ids_a=None, ttb=PTR, ttb_rows=100, ttb_elem_bytes=2, pull_dir=capi.PULL_LEFT), b"MOT_IDS_FROM_TTB"),
])
def test_what_is_not_built_is_refused_before_any_launch(kw, follow_up):
    """With a non-empty batch too: the pointers are fake, so a launch would fault."""
    for n_rows in (0, 2):
        d = _desc(n_rows=n_rows, **dict(kw))
        assert _rc(d) == capi.MOT_EUNSUPPORTED, capi.lib.mot_last_error()
        msg = capi.lib.mot_last_error()
        assert msg.startswith(b"embed_mix_bwd_once") and follow_up in msg and b"follow-up" in msg, msg
        assert _ws(d) == 0


@pytest.mark.parametrize("kw, want, says", [
    (dict(tok_dim=1000, model_dim=1000), capi.MOT_ESHAPE, b"bpt*byte_dim == tok_dim == model_dim"),
    (dict(byte_dim=6, bpt=16, tok_dim=96, model_dim=96), capi.MOT_EUNSUPPORTED, b"byte_dim 6 must be a multiple of 4"),
    (dict(dtype=capi.BF16, byte_dim=4, tok_dim=64, model_dim=64), capi.MOT_EUNSUPPORTED, b"byte_dim 4 must be a multiple of 8"),
    (dict(tok_dim=2112, model_dim=2112, byte_dim=132), capi.MOT_EUNSUPPORTED, b"model_dim 2112 > 2048"),
    (dict(CONCAT, model_dim=1000), capi.MOT_ESHAPE, b"model_dim == tok_dim + bpt*byte_dim"),
    (dict(NOOP, model_dim=512), capi.MOT_ESHAPE, b"model_dim 512 != tok_dim 1024"),
    (dict(tok_rows=(1 << 21) - 1), capi.MOT_EUNSUPPORTED, b"token order's limit"),
    (dict(bpt=0), capi.MOT_EUNSUPPORTED, b"bytes_per_token 0 outside [1, 64]"),
    (dict(dtype=2), capi.MOT_EINVAL, b"bad dtype 2"),
    (dict(mode=7), capi.MOT_EINVAL, b"bad mode 7"),
    (dict(struct_size=8), capi.MOT_EINVAL, b"struct_size"),
])
def test_shape_refusals_and_the_size_query(kw, want, says):
    for n_rows in (0, 2):
        d = _desc(n_rows=n_rows, **dict(kw))
        assert _rc(d) == want, capi.lib.mot_last_error()
        assert capi.lib.mot_last_error().startswith(b"embed_mix_bwd_once") and says in capi.lib.mot_last_error(), capi.lib.mot_last_error()
        assert _ws(d) == 0


def test_null_pointers_and_a_bad_grads_struct():
    for n_rows in (0, 2):
        for kw, says in ((dict(tokens=None), b"tokens"), (dict(tok_table=None), b"tok_table"), (dict(byte_table=None), b"byte_table"),
                         (dict(ids_a=None), b"ids_a"), (dict(tok_table=PTR + 4), b"16-byte aligned")):
            assert _rc(_desc(n_rows=n_rows, **kw)) == capi.MOT_EINVAL, kw
            assert capi.lib.mot_last_error().startswith(b"embed_mix_bwd_once") and says in capi.lib.mot_last_error()
        d = _desc(n_rows=n_rows)
        assert _rc(d, _grads(grad_out=None)) == capi.MOT_EINVAL and b"grad_out" in capi.lib.mot_last_error()
        assert _rc(d, _grads(d_tok_table=PTR + 8)) == capi.MOT_EINVAL and b"16-byte aligned" in capi.lib.mot_last_error()
        assert _rc(d, _grads(struct_size=8)) == capi.MOT_EINVAL and b"struct_size" in capi.lib.mot_last_error()
        assert _rc(d, _grads(reserved=1)) == capi.MOT_EINVAL
        assert capi.lib.mot_embed_mix_bwd_once(C.byref(d), None, None) == capi.MOT_EINVAL
        assert capi.lib.mot_embed_mix_bwd_once(None, C.byref(_grads()), None) == capi.MOT_EINVAL
        assert _rc(_desc(n_rows=n_rows, **NOOP), _grads()) == capi.MOT_EINVAL and b"no byte table" in capi.lib.mot_last_error()
    assert capi.lib.mot_embed_mix_bwd_once_workspace_bytes(None) == 0


def test_a_call_without_its_workspace():
    d = _desc(n_rows=2, tokens_per_row=64)
    need = _ws(d)
    assert need > 0 and _ws(_desc()) == 0            # an empty batch needs none
    for ws, ws_bytes in ((None, 0), (PTR, 0), (PTR, need - 1), (PTR + 4, need)):   # refused, not run: the pointers are fake
        d.workspace, d.workspace_bytes = ws, ws_bytes
        assert _rc(d) == capi.MOT_EWORKSPACE
        assert capi.lib.mot_last_error().startswith(b"embed_mix_bwd_once") and str(need).encode() in capi.lib.mot_last_error()


def test_the_workspace_has_no_term_in_tokens_times_columns():
    """The two caps of the headline batches, and what the pieces add up to: the order and the canonical positions, 16 bytes of scalars
    per position, the slice pieces, ONE slab of the byte part, and the byte table's fixed-point sums with a word per slab."""
    head = _desc(n_rows=1, tokens_per_row=524288, tok_rows=50257, tok_dim=768, model_dim=768, byte_dim=48)
    run71 = _desc(n_rows=1, tokens_per_row=65536, tok_rows=50257)
    assert 0 < _ws(head) <= 256 * MiB
    assert 0 < _ws(run71) <= 128 * MiB
    for d, N, D, nbk in ((head, 524288, 768, 768), (run71, 65536, 1024, 1024), (_desc(n_rows=1, tokens_per_row=65536, tok_rows=50257, **CONCAT), 65536, 512, 512)):
        order = capi.lib.mot_token_order_ints(N, 50257) * 4
        pieces = (N // 64) * 2 * D * 4
        want = order + 4 * N + pieces + 16 * N + 8 * (N // 16) + 16384 * nbk * 4 + 458 * 4 + 458 * (nbk // 16) * 8 + 4 * (N // 16384)
        for dt in (capi.F32, capi.BF16):
            d.dtype = dt
            assert want <= _ws(d) < want + 4096, (N, D, _ws(d), want)
        assert _ws(d) < N * D * 4                    # less than the fp32 row buffer d a alone (1.5 GiB at the headline batch)
    # twice the tokens: only the O(N) terms and the pieces grow, the slab does not
    d2 = _desc(n_rows=2, tokens_per_row=524288, tok_rows=50257, tok_dim=768, model_dim=768, byte_dim=48)
    assert _ws(d2) - _ws(head) < _ws(head) - 16384 * 768 * 4 + 4096


def test_module_flags_and_state_dict_keys():
    torch.manual_seed(0)
    for make in (lambda **kw: M.SumFrontEnd(100, 458, 64, 4, variant="71041", **kw), lambda **kw: M.ConcatFrontEnd(100, 458, 32, 2, **kw)):
        a, b = make(), make(write_once_grads=True)
        assert a.write_once_grads is False and b.write_once_grads is True
        assert sorted(a.state_dict()) == sorted(b.state_dict())
        a.load_state_dict(b.state_dict())
        with pytest.raises(RuntimeError, match="HIP device only"):
            b(torch.zeros(8, dtype=torch.int32), torch.zeros(8 * 16, dtype=torch.int64))
    assert sorted(M.SumFrontEnd(100, 458, 64, 4, write_once_grads=True).state_dict()) == ["embed_bytes.weight", "embed_tokens.weight"]


def test_functional_refuses_cpu_tensors_and_what_the_call_does_not_build_at_forward_time():
    Et, Eb = torch.zeros(10, 64, requires_grad=True), torch.zeros(458, 8, requires_grad=True)
    toks, ids = torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, 32, dtype=torch.int64)
    for kw in (dict(mode="sum", bpt=8, ids_a=ids, norm_out=True), dict(mode="noop")):
        with pytest.raises(RuntimeError, match="HIP device only"):
            mot.embed_mix(toks, Et, None if kw["mode"] == "noop" else Eb, write_once=True, **kw)
    with pytest.raises(RuntimeError, match="HIP device only"):
        Fm.embed_mix_backward_once(torch.zeros(1, 4, 64), toks, Et.detach(), Eb.detach(), mode="sum", bpt=8, ids_a=ids, norm_out=True)
    W = torch.zeros(64, 64 + 8 * 8, requires_grad=True)
    for kw, says in ((dict(mode="concat_linear", bpt=8, ids_a=ids, weight=W), "concat_linear"), (dict(mode="mean", bpt=8, ids_a=ids), "mean"),
                     (dict(mode="sum", bpt=8, ids_a=ids, ids_b=ids), "second id tensor"),
                     (dict(mode="sum", bpt=8, ttb=torch.zeros(10, 8, dtype=torch.int16), pull="left", add_padded=True), "second id tensor")):
        with pytest.raises(NotImplementedError, match=says):       # before anything looks at the tensors' device
            mot.embed_mix(toks, Et, Eb, write_once=True, **kw)
    with pytest.raises(NotImplementedError, match="mean"):
        Fm.embed_mix_backward_once(torch.zeros(1, 4, 64), toks, Et.detach(), Eb.detach(), mode="mean", bpt=8, ids_a=ids)
    # the default leaves the existing refusals as they are
    with pytest.raises(RuntimeError, match="HIP device only"):
        mot.embed_mix(toks, Et, Eb, mode="mean", bpt=8, ids_a=ids)
