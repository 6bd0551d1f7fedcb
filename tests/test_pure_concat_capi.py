"""CPU checks of the pure-concatenation mixin (MOT_MIX_CONCAT, modded-nanogpt/runs/711_*.py:224-232): the enumerator and its
Python names, the C ABI's validation table (argument checks run before any HIP call, so no GPU is needed), the module surface of
ConcatFrontEnd, and the plain-torch restatement (tests/pure_concat_ref.py) against the reference's own float64 outputs in
tests/golden/pure_concat.npz."""
import ctypes as C

import numpy as np
import pytest
import torch

import pure_concat_ref as pc
import mixture_of_tokenizers_amd as mot
from mixture_of_tokenizers_amd import _capi as capi
from mixture_of_tokenizers_amd import functional as Fm
from mixture_of_tokenizers_amd import modules as M

GOLDEN = pc.load_golden()
PTR = 64   # never dereferenced: validation fails first


def _desc(**kw):
    """A valid run-711 descriptor (512 + 16 x 32 = 1024 columns, ids given) with fake pointers."""
    d = capi.MotEmbedMixDesc()
    d.struct_size = C.sizeof(capi.MotEmbedMixDesc)
    d.dtype, d.mode = capi.F32, capi.MIX_CONCAT
    d.n_rows, d.tokens_per_row, d.bpt = 0, 4, 16          # an empty batch: a valid descriptor returns MOT_OK without a launch
    d.tokens = d.tok_table = d.out = d.byte_table = d.ids_a = PTR
    d.tok_rows, d.tok_dim, d.byte_rows, d.byte_dim, d.model_dim = 100, 512, 458, 32, 1024
    d.id_source, d.norm_out = capi.IDS_GIVEN, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _grads():
    g = capi.MotEmbedMixGrads()
    g.struct_size = C.sizeof(capi.MotEmbedMixGrads)
    g.grad_out = g.d_tok_table = g.d_byte_table = PTR
    return g


def _rc(d):
    return capi.lib.mot_embed_mix_fwd(C.byref(d), None), capi.lib.mot_embed_mix_bwd(C.byref(d), C.byref(_grads()), None)


def test_enumerator_and_names():
    assert capi.MIX_CONCAT == 4
    assert (capi.MIX_NOOP, capi.MIX_SUM, capi.MIX_MEAN, capi.MIX_CONCAT_LINEAR) == (0, 1, 2, 3)
    assert Fm._MODES["concat"] == capi.MIX_CONCAT and "concat" in Fm._BWD_MODES
    assert mot.ConcatFrontEnd is M.ConcatFrontEnd and "ConcatFrontEnd" in mot.__all__


def test_abi_version_and_exports_are_unchanged():
    assert capi.ABI_VERSION == 13 == capi.lib.mot_version()
    assert capi.lib.mot_embed_mix_desc_size() == C.sizeof(capi.MotEmbedMixDesc)
    assert not [s for s in capi.EXPORTS if "concat" in s]      # the mode goes through mot_embed_mix_fwd / _bwd: no new symbol


def test_valid_descriptor_passes_validation():
    for kw in (dict(), dict(dtype=capi.BF16), dict(tok_dim=64, byte_dim=4, model_dim=128), dict(tok_dim=24, byte_dim=8, bpt=8, model_dim=88),
               dict(ids_b=PTR), dict(ids_b=PTR, norm_byte=1), dict(norm_tok=1, norm_byte=1, scale_tok=PTR, scale_byte=PTR),
               dict(id_source=capi.IDS_FROM_TTB, ids_a=None, ttb=PTR, ttb_rows=100, ttb_elem_bytes=2, pull_dir=capi.PULL_LEFT, add_padded=1)):
        assert _rc(_desc(**kw)) == (capi.MOT_OK, capi.MOT_OK), (kw, capi.lib.mot_last_error())


@pytest.mark.parametrize("kw, want, says", [
    (dict(model_dim=1000), capi.MOT_ESHAPE, b"tok_dim + bpt*byte_dim"),
    (dict(model_dim=512), capi.MOT_ESHAPE, b"tok_dim + bpt*byte_dim"),                          # SUM's shape rule does not apply
    (dict(tok_dim=30, model_dim=30 + 512), capi.MOT_EUNSUPPORTED, b"tok_dim 30 / byte_dim 32"),
    (dict(byte_dim=6, model_dim=512 + 96), capi.MOT_EUNSUPPORTED, b"tok_dim 512 / byte_dim 6"),
    (dict(dtype=capi.BF16, tok_dim=516, model_dim=516 + 512), capi.MOT_EUNSUPPORTED, b"multiples of 8"),   # 4 | 516, 8 does not
    (dict(dtype=capi.BF16, byte_dim=4, model_dim=512 + 64), capi.MOT_EUNSUPPORTED, b"multiples of 8"),
    (dict(tok_dim=2048, model_dim=2048 + 512), capi.MOT_EUNSUPPORTED, b"model_dim 2560 > 2048"),
    (dict(tok_dim=1024, byte_dim=128, model_dim=1024 + 2048), capi.MOT_EUNSUPPORTED, b"> 2048"),
    (dict(weight=PTR), capi.MOT_EINVAL, b"no weight"),
    (dict(bias=PTR), capi.MOT_EINVAL, b"no weight"),
    (dict(bpt=0, model_dim=512), capi.MOT_EUNSUPPORTED, b"bytes_per_token"),
    (dict(byte_table=None), capi.MOT_EINVAL, b"byte table"),
    (dict(ids_a=None), capi.MOT_EINVAL, b"ids_a"),
    # the per-(token, slot) norm over two id tensors is reduced inside an aligned power-of-two lane group
    (dict(ids_b=PTR, norm_byte=1, byte_dim=24, model_dim=512 + 16 * 24), capi.MOT_EUNSUPPORTED, b"two id tensors"),
    (dict(ids_b=PTR, norm_byte=1, tok_dim=48, model_dim=48 + 512), capi.MOT_EUNSUPPORTED, b"two id tensors"),
])
def test_validation_without_gpu(kw, want, says):
    """Every refusal comes back before any launch -- with a non-empty batch too (the pointers are fake)."""
    for n_rows in (0, 2):
        d = _desc(n_rows=n_rows, **kw)
        assert _rc(d) == (want, want), capi.lib.mot_last_error()
        assert says in capi.lib.mot_last_error(), capi.lib.mot_last_error()


def test_other_modes_keep_their_shape_rules():
    assert capi.lib.mot_embed_mix_fwd(C.byref(_desc(mode=capi.MIX_SUM)), None) == capi.MOT_ESHAPE        # 16*32 == 512 but model_dim 1024
    assert capi.lib.mot_embed_mix_fwd(C.byref(_desc(mode=capi.MIX_SUM, model_dim=512)), None) == capi.MOT_OK
    assert capi.lib.mot_embed_mix_fwd(C.byref(_desc(mode=5)), None) == capi.MOT_EINVAL
    assert capi.lib.mot_embed_mix_fwd(C.byref(_desc(mode=capi.MIX_SUM, model_dim=512, ids_b=PTR, norm_byte=1)), None) == capi.MOT_EUNSUPPORTED


def test_workspace_queries():
    d = _desc(n_rows=2, tokens_per_row=64)
    assert capi.lib.mot_embed_mix_workspace_bytes(C.byref(d)) == 0              # no norm_byte: nothing to precompute
    d = _desc(n_rows=2, tokens_per_row=64, norm_byte=1)
    assert capi.lib.mot_embed_mix_workspace_bytes(C.byref(d)) >= 458 * 4        # the 458-entry byte-row rms table
    # backward: the rms table and the positions grouped by token id (2 * rows + 3 * tokens int32)
    assert capi.lib.mot_embed_mix_bwd_workspace_bytes(C.byref(d)) >= 458 * 4 + (2 * 100 + 3 * 128) * 4


def test_concat_front_end_surface():
    fe = M.ConcatFrontEnd(token_vocab_size=50257, byte_vocab_size=458, token_dim=512, byte_dim=32)
    sd = fe.state_dict()
    assert list(sd) == ["embed_tokens.weight", "embed_bytes.weight"]            # run 711's attribute names; the ttb is no state
    assert tuple(sd["embed_tokens.weight"].shape) == (50257, 512) and tuple(sd["embed_bytes.weight"].shape) == (458, 32)
    assert fe.bpt == 16 and fe.model_dim == 1024 and (fe.pad_byte, fe.eot_byte) == (456, 457) and fe.ttb is None
    small = M.ConcatFrontEnd(40, 458, 24, 8, bytes_per_token=8, ttb=torch.from_numpy(pc.case_ttb("d24_b8_bpt8")))
    assert small.model_dim == 88 and tuple(small.ttb.shape) == (40, 8) and list(small.state_dict()) == list(sd)
    with pytest.raises(ValueError, match="byte_inputs"):
        fe(torch.zeros(8, dtype=torch.int32))                                   # no ttb attached, no ids given
    with pytest.raises(RuntimeError, match="HIP device only"):
        fe(torch.zeros(8, dtype=torch.int32), torch.zeros(128, dtype=torch.int64))


def test_functional_refuses_weight_and_cpu_tensors():
    Et, Eb = torch.zeros(10, 64), torch.zeros(458, 4)
    toks, ids = torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, 64, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="HIP device only"):
        mot.embed_mix(toks, Et, Eb, mode="concat", bpt=16, ids_a=ids, norm_out=True)
    with pytest.raises(KeyError):
        mot.embed_mix(toks, Et, Eb, mode="concatenate", bpt=16, ids_a=ids)


@pytest.mark.parametrize("name", list(pc.CASES))
def test_restatement_reproduces_reference_float64(name):
    Dt, Db, bpt, B, T, Vt, dual, seed = pc.CASES[name]
    toks, padded, pulled = (GOLDEN[pc.key(name, k)] for k in ("tokens", "ids_padded", "ids_pulled"))
    np.testing.assert_array_equal(toks, pc.case_tokens(name))
    np.testing.assert_array_equal(padded.reshape(B, T, bpt), pc.case_ttb(name)[toks])
    Et, Eb, g = pc.case_tables(name)
    r = pc.run(toks, pulled, padded if dual else None, Et, Eb, g, bpt=bpt, dtype=torch.float64)
    for what in pc.QUANTITIES:
        ref = GOLDEN[pc.key(name, f"f64/{what}")]
        assert r[what].shape == ref.shape, what
        err = pc.rel_err(r[what], ref)
        print(f"{name} {what}: restatement vs reference float64 {err:.2e}")
        assert err <= 1e-12, (what, err)
        assert 0 < float(GOLDEN[pc.key(name, f"f32err/{what}")]) < 1e-5
    # and the reference's float32 output is its float64 output to float32 accuracy
    assert pc.rel_err(GOLDEN[pc.key(name, "f32/out")], GOLDEN[pc.key(name, "f64/out")]) < 1e-6


def test_fixture_covers_the_eot_positions_and_stays_small():
    name = "d64_b4_bpt16"
    Dt, Db, bpt, B, T, Vt, dual, seed = pc.CASES[name]
    toks = GOLDEN[pc.key(name, "tokens")]
    e = Vt - 1
    assert toks[0, 0] == e and toks[0, T // 2] == e and toks[B - 1, 3] == e and toks[B - 1, 4] == e
    pulled, padded = GOLDEN[pc.key(name, "ids_pulled")], GOLDEN[pc.key(name, "ids_padded")]
    assert (pulled != padded).any()                                              # the pull moved bytes
    assert {pc.CASES[n][2] for n in pc.CASES} == {16, 8, 4} and any(pc.CASES[n][6] for n in pc.CASES)
    assert pc.GOLDEN.stat().st_size < (1 << 19)
    assert str(GOLDEN["torch_version"])
