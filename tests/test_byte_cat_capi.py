"""CPU checks of the bytes-only front-end and the byte value embeddings (mot_byte_cat_fwd / _bwd,
modded-nanogpt/runs/5_bytes-in_bytes-valemb.py:225-232, 248, 305, 314): the new symbols and structs, the C ABI's validation table
(argument checks run before any HIP call, so no GPU is needed), the module surface of BytesFrontEnd, and the plain-torch
restatement (tests/byte_cat_ref.py) against the reference's own float64, float32 and bfloat16 runs in tests/golden/byte_cat.npz."""
import ctypes as C

import numpy as np
import pytest
import torch

import byte_cat_ref as bc
import pure_concat_ref as pc
import mixture_of_tokenizers_amd as mot
from mixture_of_tokenizers_amd import _capi as capi
from mixture_of_tokenizers_amd import functional as Fm
from mixture_of_tokenizers_amd import modules as M

GOLDEN = bc.load_golden()
PTR = 64   # never dereferenced: validation fails first
SYMBOLS = ("mot_byte_cat_fwd", "mot_byte_cat_bwd", "mot_byte_cat_desc_size", "mot_byte_cat_workspace_bytes", "mot_byte_cat_bwd_workspace_bytes")


def _desc(slot=None, **kw):
    """A valid run-5 descriptor (16 x 64 = 1024 columns, four tables, ids given) with fake pointers; slot = {index: {field: value}}."""
    d = capi.MotByteCatDesc()
    d.struct_size = C.sizeof(capi.MotByteCatDesc)
    d.dtype = kw.get("dtype", capi.F32)
    d.n_rows, d.tokens_per_row, d.bpt, d.byte_dim, d.n_out = 0, 4, 16, 64, 4   # an empty batch: a valid descriptor returns MOT_OK without a launch
    d.id_source, d.ids = capi.IDS_GIVEN, PTR
    for j in range(4):
        d.slot[j].table, d.slot[j].rows, d.slot[j].out, d.slot[j].norm, d.slot[j].dtype = PTR, 458, PTR, int(j == 0), d.dtype
    for k, v in kw.items():
        setattr(d, k, v)
    for j, fields in (slot or {}).items():
        for k, v in fields.items():
            setattr(d.slot[j], k, v)
    return d


def _grads(d):
    g = capi.MotByteCatGrads()
    g.struct_size = C.sizeof(capi.MotByteCatGrads)
    for j in range(d.n_out if 0 < d.n_out <= 4 else 0):
        g.slot[j].grad_out = g.slot[j].d_table = PTR
    return g


def _rc(d):
    return capi.lib.mot_byte_cat_fwd(C.byref(d), None), capi.lib.mot_byte_cat_bwd(C.byref(d), C.byref(_grads(d)), None)


def test_abi_version_modes_and_new_symbols():
    assert capi.ABI_VERSION == 13 == capi.lib.mot_version()
    for s in SYMBOLS:
        assert s in capi.EXPORTS and getattr(capi.lib, s) is not None
    assert capi.lib.mot_byte_cat_desc_size() == C.sizeof(capi.MotByteCatDesc)
    assert sorted(Fm._MODES) == ["concat", "concat_linear", "mean", "noop", "sum"]            # no new mode: new symbols instead
    assert (capi.MIX_NOOP, capi.MIX_SUM, capi.MIX_MEAN, capi.MIX_CONCAT_LINEAR, capi.MIX_CONCAT) == (0, 1, 2, 3, 4)
    assert mot.byte_cat is Fm.byte_cat and mot.BytesFrontEnd is M.BytesFrontEnd
    assert "byte_cat" in mot.__all__ and "BytesFrontEnd" in mot.__all__ and callable(Fm.byte_cat_backward)


def test_valid_descriptors_pass_validation():
    for kw in (dict(), dict(dtype=capi.BF16), dict(n_out=1), dict(bpt=4, byte_dim=12), dict(bpt=16, byte_dim=128), dict(dtype=capi.BF16, byte_dim=8),
               dict(slot={1: dict(rows=300), 2: dict(rows=64), 3: dict(rows=5)}), dict(tokens=None)):
        assert _rc(_desc(**kw)) == (capi.MOT_OK, capi.MOT_OK), (kw, capi.lib.mot_last_error())
    ttb = dict(id_source=capi.IDS_FROM_TTB, ids=None, tokens=PTR, ttb=PTR, ttb_rows=100, ttb_elem_bytes=2, pull_dir=capi.PULL_LEFT)
    assert capi.lib.mot_byte_cat_fwd(C.byref(_desc(**ttb)), None) == capi.MOT_OK, capi.lib.mot_last_error()
    d = _desc(**ttb)   # the backward takes the ids the forward used
    assert capi.lib.mot_byte_cat_bwd(C.byref(d), C.byref(_grads(d)), None) == capi.MOT_EUNSUPPORTED and b"MOT_IDS_GIVEN" in capi.lib.mot_last_error()


@pytest.mark.parametrize("kw, want, says", [
    (dict(byte_dim=6, bpt=4), capi.MOT_EUNSUPPORTED, b"byte_dim 6"),                              # no multiple of the 16-byte vector
    (dict(dtype=capi.BF16, byte_dim=4), capi.MOT_EUNSUPPORTED, b"byte_dim 4"),                     # 4 fp32 elements are 16 bytes, 4 bf16 are not
    (dict(dtype=capi.BF16, byte_dim=12, bpt=4), capi.MOT_EUNSUPPORTED, b"multiple of 8"),
    (dict(byte_dim=132), capi.MOT_EUNSUPPORTED, b"model_dim 2112"),
    (dict(bpt=64, byte_dim=64), capi.MOT_EUNSUPPORTED, b"model_dim 4096"),
    (dict(n_out=0), capi.MOT_EUNSUPPORTED, b"n_out 0"),
    (dict(n_out=5), capi.MOT_EUNSUPPORTED, b"n_out 5"),
    (dict(slot={2: dict(dtype=capi.BF16)}), capi.MOT_EINVAL, b"slot 2 has dtype 1"),               # mixed dtypes
    (dict(dtype=capi.BF16, byte_dim=8, slot={0: dict(dtype=capi.F32)}), capi.MOT_EINVAL, b"slot 0 has dtype 0"),
    (dict(slot={1: dict(table=None)}), capi.MOT_EINVAL, b"slot 1 has a null table"),
    (dict(bpt=0), capi.MOT_EUNSUPPORTED, b"bytes_per_token 0"),
    (dict(dtype=2), capi.MOT_EINVAL, b"bad dtype 2"),
    (dict(ids=None), capi.MOT_EINVAL, b"ids missing"),
    (dict(struct_size=8), capi.MOT_EINVAL, b"struct_size 8"),
])
def test_refusals_without_gpu(kw, want, says):
    """Every refusal comes back before any launch -- with a non-empty batch too (the pointers are fake) -- and both workspace
    queries return 0 for a descriptor that the shape rules refuse."""
    for n_rows in (0, 2):
        d = _desc(n_rows=n_rows, **kw)
        assert _rc(d) == (want, want), capi.lib.mot_last_error()
        assert says in capi.lib.mot_last_error(), capi.lib.mot_last_error()
        assert capi.lib.mot_byte_cat_workspace_bytes(C.byref(d)) == 0
        if b"ids missing" not in says:      # (not one of the listed refusals: the id tensor is the call's to check)
            assert capi.lib.mot_byte_cat_bwd_workspace_bytes(C.byref(d)) == 0


def test_null_out_is_refused_by_the_forward_only():
    d = _desc(n_rows=2, tokens_per_row=64, slot={3: dict(out=None)})
    assert capi.lib.mot_byte_cat_fwd(C.byref(d), None) == capi.MOT_EINVAL and b"slot 3 has a null out" in capi.lib.mot_last_error()
    assert capi.lib.mot_byte_cat_workspace_bytes(C.byref(d)) == 0               # the forward's query: 0 for the descriptor its call refuses
    assert capi.lib.mot_byte_cat_bwd_workspace_bytes(C.byref(d)) >= 128 * 8     # the backward never reads `out`: its call takes this descriptor
    d = _desc(n_rows=0, slot={3: dict(out=None)})
    assert capi.lib.mot_byte_cat_bwd(C.byref(d), C.byref(_grads(d)), None) == capi.MOT_OK          # the backward never writes `out`
    d = _desc(n_rows=0, n_out=3, slot={3: dict(out=None, table=None)})                                # an unused slot is not looked at
    assert _rc(d) == (capi.MOT_OK, capi.MOT_OK)


def test_workspace_queries():
    d = _desc(n_rows=2, tokens_per_row=64)
    assert capi.lib.mot_byte_cat_workspace_bytes(C.byref(d)) == 0                # the forward needs none
    assert capi.lib.mot_byte_cat_bwd_workspace_bytes(C.byref(d)) >= 128 * 8      # two row scalars per token for the one normed table
    d = _desc(n_rows=2, tokens_per_row=64, slot={0: dict(norm=0)})
    assert capi.lib.mot_byte_cat_bwd_workspace_bytes(C.byref(d)) == 0            # no norm: nothing to precompute
    d = _desc(n_rows=2, tokens_per_row=64)                                       # a backward without its workspace is refused, not run
    assert capi.lib.mot_byte_cat_bwd(C.byref(d), C.byref(_grads(d)), None) == capi.MOT_EWORKSPACE


def test_bytes_front_end_surface():
    fe = M.BytesFrontEnd(458, 64)
    sd = fe.state_dict()
    assert list(sd) == ["embed_bytes.weight"] and tuple(sd["embed_bytes.weight"].shape) == (458, 64)      # runs 4, 6
    assert fe.bpt == 16 and fe.model_dim == 1024 and (fe.pad_byte, fe.eot_byte) == (456, 457) and fe.ttb is None
    fe3 = M.BytesFrontEnd(458, 64, n_value_embeds=3, value_rows=50257)
    sd = fe3.state_dict()
    assert list(sd) == ["embed_bytes.weight"] + [f"value_embeds_bytes.{j}.weight" for j in range(3)]       # run 5's attribute names
    assert all(tuple(sd[f"value_embeds_bytes.{j}.weight"].shape) == (50257, 64) for j in range(3))
    assert tuple(M.BytesFrontEnd(458, 8, 4, n_value_embeds=3).state_dict()["value_embeds_bytes.2.weight"].shape) == (458, 8)
    with pytest.raises(ValueError, match="value_rows"):
        M.BytesFrontEnd(458, 64, n_value_embeds=3, value_rows=100)
    with pytest.raises(ValueError, match="byte_inputs"):
        fe(torch.zeros(8, dtype=torch.int32))                                   # no ttb attached, no ids given
    with pytest.raises(ValueError, match="produces nothing"):
        fe(byte_inputs=torch.zeros(128, dtype=torch.int64), x0=False)
    with pytest.raises(RuntimeError, match="HIP device only"):
        fe3(byte_inputs=torch.zeros(128, dtype=torch.int64))


def test_functional_refuses_cpu_tensors_and_bad_arguments():
    T4 = [torch.zeros(458, 4) for _ in range(4)]
    ids = torch.zeros(1, 64, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="HIP device only"):
        mot.byte_cat(T4, bpt=16, norm=(True, False, False, False), ids=ids)
    with pytest.raises(RuntimeError, match="HIP device only"):
        Fm.byte_cat_backward([torch.zeros(1, 4, 64)], T4[:1], bpt=16, norm=(True,), ids=ids)
    with pytest.raises(TypeError, match="share one dtype"):
        mot.byte_cat([T4[0], T4[1].bfloat16()], bpt=16, norm=(True, False), ids=ids)


@pytest.mark.parametrize("name", list(bc.CASES))
def test_restatement_reproduces_reference(name):
    Db, bpt, B, T, Vt, norm, std, seed = bc.CASES[name]
    toks, padded, pulled = (GOLDEN[bc.key(name, k)] for k in ("tokens", "ids_padded", "ids_pulled"))
    np.testing.assert_array_equal(toks, bc.case_tokens(name))
    np.testing.assert_array_equal(padded.reshape(B, T, bpt), bc.case_ttb(name)[toks])
    tables, gs = bc.case_tables(name)
    r64 = bc.run(pulled, tables, norm, gs, bpt=bpt, dtype=torch.float64)
    r32 = bc.run(pulled, tables, norm, gs, bpt=bpt, dtype=torch.float32)
    # bfloat16 with the FLOAT32 epsilon handed over explicitly: equal bits with the reference's bfloat16 run (eps=None) is what
    # pins the epsilon that F.rms_norm(eps=None) applies to bfloat16 rows
    r16 = bc.run(pulled, tables, norm, gs, bpt=bpt, dtype=torch.bfloat16, eps=bc.F32_EPS)
    for j in range(len(norm)):
        for what in ("out", "d_table"):
            ref = GOLDEN[bc.key(name, f"f64/{what}{j}")]
            assert r64[what][j].shape == ref.shape, what
            err = pc.rel_err(r64[what][j], ref)
            print(f"{name} {what}{j}: restatement vs reference float64 {err:.2e}")
            assert err <= 1e-12, (what, j, err)
        ref32 = GOLDEN[bc.key(name, f"f32/out{j}")].astype(np.float64)
        assert (np.abs(r32["out"][j] - ref32) <= 1e-6 + 1e-6 * np.abs(ref32)).all()
        ref16 = torch.from_numpy(GOLDEN[bc.key(name, f"bf16/out{j}")]).view(torch.bfloat16).double().numpy()
        np.testing.assert_array_equal(r16["out"][j], ref16)
        if not norm[j]:   # a copy in every dtype
            np.testing.assert_array_equal(ref32, GOLDEN[bc.key(name, f"f64/out{j}")])
            np.testing.assert_array_equal(ref16, ref32)
        assert float(GOLDEN[bc.key(name, f"bf16err/d_table{j}")]) < 0.05


def test_small_rows_tell_the_two_epsilons_apart():
    """On rows of magnitude 0.02 the float32 and the bfloat16 epsilon give different bfloat16 outputs: the equality above is no accident."""
    name = "b8_bpt8_n2_small"
    Db, bpt, B, T, Vt, norm, std, seed = bc.CASES[name]
    tables, gs = bc.case_tables(name)
    r = bc.run(GOLDEN[bc.key(name, "ids_pulled")], tables, norm, gs, bpt=bpt, dtype=torch.bfloat16, eps=bc.BF16_EPS)
    ref16 = torch.from_numpy(GOLDEN[bc.key(name, "bf16/out0")]).view(torch.bfloat16).double().numpy()
    assert (r["out"][0] != ref16).mean() > 0.5


def test_fixture_covers_the_listed_cases_and_stays_small():
    cases = bc.CASES.values()
    assert {c[1] for c in cases} == {16, 8, 4} and {4, 8, 48, 64} <= {c[0] for c in cases}
    assert (True, False, False, False) in {c[5] for c in cases} and (True,) in {c[5] for c in cases}
    name = "b8_bpt16_n4"
    Db, bpt, B, T, Vt, norm, std, seed = bc.CASES[name]
    toks = GOLDEN[bc.key(name, "tokens")]
    e = Vt - 1
    assert toks[0, 0] == e and toks[0, T // 2] == e and toks[B - 1, 3] == e and toks[B - 1, 4] == e
    assert (GOLDEN[bc.key(name, "ids_pulled")] != GOLDEN[bc.key(name, "ids_padded")]).any()      # the pull moved bytes
    assert bc.GOLDEN.stat().st_size <= pc.GOLDEN.stat().st_size
    assert str(GOLDEN["torch_version"])
