"""CPU checks of the linear-on-bytes mixin (modded-nanogpt/runs/71051_*.py:225-229): the new C symbols and the ctypes mirror of
MotByteFcMixDesc, the C ABI's validation table (argument checks run before any HIP call, so no GPU is needed), the module surface of
ByteFcFrontEnd, and the plain-torch restatement (tests/byte_fc_ref.py) against the reference's own float64, float32 and bfloat16
runs in tests/golden/byte_fc.npz."""
import ctypes as C

import numpy as np
import pytest
import torch

import byte_fc_ref as bf
import mixture_of_tokenizers_amd as mot
from mixture_of_tokenizers_amd import _capi as capi
from mixture_of_tokenizers_amd import functional as Fm
from mixture_of_tokenizers_amd import modules as M

GOLDEN = bf.load_golden()
PTR = 64   # never dereferenced: validation fails first
NEW = ("mot_byte_fc_mix_desc_size", "mot_byte_fc_mix_workspace_bytes", "mot_byte_fc_mix_bwd_workspace_bytes", "mot_byte_fc_mix_fwd",
       "mot_byte_fc_mix_bwd")


def _desc(**kw):
    """A valid run-71051 descriptor (model 1024, 16 x 64 byte columns, ids given) with fake pointers and an empty batch."""
    d = capi.MotByteFcMixDesc()
    d.struct_size = C.sizeof(capi.MotByteFcMixDesc)
    d.dtype = capi.F32
    d.n_rows, d.tokens_per_row, d.bpt = 0, 4, 16          # an empty batch: a valid descriptor returns MOT_OK without a launch
    d.tokens = d.tok_table = d.byte_table = d.byte_fc = d.ids = d.out = d.out_row_rnorm = PTR
    d.tok_rows, d.tok_dim, d.model_dim, d.byte_rows, d.byte_dim = 100, 1024, 1024, 458, 64
    d.id_source, d.norm_out = capi.IDS_GIVEN, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _grads():
    g = capi.MotByteFcMixGrads()
    g.struct_size = C.sizeof(capi.MotByteFcMixGrads)
    g.grad_out = g.d_tok = g.d_byte = g.d_byte_fc = PTR
    return g


def _rc(d):
    return capi.lib.mot_byte_fc_mix_fwd(C.byref(d), None), capi.lib.mot_byte_fc_mix_bwd(C.byref(d), C.byref(_grads()), None)


def test_new_symbols_are_exported_and_the_abi_version_stays():
    for name in NEW:
        assert name in capi.EXPORTS and hasattr(capi.lib, name), name
    assert capi.ABI_VERSION == 13 == capi.lib.mot_version()
    assert capi.lib.mot_byte_fc_mix_desc_size() == C.sizeof(capi.MotByteFcMixDesc)
    assert mot.byte_fc_mix is Fm.byte_fc_mix and mot.ByteFcFrontEnd is M.ByteFcFrontEnd
    assert "byte_fc_mix" in mot.__all__ and "ByteFcFrontEnd" in mot.__all__


def test_embed_mix_gets_no_new_mode():
    assert (capi.MIX_NOOP, capi.MIX_SUM, capi.MIX_MEAN, capi.MIX_CONCAT_LINEAR, capi.MIX_CONCAT) == (0, 1, 2, 3, 4)
    assert sorted(Fm._MODES) == ["concat", "concat_linear", "mean", "noop", "sum"]
    e = capi.MotEmbedMixDesc()
    e.struct_size = C.sizeof(capi.MotEmbedMixDesc)
    e.mode, e.tokens, e.tok_table, e.out, e.tok_rows, e.tok_dim, e.model_dim = 5, PTR, PTR, PTR, 10, 64, 64
    assert capi.lib.mot_embed_mix_fwd(C.byref(e), None) == capi.MOT_EINVAL


def test_valid_descriptors_pass_validation():
    for kw in (dict(), dict(dtype=capi.BF16), dict(dtype=capi.BF16, flags=capi.BYTE_FC_COMPOSED), dict(norm_out=0, out_row_rnorm=None), dict(tok_dim=64, model_dim=64, byte_dim=4, bpt=8),
               dict(tok_dim=96, model_dim=96, byte_dim=24, bpt=4), dict(tok_dim=2048, model_dim=2048, byte_dim=128),
               dict(id_source=capi.IDS_FROM_TTB, ids=None, ttb=PTR, ttb_rows=100, ttb_elem_bytes=2, pull_dir=capi.PULL_LEFT)):
        d = _desc(**kw)
        assert capi.lib.mot_byte_fc_mix_fwd(C.byref(d), None) == capi.MOT_OK, (kw, capi.lib.mot_last_error())
        if d.id_source == capi.IDS_GIVEN and d.model_dim <= 1024:   # (rows of 2048 + 2048 columns: forward only, see below)
            assert capi.lib.mot_byte_fc_mix_bwd(C.byref(d), C.byref(_grads()), None) == capi.MOT_OK, (kw, capi.lib.mot_last_error())


@pytest.mark.parametrize("kw, want, says", [
    (dict(tok_dim=512), capi.MOT_ESHAPE, b"tok_dim 512 != model_dim 1024"),
    (dict(byte_fc=None), capi.MOT_EINVAL, b"byte_fc [1024, 1024]"),
    (dict(tok_dim=1022, model_dim=1022), capi.MOT_EUNSUPPORTED, b"model_dim 1022 / byte_dim 64 must be multiples of 4"),
    (dict(byte_dim=6), capi.MOT_EUNSUPPORTED, b"model_dim 1024 / byte_dim 6 must be multiples of 4"),
    (dict(dtype=capi.BF16, tok_dim=516, model_dim=516), capi.MOT_EUNSUPPORTED, b"model_dim 516 / byte_dim 64 must be multiples of 8"),   # 4 | 516, 8 does not
    (dict(dtype=capi.BF16, byte_dim=4), capi.MOT_EUNSUPPORTED, b"model_dim 1024 / byte_dim 4 must be multiples of 8"),
    (dict(tok_dim=2052, model_dim=2052), capi.MOT_EUNSUPPORTED, b"model_dim 2052 / bpt*byte_dim 1024 above 2048"),
    (dict(byte_dim=132), capi.MOT_EUNSUPPORTED, b"model_dim 1024 / bpt*byte_dim 2112 above 2048"),
    (dict(dtype=2), capi.MOT_EINVAL, b"bad dtype 2"),
    (dict(id_source=capi.IDS_NONE), capi.MOT_EINVAL, b"bad id_source 0"),
    (dict(id_source=7), capi.MOT_EINVAL, b"bad id_source 7"),
    (dict(bpt=0), capi.MOT_EUNSUPPORTED, b"bytes_per_token 0"),
    (dict(ids=None), capi.MOT_EINVAL, b"ids missing"),
    (dict(byte_table=None), capi.MOT_EINVAL, b"byte_table"),
    (dict(out_ids_pulled=PTR), capi.MOT_EINVAL, b"MOT_IDS_FROM_TTB"),
    (dict(flags=2), capi.MOT_EINVAL, b"unknown flags 0x2"),
    (dict(struct_size=8), capi.MOT_EINVAL, b"struct_size"),
])
def test_refusals_come_back_before_any_launch(kw, want, says):
    """With a non-empty batch too: the pointers are fake, so a launch would fault."""
    for n_rows in (0, 2):
        d = _desc(n_rows=n_rows, **kw)
        assert _rc(d) == (want, want), capi.lib.mot_last_error()
        assert says in capi.lib.mot_last_error(), capi.lib.mot_last_error()
        if kw.keys() & {"tok_dim", "byte_dim", "dtype", "id_source", "bpt", "flags", "struct_size"}:   # what a size query can see
            assert capi.lib.mot_byte_fc_mix_workspace_bytes(C.byref(d)) == 0
            assert capi.lib.mot_byte_fc_mix_bwd_workspace_bytes(C.byref(d)) == 0


def test_bad_pull_direction_and_table_source():
    ttb = dict(id_source=capi.IDS_FROM_TTB, ids=None, ttb=PTR, ttb_rows=100, ttb_elem_bytes=2, pull_dir=capi.PULL_LEFT)
    for n_rows in (0, 2):
        for kw, says in ((dict(pull_dir=3), b"bad pull_dir 3"), (dict(pull_dir=-1), b"bad pull_dir -1"), (dict(ttb_elem_bytes=8), b"ttb_elem_bytes"),
                         (dict(ttb=None), b"ttb missing")):
            d = _desc(n_rows=n_rows, **{**ttb, **kw})
            assert capi.lib.mot_byte_fc_mix_fwd(C.byref(d), None) == capi.MOT_EINVAL
            assert says in capi.lib.mot_last_error(), capi.lib.mot_last_error()
    # the backward takes the ids the forward used
    d = _desc(**ttb)
    assert capi.lib.mot_byte_fc_mix_bwd(C.byref(d), C.byref(_grads()), None) == capi.MOT_EUNSUPPORTED
    assert capi.lib.mot_byte_fc_mix_bwd_workspace_bytes(C.byref(d)) == 0


def test_backward_wants_its_buffers():
    g = _grads()
    g.d_byte_fc = None
    assert capi.lib.mot_byte_fc_mix_bwd(C.byref(_desc(n_rows=2)), C.byref(g), None) == capi.MOT_EINVAL
    assert capi.lib.mot_byte_fc_mix_bwd(C.byref(_desc(n_rows=2, out_row_rnorm=None)), C.byref(_grads()), None) == capi.MOT_EINVAL
    assert b"out_row_rnorm" in capi.lib.mot_last_error()
    assert capi.lib.mot_byte_fc_mix_bwd(C.byref(_desc(n_rows=2)), None, None) == capi.MOT_EINVAL
    # gradient rows wider than 2048 columns go part by part through the lane-contiguous scatter, or not at all
    d = _desc(n_rows=2, tok_dim=1032, model_dim=1032, byte_dim=64)
    assert capi.lib.mot_byte_fc_mix_fwd(C.byref(_desc(tok_dim=1032, model_dim=1032)), None) == capi.MOT_OK
    assert capi.lib.mot_byte_fc_mix_bwd(C.byref(d), C.byref(_grads()), None) == capi.MOT_EUNSUPPORTED
    assert b"model_dim 1032 + bpt*byte_dim 1024" in capi.lib.mot_last_error()


def test_workspace_queries_and_a_workspace_that_is_too_small():
    d = _desc(n_rows=2, tokens_per_row=64)
    K = 16 * 64
    fwd, bwd = capi.lib.mot_byte_fc_mix_workspace_bytes(C.byref(d)), capi.lib.mot_byte_fc_mix_bwd_workspace_bytes(C.byref(d))
    assert 128 * K * 4 <= fwd < 128 * K * 4 + 4096                                   # u of the 128 tokens, nothing else
    assert bwd >= 128 * (1024 + K) * 4 + 128 * K * 4 + (2 * 100 + 3 * 128) * 4       # the rows [ds | du], u, the grouped positions
    for ws_bytes in (0, fwd - 1):
        d.workspace, d.workspace_bytes = PTR, ws_bytes
        assert capi.lib.mot_byte_fc_mix_fwd(C.byref(d), None) == capi.MOT_EWORKSPACE
        assert str(fwd).encode() in capi.lib.mot_last_error()
    d.workspace, d.workspace_bytes = PTR, bwd - 1
    assert capi.lib.mot_byte_fc_mix_bwd(C.byref(d), C.byref(_grads()), None) == capi.MOT_EWORKSPACE
    # ids from the token->byte table: room for the two int64 id tensors; more tokens than one slab: u stays one slab
    t = _desc(n_rows=2, tokens_per_row=64, id_source=capi.IDS_FROM_TTB, ids=None, ttb=PTR, ttb_rows=100, ttb_elem_bytes=2)
    assert capi.lib.mot_byte_fc_mix_workspace_bytes(C.byref(t)) >= fwd + 2 * 128 * 16 * 8
    big = _desc(n_rows=8, tokens_per_row=65536)
    assert capi.lib.mot_byte_fc_mix_workspace_bytes(C.byref(big)) < 65536 * K * 4
    assert capi.lib.mot_byte_fc_mix_bwd_workspace_bytes(C.byref(big)) < 2 * 65536 * (1024 + 2 * K) * 4
    # bf16: u in bf16, and the backward's bf16 copies and widened tables
    h = _desc(n_rows=2, tokens_per_row=64, dtype=capi.BF16)
    assert capi.lib.mot_byte_fc_mix_workspace_bytes(C.byref(h)) == fwd // 2
    assert capi.lib.mot_byte_fc_mix_bwd_workspace_bytes(C.byref(h)) >= 128 * (1024 + K) * 4 + (100 * 1024 + 458 * 64) * 4


def test_front_end_surface():
    torch.manual_seed(0)
    fe = M.ByteFcFrontEnd(token_vocab_size=50257, byte_vocab_size=458, model_dim=1024, byte_dim=64)
    sd = fe.state_dict()
    assert sorted(sd) == ["byte_fc", "embed_bytes.weight", "embed_tokens.weight"]      # run 71051's attribute names; the ttb is no state
    assert tuple(sd["embed_tokens.weight"].shape) == (50257, 1024) and tuple(sd["embed_bytes.weight"].shape) == (458, 64)
    assert tuple(sd["byte_fc"].shape) == (1024, 1024) and isinstance(fe.byte_fc, torch.nn.Parameter)
    bound = 3 ** 0.5 * 0.5 / 1024 ** 0.5                                              # init_linear, runs/71051_*.py:134-137
    w = fe.byte_fc.detach()
    assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.99 * bound
    assert abs(float(w.std()) - 0.5 / 1024 ** 0.5) < 0.01 * 0.5 / 1024 ** 0.5 and abs(float(w.mean())) < 1e-3 * bound * 10
    assert fe.bpt == 16 and fe.model_dim == 1024 and (fe.pad_byte, fe.eot_byte) == (456, 457) and fe.ttb is None
    small = M.ByteFcFrontEnd(40, 458, 64, 4, bytes_per_token=8, ttb=torch.from_numpy(bf.case_ttb("m64_b4_bpt8")))
    assert tuple(small.byte_fc.shape) == (64, 32) and tuple(small.ttb.shape) == (40, 8) and sorted(small.state_dict()) == sorted(sd)
    with pytest.raises(ValueError, match="byte_inputs"):
        fe(torch.zeros(8, dtype=torch.int32))                                   # no ttb attached, no ids given
    with pytest.raises(RuntimeError, match="HIP device only"):
        fe(torch.zeros(8, dtype=torch.int32), torch.zeros(128, dtype=torch.int64))


def test_functional_refuses_cpu_and_mixed_dtypes():
    Et, Eb, W = torch.zeros(10, 64), torch.zeros(458, 8), torch.zeros(64, 64)
    toks, ids = torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, 32, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="HIP device only"):
        mot.byte_fc_mix(toks, Et, Eb, W, bpt=8, ids=ids)
    with pytest.raises(RuntimeError, match="HIP device only"):
        Fm.byte_fc_mix_backward(torch.zeros(1, 4, 64), toks, Et, Eb, W, bpt=8, ids=ids, norm_out=False)
    with pytest.raises(TypeError, match="share one dtype"):
        mot.byte_fc_mix(toks, Et, Eb.bfloat16(), W, bpt=8, ids=ids)
    with pytest.raises(TypeError, match="share one dtype"):
        mot.byte_fc_mix(toks, Et.bfloat16(), Eb.bfloat16(), W, bpt=8, ids=ids)
    with pytest.raises(TypeError, match="float32 or bfloat16"):
        mot.byte_fc_mix(toks, Et.double(), Eb.double(), W.double(), bpt=8, ids=ids)


@pytest.mark.parametrize("name", list(bf.CASES))
def test_restatement_reproduces_the_reference(name):
    Dm, Db, bpt, B, T, Vt, std, seed = bf.CASES[name]
    toks, padded, pulled = (GOLDEN[bf.key(name, k)] for k in ("tokens", "ids_padded", "ids_pulled"))
    np.testing.assert_array_equal(toks, bf.case_tokens(name))
    np.testing.assert_array_equal(padded.reshape(B, T, bpt), bf.case_ttb(name)[toks])
    Et, Eb, W, g = bf.case_tables(name)
    r = bf.run(toks, pulled, Et, Eb, W, g, bpt=bpt, dtype=torch.float64)          # eps None: the float64 epsilon, as the reference's run
    for what in bf.QUANTITIES:
        ref = GOLDEN[bf.key(name, f"f64/{what}")]
        assert r[what].shape == ref.shape, what
        err = bf.rel_err(r[what], ref)
        print(f"{name} {what}: restatement vs reference float64 {err:.2e}")
        assert err <= 1e-12, (what, err)
        assert 0 < float(GOLDEN[bf.key(name, f"f32err/{what}")]) < (1e-5 if std == 1.0 else 1e-3)
        assert 0 < float(GOLDEN[bf.key(name, f"bf16err/{what}")]) < 2.0 ** -5
    # the float32 and bfloat16 runs: the same torch operations in the same order, so the same bits or one rounding apart
    x32 = bf.run(toks, pulled, Et, Eb, W, g, bpt=bpt, dtype=torch.float32)["out"]
    ref32 = GOLDEN[bf.key(name, "f32/out")].astype(np.float64)
    assert (np.abs(x32 - ref32) <= 2.0 ** -23 * np.abs(ref32)).all()
    x16 = bf.run(toks, pulled, Et, Eb, W, g, bpt=bpt, dtype=torch.bfloat16)["out"]
    ref16 = GOLDEN[bf.key(name, "bf16/out")].astype(np.float64)
    assert (np.abs(x16 - ref16) <= 2.0 ** -7 * np.abs(ref16)).all()
    # F.rms_norm(eps=None) on bfloat16 rows takes the float32 epsilon (its fp32 opmath type): what MotByteFcMixDesc.eps <= 0 means
    x16e = bf.run(toks, pulled, Et, Eb, W, g, bpt=bpt, dtype=torch.bfloat16, eps=bf.F32_EPS)["out"]
    np.testing.assert_array_equal(x16e, x16)
    if std != 1.0:   # and with 2^-7 the small-magnitude rows are off by whole bfloat16 steps
        x16b = bf.run(toks, pulled, Et, Eb, W, g, bpt=bpt, dtype=torch.bfloat16, eps=2.0 ** -7)["out"]
        assert np.abs(x16b - ref16).max() > 2.0 ** -6 * np.abs(ref16).max()


@pytest.mark.parametrize("name", list(bf.CASES))
def test_restatement_equals_the_concat_linear_emulation(name):
    """norm(tok + byte_fc u) == norm([I | byte_fc] cat(tok, u)): the identity the benchmark's emulation baseline rests on."""
    Dm, Db, bpt, B, T, Vt, std, seed = bf.CASES[name]
    toks, pulled = GOLDEN[bf.key(name, "tokens")], GOLDEN[bf.key(name, "ids_pulled")].astype(np.int64)
    Et, Eb, W, g = bf.case_tables(name)
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    x = bf.forward(toks, pulled, t(Et), t(Eb), t(W), bpt=bpt).numpy()
    Wc = t(bf.as_concat_linear_weight(W))
    assert tuple(Wc.shape) == (Dm, Dm + bpt * Db)
    cat = torch.cat([t(Et)[torch.as_tensor(toks).long()], t(Eb)[torch.as_tensor(pulled).reshape(B, T, bpt)].reshape(B, T, bpt * Db)], dim=-1)
    y = torch.nn.functional.rms_norm(torch.nn.functional.linear(cat, Wc), (Dm,)).numpy()
    assert bf.rel_err(y, x) <= 1e-12


def test_fixture_covers_the_eot_positions_and_stays_small():
    name = "m64_b8_bpt8"
    Dm, Db, bpt, B, T, Vt, std, seed = bf.CASES[name]
    toks = GOLDEN[bf.key(name, "tokens")]
    e = Vt - 1
    assert toks[0, 0] == e and toks[0, T // 2] == e and toks[B - 1, 3] == e and toks[B - 1, 4] == e
    assert (GOLDEN[bf.key(name, "ids_pulled")] != GOLDEN[bf.key(name, "ids_padded")]).any()      # the pull moved bytes
    assert all((B, T) == (2, 24) and Vt <= 128 for (_, _, _, B, T, Vt, _, _) in bf.CASES.values())
    assert any(c[1] * c[2] != c[0] for c in bf.CASES.values()) and any(c[6] == 0.02 for c in bf.CASES.values())
    assert bf.GOLDEN.stat().st_size < (1 << 20)
    assert str(GOLDEN["torch_version"])
