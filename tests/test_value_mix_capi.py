"""CPU checks of the mixture-of-tokenizers value embeddings (modded-nanogpt/runs/9_mot-in_mot-valemb.py:310-313): the new C symbols
and the ctypes mirror of MotValueMixDesc, the C ABI's validation table (argument checks run before any HIP call, so no GPU is
needed), the module surface of MotValueEmbeds, and the plain-torch restatement (tests/value_mix_ref.py) against the reference's own
float64, float32 and bfloat16 runs in tests/golden/value_mix.npz."""
import ctypes as C

import numpy as np
import pytest
import torch

import mixture_of_tokenizers_amd as mot
import value_mix_ref as vm
from mixture_of_tokenizers_amd import _capi as capi
from mixture_of_tokenizers_amd import functional as Fm
from mixture_of_tokenizers_amd import modules as M

GOLDEN = vm.load_golden()
PTR = 64   # never dereferenced: validation fails first
NEW = ("mot_value_mix_desc_size", "mot_value_mix_workspace_bytes", "mot_value_mix_fwd", "mot_value_mix_bwd")


def _desc(**kw):
    """A valid descriptor of the runs (3 slots, 1024 / 64 / 16 -> 1024, ids given) with fake pointers and an empty batch."""
    d = capi.MotValueMixDesc()
    d.struct_size = C.sizeof(capi.MotValueMixDesc)
    d.dtype = capi.F32
    d.n_rows, d.tokens_per_row, d.bpt = 0, 4, 16          # an empty batch: a valid descriptor returns MOT_OK without a launch
    d.tokens = d.ids = PTR
    d.tok_rows, d.byte_rows, d.token_dim, d.byte_dim, d.out_dim, d.n_slots = 100, 458, 1024, 64, 1024, 3
    d.id_source, d.norm_out = capi.IDS_GIVEN, 1
    slot = kw.pop("slot", {})
    for j in range(capi.VALUE_MIX_MAX_SLOTS):
        s = d.slot[j]
        s.tok_table = s.byte_table = s.weight = s.out = s.out_row_rnorm = PTR
    for k, v in kw.items():
        setattr(d, k, v)
    for (j, k), v in slot.items():
        setattr(d.slot[j], k, v)
    return d


def _grads(kw=None):
    g = capi.MotValueMixGrads()
    g.struct_size = C.sizeof(capi.MotValueMixGrads)
    for j in range(capi.VALUE_MIX_MAX_SLOTS):
        g.slot[j].grad_out = g.slot[j].d_tok = g.slot[j].d_byte = g.slot[j].d_weight = PTR
    for (j, k), v in (kw or {}).items():
        setattr(g.slot[j], k, v)
    return g


def _rc(d):
    return capi.lib.mot_value_mix_fwd(C.byref(d), None), capi.lib.mot_value_mix_bwd(C.byref(d), C.byref(_grads()), None)


def test_new_symbols_are_exported_and_the_abi_version_stays():
    for name in NEW:
        assert name in capi.EXPORTS and hasattr(capi.lib, name), name
    assert capi.ABI_VERSION == 13 == capi.lib.mot_version()
    assert capi.lib.mot_value_mix_desc_size() == C.sizeof(capi.MotValueMixDesc)
    assert mot.value_mix is Fm.value_mix and mot.MotValueEmbeds is M.MotValueEmbeds
    assert "value_mix" in mot.__all__ and "MotValueEmbeds" in mot.__all__


def test_valid_descriptors_pass_validation():
    for kw in (dict(), dict(dtype=capi.BF16), dict(n_slots=1), dict(n_slots=4), dict(norm_out=0, slot={(0, "out_row_rnorm"): None}),
               dict(token_dim=32, byte_dim=8, bpt=8, out_dim=32), dict(token_dim=64, byte_dim=24, bpt=4, out_dim=64),
               dict(token_dim=128, byte_dim=16, bpt=8, out_dim=512), dict(token_dim=1024, byte_dim=64, bpt=16, out_dim=2048),
               dict(id_source=capi.IDS_FROM_TTB, ids=None, ttb=PTR, ttb_rows=100, ttb_elem_bytes=2, pull_dir=capi.PULL_LEFT)):
        d = _desc(**kw)
        assert capi.lib.mot_value_mix_fwd(C.byref(d), None) == capi.MOT_OK, (kw, capi.lib.mot_last_error())
        if d.id_source == capi.IDS_GIVEN:
            assert capi.lib.mot_value_mix_bwd(C.byref(d), C.byref(_grads()), None) == capi.MOT_OK, (kw, capi.lib.mot_last_error())


@pytest.mark.parametrize("kw, want, says", [
    (dict(token_dim=1022), capi.MOT_EUNSUPPORTED, b"token_dim 1022 must be a multiple of 4"),
    (dict(byte_dim=6), capi.MOT_EUNSUPPORTED, b"byte_dim 6 must be a multiple of 4"),
    (dict(out_dim=1022), capi.MOT_EUNSUPPORTED, b"out_dim 1022 must be a multiple of 4"),
    (dict(dtype=capi.BF16, token_dim=516), capi.MOT_EUNSUPPORTED, b"token_dim 516 must be a multiple of 8"),   # 4 | 516, 8 does not
    (dict(dtype=capi.BF16, byte_dim=4), capi.MOT_EUNSUPPORTED, b"byte_dim 4 must be a multiple of 8"),
    (dict(dtype=capi.BF16, out_dim=516), capi.MOT_EUNSUPPORTED, b"out_dim 516 must be a multiple of 8"),
    (dict(token_dim=1028), capi.MOT_EUNSUPPORTED, b"K = token_dim + bpt*byte_dim = 2052 above 2048"),
    (dict(byte_dim=68), capi.MOT_EUNSUPPORTED, b"K = token_dim + bpt*byte_dim = 2112 above 2048"),
    (dict(out_dim=2052), capi.MOT_EUNSUPPORTED, b"out_dim 2052 above 2048"),
    (dict(n_slots=0), capi.MOT_EUNSUPPORTED, b"n_slots 0 outside [1, 4]"),
    (dict(n_slots=5), capi.MOT_EUNSUPPORTED, b"n_slots 5 outside [1, 4]"),
    (dict(bpt=0), capi.MOT_EUNSUPPORTED, b"bytes_per_token 0"),
    (dict(dtype=2), capi.MOT_EINVAL, b"bad dtype 2"),
    (dict(id_source=capi.IDS_NONE), capi.MOT_EINVAL, b"bad id_source 0"),
    (dict(struct_size=8), capi.MOT_EINVAL, b"struct_size"),
    (dict(ids=None), capi.MOT_EINVAL, b"ids missing"),
    (dict(tokens=None), capi.MOT_EINVAL, b"tokens"),
    (dict(out_ids=PTR), capi.MOT_EINVAL, b"MOT_IDS_FROM_TTB"),
    (dict(slot={(0, "tok_table"): None}), capi.MOT_EINVAL, b"slot 0 has a null"),
    (dict(slot={(1, "byte_table"): None}), capi.MOT_EINVAL, b"slot 1 has a null"),
    (dict(slot={(2, "weight"): None}), capi.MOT_EINVAL, b"slot 2 has a null"),
    (dict(slot={(1, "weight"): PTR + 4}), capi.MOT_EINVAL, b"16-byte aligned"),
])
def test_refusals_come_back_before_any_launch(kw, want, says):
    """With a non-empty batch too: the pointers are fake, so a launch would fault."""
    for n_rows in (0, 2):
        d = _desc(n_rows=n_rows, **dict(kw))
        assert _rc(d) == (want, want), capi.lib.mot_last_error()
        assert says in capi.lib.mot_last_error(), capi.lib.mot_last_error()
        if kw.keys() & {"token_dim", "byte_dim", "out_dim", "dtype", "id_source", "bpt", "n_slots", "struct_size"}:   # what a size query can see
            assert capi.lib.mot_value_mix_workspace_bytes(C.byref(d), 0) == 0
            assert capi.lib.mot_value_mix_workspace_bytes(C.byref(d), 1) == 0


def test_an_unused_slot_may_be_null_and_a_used_one_needs_its_out():
    d = _desc(n_slots=2, slot={(2, "tok_table"): None, (3, "weight"): None})
    assert _rc(d) == (capi.MOT_OK, capi.MOT_OK)
    d = _desc(n_rows=2, slot={(1, "out"): None})
    assert capi.lib.mot_value_mix_fwd(C.byref(d), None) == capi.MOT_EINVAL and b"slot 1 has a null out" in capi.lib.mot_last_error()


def test_bad_pull_direction_and_table_source():
    ttb = dict(id_source=capi.IDS_FROM_TTB, ids=None, ttb=PTR, ttb_rows=100, ttb_elem_bytes=2, pull_dir=capi.PULL_LEFT)
    for n_rows in (0, 2):
        for kw, says in ((dict(pull_dir=3), b"bad pull_dir 3"), (dict(pull_dir=-1), b"bad pull_dir -1"), (dict(ttb_elem_bytes=8), b"ttb_elem_bytes"),
                         (dict(ttb=None), b"ttb missing")):
            d = _desc(n_rows=n_rows, **{**ttb, **kw})
            assert capi.lib.mot_value_mix_fwd(C.byref(d), None) == capi.MOT_EINVAL
            assert says in capi.lib.mot_last_error(), capi.lib.mot_last_error()
    d = _desc(**ttb)   # the backward takes the ids the forward used
    assert capi.lib.mot_value_mix_bwd(C.byref(d), C.byref(_grads()), None) == capi.MOT_EUNSUPPORTED
    assert capi.lib.mot_value_mix_workspace_bytes(C.byref(d), 1) == 0


def test_backward_wants_its_buffers():
    d = _desc(n_rows=2)
    assert capi.lib.mot_value_mix_bwd(C.byref(d), C.byref(_grads({(1, "d_weight"): None})), None) == capi.MOT_EINVAL
    assert b"slot 1 has a grad_out but a null" in capi.lib.mot_last_error()
    assert capi.lib.mot_value_mix_bwd(C.byref(_desc(n_rows=2, slot={(2, "out_row_rnorm"): None})), C.byref(_grads()), None) == capi.MOT_EINVAL
    assert b"out_row_rnorm" in capi.lib.mot_last_error()
    assert capi.lib.mot_value_mix_bwd(C.byref(d), None, None) == capi.MOT_EINVAL
    g = _grads()
    g.struct_size = 8
    assert capi.lib.mot_value_mix_bwd(C.byref(d), C.byref(g), None) == capi.MOT_EINVAL
    # a slot without a grad_out is skipped: none of its buffers is looked at
    d0 = _desc(slot={(1, "out_row_rnorm"): None})
    assert capi.lib.mot_value_mix_bwd(C.byref(d0), C.byref(_grads({(1, "grad_out"): None, (1, "d_tok"): None})), None) == capi.MOT_OK
    # the token order's limit
    assert capi.lib.mot_value_mix_bwd(C.byref(_desc(tok_rows=1 << 21)), C.byref(_grads()), None) == capi.MOT_EUNSUPPORTED
    assert capi.lib.mot_value_mix_fwd(C.byref(_desc(tok_rows=1 << 21)), None) == capi.MOT_OK


def test_workspace_queries_and_a_workspace_that_is_too_small():
    K = 1024 + 16 * 64
    d = _desc(n_rows=2, tokens_per_row=64)
    fwd, bwd = capi.lib.mot_value_mix_workspace_bytes(C.byref(d), 0), capi.lib.mot_value_mix_workspace_bytes(C.byref(d), 1)
    assert 128 * K * 4 <= fwd < 128 * K * 4 + 4096                                       # u of the 128 tokens, nothing else
    assert bwd >= 128 * 1024 * 4 + 128 * 1024 * 4 + 128 * K * 4 + 128 * 1024 * 4           # du's two parts, u, dy
    assert capi.lib.mot_value_mix_workspace_bytes(C.byref(_desc()), 0) == 0 == capi.lib.mot_value_mix_workspace_bytes(C.byref(_desc()), 1)   # an empty batch
    for ws_bytes in (0, fwd - 1):
        d.workspace, d.workspace_bytes = PTR, ws_bytes
        assert capi.lib.mot_value_mix_fwd(C.byref(d), None) == capi.MOT_EWORKSPACE
        assert str(fwd).encode() in capi.lib.mot_last_error()
    d.workspace, d.workspace_bytes = PTR, bwd - 1
    assert capi.lib.mot_value_mix_bwd(C.byref(d), C.byref(_grads()), None) == capi.MOT_EWORKSPACE
    # one slot's rows plus the shared order, whatever n_slots is
    for n in (1, 2, 4):
        assert capi.lib.mot_value_mix_workspace_bytes(C.byref(_desc(n_rows=2, tokens_per_row=64, n_slots=n)), 1) == bwd
        assert capi.lib.mot_value_mix_workspace_bytes(C.byref(_desc(n_rows=2, tokens_per_row=64, n_slots=n)), 0) == fwd
    # ids from the token->byte table: room for the two int64 id tensors
    t = _desc(n_rows=2, tokens_per_row=64, id_source=capi.IDS_FROM_TTB, ids=None, ttb=PTR, ttb_rows=100, ttb_elem_bytes=2)
    assert capi.lib.mot_value_mix_workspace_bytes(C.byref(t), 0) >= fwd + 2 * 128 * 16 * 8
    # bf16 at the runs' shape: the one gather-GEMM launch builds no u; a shape it does not take (out_dim 2048) does
    h = _desc(n_rows=2, tokens_per_row=64, dtype=capi.BF16)
    assert capi.lib.mot_value_mix_workspace_bytes(C.byref(h), 0) == 0
    h2 = _desc(n_rows=2, tokens_per_row=64, dtype=capi.BF16, out_dim=2048)
    assert 128 * K * 2 <= capi.lib.mot_value_mix_workspace_bytes(C.byref(h2), 0) < 128 * K * 2 + 4096
    # the runs' step: u, dy and the byte part of du stay one slab; the token part of du is the whole batch in fp32
    step = _desc(n_rows=1, tokens_per_row=65536, dtype=capi.BF16, tok_rows=50257)
    b = capi.lib.mot_value_mix_workspace_bytes(C.byref(step), 1)
    assert 65536 * 1024 * 4 < b < 65536 * 1024 * 4 + 16384 * (K * 2 + 1024 * 4 + 1024 * 2) + K * 1024 * 2 + (64 << 20)


def test_module_surface():
    torch.manual_seed(0)
    m = M.MotValueEmbeds(token_vocab_size=50257, token_dim=1024, byte_dim=64)
    sd = m.state_dict()
    want = [f"value_byte_mixin_weights.{j}" for j in range(3)] + [f"value_embeds_bytes.{j}.weight" for j in range(3)] + \
           [f"value_embeds_toks.{j}.weight" for j in range(3)]
    assert sorted(sd) == want                                                   # the runs' attribute names; the ttb is no state
    assert all(tuple(sd[f"value_embeds_toks.{j}.weight"].shape) == (50257, 1024) for j in range(3))
    assert all(tuple(sd[f"value_embeds_bytes.{j}.weight"].shape) == (50257, 64) for j in range(3))     # the runs allocate token_vocab_size rows
    K = 1024 + 16 * 64
    bound = 3 ** 0.5 * 0.5 / K ** 0.5                                           # init_linear, runs/9_*.py:134-137
    for w in m.value_byte_mixin_weights:
        assert tuple(w.shape) == (1024, K) and isinstance(w, torch.nn.Parameter)
        w = w.detach()
        assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.99 * bound
        assert abs(float(w.std()) - 0.5 / K ** 0.5) < 0.01 * 0.5 / K ** 0.5 and abs(float(w.mean())) < 1e-2 * bound
    assert isinstance(m.value_embeds_toks, torch.nn.ModuleList) and isinstance(m.value_embeds_toks[0], torch.nn.Embedding)
    assert isinstance(m.value_byte_mixin_weights, torch.nn.ParameterList)
    assert m.bpt == 16 and m.out_dim == 1024 and m.byte_vocab_size == 458 and (m.pad_byte, m.eot_byte) == (456, 457) and m.ttb is None
    small = M.MotValueEmbeds(40, 32, 8, bytes_per_token=8, n=2, byte_vocab_size=30, out_dim=64, ttb=torch.from_numpy(vm.case_ttb("t32_b8_bpt8")))
    assert tuple(small.value_byte_mixin_weights[1].shape) == (64, 96) and tuple(small.ttb.shape) == (40, 8) and len(small.state_dict()) == 6
    m2 = M.MotValueEmbeds(50257, 1024, 64)
    m2.load_state_dict(sd)                                                      # an existing checkpoint loads
    for n in (0, 5):
        with pytest.raises(ValueError, match="1..4"):
            M.MotValueEmbeds(40, 32, 8, n=n)
    with pytest.raises(ValueError, match="byte_inputs"):
        m(torch.zeros(8, dtype=torch.int32))                                    # no ttb attached, no ids given
    with pytest.raises(RuntimeError, match="HIP device only"):
        m(torch.zeros(8, dtype=torch.int32), torch.zeros(128, dtype=torch.int64))


def test_functional_refuses_cpu_and_mismatched_inputs():
    Vt, Vb, W = torch.zeros(10, 32), torch.zeros(458, 8), torch.zeros(32, 96)
    toks, ids = torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, 32, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="HIP device only"):
        mot.value_mix(toks, [Vt], [Vb], [W], bpt=8, ids=ids)
    with pytest.raises(RuntimeError, match="HIP device only"):
        Fm.value_mix_backward([torch.zeros(1, 4, 32)], toks, [Vt], [Vb], [W], bpt=8, ids=ids, norm_out=False)
    # (shape and dtype checks: the descriptor builder runs them before anything touches a device)
    with pytest.raises(TypeError, match="share one dtype"):
        Fm._value_mix_desc(toks, [Vt], [Vb.bfloat16()], [W], 8, True, None, "value_mix")
    with pytest.raises(TypeError, match="float32 or bfloat16"):
        Fm._value_mix_desc(toks, [Vt.double()], [Vb.double()], [W.double()], 8, True, None, "value_mix")
    with pytest.raises(ValueError, match="one of each per slot"):
        Fm._value_mix_desc(toks, [Vt, Vt], [Vb], [W], 8, True, None, "value_mix")
    with pytest.raises(ValueError, match="1..4 are built"):
        Fm._value_mix_desc(toks, [Vt] * 5, [Vb] * 5, [W] * 5, 8, True, None, "value_mix")
    with pytest.raises(ValueError, match="token_dim \\+ bpt\\*byte_dim"):
        Fm._value_mix_desc(toks, [Vt], [Vb], [torch.zeros(32, 64)], 8, True, None, "value_mix")
    with pytest.raises(ValueError, match="must be 2-D of shape"):
        Fm._value_mix_desc(toks, [Vt, torch.zeros(11, 32)], [Vb, Vb], [W, W], 8, True, None, "value_mix")


@pytest.mark.parametrize("name", list(vm.CASES))
def test_restatement_reproduces_the_reference(name):
    Dt, Db, bpt, Do, B, T, S, Vt, std, seed = vm.CASES[name]
    toks, padded, pulled = (GOLDEN[vm.key(name, k)] for k in ("tokens", "ids_padded", "ids_pulled"))
    np.testing.assert_array_equal(toks, vm.case_tokens(name))
    np.testing.assert_array_equal(padded.reshape(B, T, bpt), vm.case_ttb(name)[toks])
    slots = vm.case_tables(name)
    assert len(slots) == S
    r64 = vm.run(toks, pulled, slots, bpt=bpt, dtype=torch.float64)           # eps None: the float64 epsilon, as the reference's run
    r32 = vm.run(toks, pulled, slots, bpt=bpt, dtype=torch.float32)
    r16 = vm.run(toks, pulled, slots, bpt=bpt, dtype=torch.bfloat16)
    r16e = vm.run(toks, pulled, slots, bpt=bpt, dtype=torch.bfloat16, eps=vm.F32_EPS)
    for j in range(S):
        for what in vm.QUANTITIES:
            ref = GOLDEN[vm.key(name, f"{j}/f64/{what}")]
            assert r64[j][what].shape == ref.shape, what
            err = vm.rel_err(r64[j][what], ref)
            print(f"{name} slot {j} {what}: restatement vs reference float64 {err:.2e}")
            assert err <= 1e-15, (what, err)
            assert 0 < float(GOLDEN[vm.key(name, f"{j}/f32err/{what}")]) < (1e-5 if std == 1.0 else 1e-3)
            assert 0 < float(GOLDEN[vm.key(name, f"{j}/bf16err/{what}")]) < 2.0 ** -5
        # the float32 and bfloat16 runs: the same torch operations on the same shapes in the same order, so the same bits
        np.testing.assert_array_equal(r32[j]["out"], GOLDEN[vm.key(name, f"{j}/f32/out")].astype(np.float64))
        ref16 = GOLDEN[vm.key(name, f"{j}/bf16/out")].astype(np.float64)
        np.testing.assert_array_equal(r16[j]["out"], ref16)
        # F.rms_norm(eps=None) on bfloat16 rows takes the float32 epsilon (its fp32 opmath type): what MotValueMixDesc.eps <= 0 means
        np.testing.assert_array_equal(r16e[j]["out"], ref16)
    if std != 1.0:   # and with 2^-7 the small-magnitude rows are off by whole bfloat16 steps
        x16b = vm.run(toks, pulled, slots, bpt=bpt, dtype=torch.bfloat16, eps=2.0 ** -7)[0]["out"]
        ref16 = GOLDEN[vm.key(name, "0/bf16/out")].astype(np.float64)
        assert np.abs(x16b - ref16).max() > 2.0 ** -6 * np.abs(ref16).max()


def test_fixture_covers_the_eot_positions_and_stays_small():
    name = "t32_b8_bpt8"
    Dt, Db, bpt, Do, B, T, S, Vt, std, seed = vm.CASES[name]
    toks = GOLDEN[vm.key(name, "tokens")]
    e = Vt - 1
    assert toks[0, 0] == e and toks[0, T // 2] == e and toks[B - 1, 3] == e and toks[B - 1, 4] == e
    assert (GOLDEN[vm.key(name, "ids_pulled")] != GOLDEN[vm.key(name, "ids_padded")]).any()      # the pull moved bytes
    assert vm.CASES["t32_b8_bpt8"][:7] == (32, 8, 8, 32, 2, 24, 3) and vm.CASES["t64_b24_bpt4"][:7] == (64, 24, 4, 64, 2, 24, 2)
    assert any(c[2] == 16 for c in vm.CASES.values()) and any(c[8] == 0.02 for c in vm.CASES.values())
    assert vm.GOLDEN.stat().st_size < (1 << 20)
    assert str(GOLDEN["torch_version"])
