"""-m gpu: the pure-concatenation mixin x = norm(cat(token row, byte rows)) (mode="concat", MOT_MIX_CONCAT;
modded-nanogpt/runs/711_*.py:224-232), forward and backward, against the reference's own outputs (tests/golden/pure_concat.npz)
and the float64 restatement of tests/pure_concat_ref.py.

Bars, all the project's existing ones for the gather + norm family:
  * fp32 forward: |hip - ref| <= 1e-6 + 1e-6 |ref| elementwise (util_gpu.assert_close);
  * gradients: max|hip - ref64| <= 2e-5 max|ref64| per tensor (tests/test_gpu_backward.py, grads.npz); two GPU results whose atomic
    order differs are each within that of the exact gradient, so 2x between them (as test_backward_is_capturable_in_a_hip_graph);
  * bf16 forward: at most one bf16 step from the float64 result rounded once (or 2e-6 of the row's largest entry), > 98 % of the
    elements identical; bf16 backward: 2e-5 as above (tests/test_gpu_bf16.py).
"""
import numpy as np
import pytest
import torch

import golden_inputs as gi
import pure_concat_ref as pc
from oracle import oracle as orc
from util_gpu import DEV, assert_close, dev, f32, host, rel

pytestmark = pytest.mark.gpu
TOL = 2e-5
EPS32 = float(np.finfo(np.float32).eps)


def ulps(got, ref):
    """Distance in bf16 steps between two arrays of bf16-representable float32 values (as tests/test_gpu_bf16.py counts them)."""
    def ordinal(a):
        b = (np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) >> 16).astype(np.int64)
        return np.where(b & 0x8000, -(b & 0x7FFF), b & 0x7FFF)
    return np.abs(ordinal(got) - ordinal(ref))


def ref_kw(kw):
    """The restatement normalises the output unless told otherwise (run 711 does); the kernel's norm_out defaults to off."""
    return {"norm_out": False, **kw}


@pytest.fixture(scope="module")
def mot():
    import mixture_of_tokenizers_amd as m
    return m


@pytest.fixture(scope="module")
def golden():
    return pc.load_golden()


def ids_of(toks, tab, bpt, pull="left"):
    padded = orc.tokens_to_bytes(toks, tab.astype(np.float32))
    if pull == "left":
        return padded, orc.pull_from_left(padded, bpt, gi.PAD, gi.EOT)
    if pull == "right":
        return padded, orc.pull_from_right(padded, bpt, gi.PAD, gi.EOT)
    return padded, padded


def forward64(toks, ids_a, ids_b, Et, Eb, *, bpt, eps=EPS32, scale_tok=None, scale_byte=None, **kw):
    """The float64 restatement, one batch row at a time (65 536 x 1024 float64 intermediates would be 0.5 GB each)."""
    t = lambda a: None if a is None else torch.tensor(np.asarray(a), dtype=torch.float64)
    rows = []
    with torch.no_grad():
        for b in range(toks.shape[0]):
            rows.append(pc.forward(toks[b:b + 1], ids_a[b:b + 1], None if ids_b is None else ids_b[b:b + 1], t(Et), t(Eb), bpt=bpt, eps=eps,
                                   scale_tok=t(scale_tok), scale_byte=t(scale_byte), **kw))
    return torch.cat(rows).numpy()


# ------------------------------------------------------------------------------------------------ forward, fp32
@pytest.mark.parametrize("name", list(pc.CASES))
def test_forward_fixture_cases(mot, golden, name):
    Dt, Db, bpt, B, T, Vt, dual, seed = pc.CASES[name]
    toks, padded, pulled = (golden[pc.key(name, k)] for k in ("tokens", "ids_padded", "ids_pulled"))
    Et, Eb, _ = pc.case_tables(name)
    x = mot.embed_mix(dev(toks), dev(f32(Et)), dev(f32(Eb)), mode="concat", bpt=bpt, ids_a=dev(pulled.astype(np.int64)),
                      ids_b=dev(padded.astype(np.int64)) if dual else None, norm_out=True)
    mot.check_status()
    assert x.shape == (B, T, Dt + bpt * Db) and x.dtype == torch.float32
    ref32 = golden[pc.key(name, "f32/out")]
    print(f"{name}: max |hip - reference fp32| {np.abs(host(x) - ref32).max():.3e}, vs float64 {np.abs(host(x) - golden[pc.key(name, 'f64/out')]).max():.3e}")
    assert_close(host(x), ref32)
    # the same from the token->byte table, pulled in-kernel
    r = mot.embed_mix(dev(toks), dev(f32(Et)), dev(f32(Eb)), mode="concat", bpt=bpt, ttb=dev(pc.case_ttb(name)), pull="left", add_padded=dual,
                      norm_out=True, return_ids=True)
    np.testing.assert_array_equal(host(r.ids_pulled), pulled)
    np.testing.assert_array_equal(host(r.ids_padded), padded)
    assert torch.equal(r.x, x)


def test_forward_run711_dims(mot):
    """64 x 1024 tokens at token_dim 512, byte_dim 32, bpt 16 (model_dim 1024) against the float64 restatement."""
    Dt, Db, bpt, Vt, B, T = 512, 32, 16, 8192, 64, 1024
    tab = gi.synth_ttb(7201, Vt, bpt, "left")
    toks = gi.fineweb_like_tokens(7202, B, T, vocab=Vt, eot_p=1.0 / 700)
    Et, Eb = f32(gi.normal_table(7203, Vt, Dt)), f32(gi.normal_table(7204, gi.BYTE_VOCAB, Db))
    padded, pulled = ids_of(toks, tab, bpt)
    r = mot.embed_mix(dev(toks), dev(Et), dev(Eb), mode="concat", bpt=bpt, ttb=dev(tab), pull="left", norm_out=True, return_ids=True)
    mot.check_status()
    np.testing.assert_array_equal(host(r.ids_pulled), pulled)
    ref = forward64(toks, pulled, None, Et, Eb, bpt=bpt)
    got = host(r.x)
    print(f"run-711 dims: max |hip - float64| {np.abs(got - ref).max():.3e}")
    assert_close(got, ref)
    # equal bits between two runs of the forward, and between the in-kernel ids and the same ids given
    r2 = mot.embed_mix(dev(toks), dev(Et), dev(Eb), mode="concat", bpt=bpt, ttb=dev(tab), pull="left", norm_out=True)
    assert torch.equal(r2, r.x)
    assert torch.equal(mot.embed_mix(dev(toks), dev(Et), dev(Eb), mode="concat", bpt=bpt, ids_a=r.ids_pulled, norm_out=True), r.x)


@pytest.mark.parametrize("Dt,Db,bpt,kw", [
    (512, 32, 16, dict(norm_tok=True, norm_byte=True, norm_out=True, scaled=True)),     # per-embedding norms and scalars, as runs/71041
    (512, 32, 16, dict(norm_tok=True, norm_byte=True, scaled=True)),                     # no outer norm, as runs/71081
    (96, 8, 16, dict(norm_byte=True, norm_out=True)),                                     # model_dim 224: a last chunk that is half used
    (24, 8, 8, dict(norm_tok=True, norm_out=True)),
    (1024, 64, 16, dict(norm_out=True)),                                                  # model_dim 2048, the widest built
    (512, 32, 16, dict(norm_out=True, dual=True)),
    (512, 32, 16, dict(norm_byte=True, norm_out=True, dual=True)),                        # norm(E[a] + E[b]) per slot
    (24, 8, 8, dict(norm_byte=True, norm_out=True, dual=True, scaled=True)),
])
def test_forward_variants_vs_float64(mot, Dt, Db, bpt, kw):
    kw = dict(kw)
    scaled, dual = kw.pop("scaled", False), kw.pop("dual", False)
    Vt, B, T, seed = 700, 3, 333, 7300 + Dt + bpt
    tab = gi.synth_ttb(seed, Vt, bpt, "left")
    toks = gi.edge_tokens(seed + 1, B, T, Vt, eot_p=0.05)
    Et, Eb = f32(gi.normal_table(seed + 2, Vt, Dt)), f32(gi.normal_table(seed + 3, gi.BYTE_VOCAB, Db))
    padded, pulled = ids_of(toks, tab, bpt)
    st, sb = (1.3, 0.6) if scaled else (None, None)
    ref = forward64(toks, pulled, padded if dual else None, Et, Eb, bpt=bpt, scale_tok=st, scale_byte=sb, **ref_kw(kw))
    gkw = dict(kw)
    if scaled:
        gkw.update(scale_tok=torch.tensor([st], device=DEV), scale_byte=torch.tensor([sb], device=DEV))
    x = mot.embed_mix(dev(toks), dev(Et), dev(Eb), mode="concat", bpt=bpt, ttb=dev(tab), pull="left", add_padded=dual, **gkw)
    mot.check_status()
    print(f"{Dt}+{bpt}x{Db} {kw} dual={dual}: max |hip - float64| {np.abs(host(x) - ref).max():.3e}")
    # outputs without the outer norm are not O(1) per element by construction but are here (unit-variance tables, scalars near 1)
    assert_close(host(x), ref)


# ------------------------------------------------------------------------------------------------ ids, counters
@pytest.mark.parametrize("pull", ["left", "right", None])
def test_ids_in_kernel_equal_ids_given_and_sum_mode(mot, pull):
    Dt, Db, bpt, Vt, B, T = 64, 4, 16, 300, 5, 257
    tab = gi.synth_ttb(7401, Vt, bpt, "right" if pull == "right" else "left")
    toks = gi.edge_tokens(7402, B, T, Vt, eot_p=0.08)
    Et, Eb = dev(f32(gi.normal_table(7403, Vt, Dt))), dev(f32(gi.normal_table(7404, gi.BYTE_VOCAB, Db)))
    padded, pulled = ids_of(toks, tab, bpt, pull)
    cnt, cnt_sum = torch.zeros(4, dtype=torch.int64, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV)
    r = mot.embed_mix(dev(toks), Et, Eb, mode="concat", bpt=bpt, ttb=dev(tab), pull=pull, norm_out=True, return_ids=True, counters=cnt)
    s = mot.embed_mix(dev(toks), Et, Eb, mode="sum", bpt=bpt, ttb=dev(tab), pull=pull, norm_out=True, return_ids=True, counters=cnt_sum)
    mot.check_status()
    np.testing.assert_array_equal(host(r.ids_padded), padded)
    np.testing.assert_array_equal(host(r.ids_pulled), pulled)
    assert torch.equal(r.ids_padded, s.ids_padded) and torch.equal(r.ids_pulled, s.ids_pulled)
    assert torch.equal(cnt, cnt_sum) and cnt.tolist()[:2] == [B * T, B * T * bpt]
    given = mot.embed_mix(dev(toks), Et, Eb, mode="concat", bpt=bpt, ids_a=dev(pulled), norm_out=True)
    assert torch.equal(given, r.x)
    # two id tensors: in-kernel (pulled + padded) against the same two tensors given
    two = mot.embed_mix(dev(toks), Et, Eb, mode="concat", bpt=bpt, ttb=dev(tab), pull=pull, add_padded=True, norm_out=True)
    assert torch.equal(two, mot.embed_mix(dev(toks), Et, Eb, mode="concat", bpt=bpt, ids_a=dev(pulled), ids_b=dev(padded), norm_out=True))


def test_out_of_range_ids_are_flagged_not_faulted_on(mot):
    Dt, Db, bpt, Vt = 64, 4, 16, 50
    Et, Eb = dev(f32(gi.normal_table(7411, Vt, Dt))), dev(f32(gi.normal_table(7412, gi.BYTE_VOCAB, Db)))
    toks = np.array([[1, 2, Vt + 5, 3]], dtype=np.int32)
    ids = np.zeros((1, 4 * bpt), dtype=np.int64)
    ids[0, 7] = 9999
    x = mot.embed_mix(dev(toks), Et, Eb, mode="concat", bpt=bpt, ids_a=dev(ids), norm_out=True)
    torch.cuda.synchronize()
    with pytest.raises(IndexError):
        mot.check_status()
    assert torch.isfinite(x).all()


# ------------------------------------------------------------------------------------------------ gradients
GRAD_CASES = [
    # Dt, Db, bpt, Vt, B, T, kw
    (512, 32, 16, 2048, 4, 300, dict(norm_out=True)),                                               # run 711: 64-column chunks, split row
    (512, 32, 16, 2048, 2, 200, dict(norm_tok=True, norm_byte=True, norm_out=True, scaled=True)),
    (512, 32, 16, 2048, 2, 200, dict(norm_tok=True, norm_byte=True, scaled=True)),
    (64, 4, 16, 300, 3, 150, dict(norm_out=True)),
    (24, 8, 8, 300, 3, 150, dict(norm_out=True)),                                                   # ragged row: the general kernel
    (96, 8, 16, 300, 2, 150, dict(norm_tok=True, norm_byte=True, norm_out=True, scaled=True)),
    (512, 32, 16, 2048, 2, 200, dict(norm_out=True, dual=True)),
    (512, 32, 16, 2048, 2, 200, dict(norm_byte=True, norm_out=True, dual=True, scaled=True)),
    (24, 8, 8, 300, 2, 150, dict(norm_byte=True, norm_out=True, dual=True)),
]


def _grad_inputs(Dt, Db, bpt, Vt, B, T, seed, repeated=False):
    tab = gi.synth_ttb(seed, Vt, bpt, "left")
    toks = gi.fineweb_like_tokens(seed + 1, B, T, vocab=Vt, eot_p=0.01)
    if repeated:
        toks[:] = 7                       # every position the same token: one run, one table row takes every add
        toks[0, ::5] = 9
    Et, Eb = f32(gi.normal_table(seed + 2, Vt, Dt)), f32(gi.normal_table(seed + 3, gi.BYTE_VOCAB, Db))
    g = f32(np.random.RandomState(seed + 4).standard_normal((B, T, Dt + bpt * Db)))
    padded, pulled = ids_of(toks, tab, bpt)
    return tab, toks, Et, Eb, g, padded, pulled


def _check_grads(got, ref, scaled, what=""):
    for k, r in (("tok_table", "d_tok"), ("byte_table", "d_byte")):
        print(f"{what} {k}: {float(rel(host(got[k]), ref[r])):.3e}")
    assert rel(host(got["tok_table"]), ref["d_tok"]) < TOL
    assert rel(host(got["byte_table"]), ref["d_byte"]) < TOL
    if scaled:
        big = max(abs(ref["d_scale_tok"]), abs(ref["d_scale_byte"]))
        assert abs(float(got["scale_tok"]) - ref["d_scale_tok"]) < TOL * big
        assert abs(float(got["scale_byte"]) - ref["d_scale_byte"]) < TOL * big


@pytest.mark.parametrize("with_order", [False, True])
@pytest.mark.parametrize("Dt,Db,bpt,Vt,B,T,kw", GRAD_CASES)
def test_backward_vs_float64(mot, Dt, Db, bpt, Vt, B, T, kw, with_order):
    kw = dict(kw)
    scaled, dual = kw.pop("scaled", False), kw.pop("dual", False)
    tab, toks, Et, Eb, g, padded, pulled = _grad_inputs(Dt, Db, bpt, Vt, B, T, 7500 + Dt + Db + bpt)
    st, sb = (1.3, 0.6) if scaled else (None, None)
    ref = pc.run(toks, pulled, padded if dual else None, Et, Eb, g, bpt=bpt, eps=EPS32, scale_tok=st, scale_byte=sb, **ref_kw(kw))
    gkw = dict(kw)
    if scaled:
        gkw.update(scale_tok=torch.tensor([st], device=DEV), scale_byte=torch.tensor([sb], device=DEV))
    order = mot.functional.token_order(dev(toks), Vt) if with_order else None
    got = mot.functional.embed_mix_backward(dev(g), dev(toks), dev(Et), dev(Eb), mode="concat", bpt=bpt, ids_a=dev(pulled),
                                            ids_b=dev(padded) if dual else None, token_order=order, **gkw)
    mot.check_status()
    _check_grads(got, ref, scaled, f"{Dt}+{bpt}x{Db} {kw} order={with_order}")


@pytest.mark.parametrize("Dt,Db,bpt", [(512, 32, 16), (24, 8, 8)])
def test_backward_repeated_token_batch(mot, Dt, Db, bpt):
    Vt, B, T = 64, 2, 400
    tab, toks, Et, Eb, g, padded, pulled = _grad_inputs(Dt, Db, bpt, Vt, B, T, 7600 + Dt, repeated=True)
    ref = pc.run(toks, pulled, None, Et, Eb, g, bpt=bpt, eps=EPS32, norm_out=True)
    got = mot.functional.embed_mix_backward(dev(g), dev(toks), dev(Et), dev(Eb), mode="concat", bpt=bpt, ids_a=dev(pulled), norm_out=True)
    mot.check_status()
    _check_grads(got, ref, False, f"repeated {Dt}")
    assert not host(got["tok_table"])[[0, 1, 8, 10]].any()       # rows no position names stay zero


@pytest.mark.parametrize("name", list(pc.CASES))
def test_autograd_fixture_cases(mot, golden, name):
    """loss.backward() through ConcatFrontEnd (ids given) and through embed_mix with the ids pulled in-kernel, against the
    reference's float64 autograd."""
    Dt, Db, bpt, B, T, Vt, dual, seed = pc.CASES[name]
    toks, padded, pulled = (golden[pc.key(name, k)] for k in ("tokens", "ids_padded", "ids_pulled"))
    Et, Eb, g = pc.case_tables(name)
    Etp, Ebp = dev(f32(Et)).requires_grad_(True), dev(f32(Eb)).requires_grad_(True)
    x = mot.embed_mix(dev(toks), Etp, Ebp, mode="concat", bpt=bpt, ttb=dev(pc.case_ttb(name)), pull="left", add_padded=dual, norm_out=True)
    x.backward(dev(f32(g)))
    mot.check_status()
    assert_close(host(x), golden[pc.key(name, "f32/out")])
    assert rel(host(Etp.grad), golden[pc.key(name, "f64/d_tok")]) < TOL
    assert rel(host(Ebp.grad), golden[pc.key(name, "f64/d_byte")]) < TOL
    if not dual:
        fe = mot.ConcatFrontEnd(Vt, gi.BYTE_VOCAB, Dt, Db, bytes_per_token=bpt, ttb=torch.from_numpy(pc.case_ttb(name))).to(DEV)
        with torch.no_grad():
            fe.embed_tokens.weight.copy_(dev(f32(Et)))
            fe.embed_bytes.weight.copy_(dev(f32(Eb)))
        for byte_inputs in (dev(pulled.astype(np.int64)), None):
            fe.zero_grad(set_to_none=True)
            y = fe(dev(toks), byte_inputs)
            assert torch.equal(y, x.detach())
            y.backward(dev(f32(g)))
            assert rel(host(fe.embed_tokens.weight.grad), golden[pc.key(name, "f64/d_tok")]) < TOL
            assert rel(host(fe.embed_bytes.weight.grad), golden[pc.key(name, "f64/d_byte")]) < TOL
        one = fe(dev(toks[0]), dev(pulled[0].astype(np.int64)))    # a single sequence, as the reference's forward takes it (:303)
        assert one.shape == (1, T, Dt + bpt * Db) and torch.equal(one[0], x.detach()[0])


# ------------------------------------------------------------------------------------------------ bf16
@pytest.mark.parametrize("Dt,Db,bpt,Vt,B,T,kw,seed", [
    (512, 32, 16, 8192, 4, 1024, dict(norm_out=True), 7701),
    (256, 32, 8, 512, 3, 333, dict(norm_tok=True, norm_byte=True, norm_out=True), 7702),
    (1024, 64, 16, 512, 2, 70, dict(), 7703),
    (64, 8, 4, 300, 2, 70, dict(norm_out=True), 7704),
])
def test_bf16_forward_vs_float64(mot, Dt, Db, bpt, Vt, B, T, kw, seed):
    tab = gi.synth_ttb(seed + 1, Vt, bpt, "left")
    toks = gi.fineweb_like_tokens(seed, B, T, vocab=Vt, eot_p=0.01)
    Et, Eb = orc.bf16_round(gi.normal_table(seed + 2, Vt, Dt)), orc.bf16_round(gi.normal_table(seed + 3, gi.BYTE_VOCAB, Db))
    padded, pulled = ids_of(toks, tab, bpt)
    ref = forward64(toks, pulled, None, Et, Eb, bpt=bpt, eps=2.0 ** -7, **ref_kw(kw))
    r = mot.embed_mix(dev(toks), dev(Et).bfloat16(), dev(Eb).bfloat16(), mode="concat", bpt=bpt, ttb=dev(tab), pull="left", return_ids=True, **kw)
    mot.check_status()
    assert r.x.dtype == torch.bfloat16 and r.x.shape == (B, T, Dt + bpt * Db)
    np.testing.assert_array_equal(host(r.ids_pulled), pulled)
    got = host(r.x.float())
    row_max = np.abs(ref).max(axis=-1, keepdims=True)
    ok = (ulps(got, orc.bf16_round(ref)) <= 1) | (np.abs(got.astype(np.float64) - ref) <= 2e-6 * row_max)
    print(f"bf16 {Dt}+{bpt}x{Db}: identical {(got == orc.bf16_round(ref)).mean():.4f}, max steps {ulps(got, orc.bf16_round(ref)).max()}")
    assert ok.all()
    assert (got == orc.bf16_round(ref)).mean() > 0.98


@pytest.mark.parametrize("Dt,Db,bpt,Vt,B,T,kw,seed", [
    (512, 32, 16, 4096, 4, 512, dict(norm_out=True), 7801),
    (512, 32, 16, 4096, 2, 300, dict(norm_tok=True, norm_byte=True, norm_out=True, scaled=True), 7802),
    (48, 24, 4, 300, 2, 100, dict(norm_out=True), 7803),
])
def test_bf16_backward_vs_float64(mot, Dt, Db, bpt, Vt, B, T, kw, seed):
    kw = dict(kw)
    scaled = kw.pop("scaled", False)
    tab = gi.synth_ttb(seed + 1, Vt, bpt, "left")
    toks = gi.fineweb_like_tokens(seed, B, T, vocab=Vt, eot_p=0.01)
    Et, Eb = orc.bf16_round(gi.normal_table(seed + 2, Vt, Dt)), orc.bf16_round(gi.normal_table(seed + 3, gi.BYTE_VOCAB, Db))
    g = orc.bf16_round(np.random.RandomState(seed + 4).standard_normal((B, T, Dt + bpt * Db)))
    padded, pulled = ids_of(toks, tab, bpt)
    st, sb = (1.3, 0.6) if scaled else (None, None)
    ref = pc.run(toks, pulled, None, Et, Eb, g, bpt=bpt, eps=2.0 ** -7, scale_tok=st, scale_byte=sb, **ref_kw(kw))
    gkw = dict(kw)
    if scaled:
        gkw.update(scale_tok=torch.tensor([st], device=DEV), scale_byte=torch.tensor([sb], device=DEV))
    got = mot.functional.embed_mix_backward(dev(g).bfloat16(), dev(toks), dev(Et).bfloat16(), dev(Eb).bfloat16(), mode="concat", bpt=bpt,
                                            ids_a=dev(pulled), **gkw)
    mot.check_status()
    assert got["tok_table"].dtype == torch.float32
    _check_grads(got, ref, scaled, f"bf16 {Dt}+{bpt}x{Db}")


def test_bf16_autograd_rounds_the_gradients_once(mot):
    Dt, Db, bpt, Vt, B, T = 512, 32, 16, 1024, 2, 128
    tab, toks, Et, Eb, g, padded, pulled = _grad_inputs(Dt, Db, bpt, Vt, B, T, 7850)
    fe = mot.ConcatFrontEnd(Vt, gi.BYTE_VOCAB, Dt, Db, ttb=torch.from_numpy(tab)).to(DEV)
    with torch.no_grad():
        fe.embed_tokens.weight.copy_(dev(Et)); fe.embed_bytes.weight.copy_(dev(Eb))
    fe = fe.bfloat16()
    y = fe(dev(toks))
    y.backward(dev(g).bfloat16())
    assert y.dtype == torch.bfloat16 and fe.embed_tokens.weight.grad.dtype == torch.bfloat16
    ref = pc.run(toks, pulled, None, host(fe.embed_tokens.weight.float()), host(fe.embed_bytes.weight.float()), orc.bf16_round(g), bpt=bpt,
                 eps=2.0 ** -7, norm_out=True)
    assert rel(host(fe.embed_tokens.weight.grad.float()), ref["d_tok"]) < 2.0 ** -8 + TOL      # one rounding to bf16 of the fp32 sums
    assert rel(host(fe.embed_bytes.weight.grad.float()), ref["d_byte"]) < 2.0 ** -8 + TOL


# ------------------------------------------------------------------------------------------------ hipGraph
def test_forward_is_capturable_in_a_hip_graph(mot):
    Dt, Db, bpt, Vt, B, T = 512, 32, 16, 2048, 4, 512
    tab = dev(gi.synth_ttb(7901, Vt, bpt, "left"))
    Et, Eb = dev(f32(gi.normal_table(7902, Vt, Dt))), dev(f32(gi.normal_table(7903, gi.BYTE_VOCAB, Db)))
    toks = dev(gi.fineweb_like_tokens(7904, B, T, vocab=Vt, eot_p=0.01))
    out = torch.empty((B, T, Dt + bpt * Db), device=DEV)
    kw = dict(mode="concat", bpt=bpt, ttb=tab, pull="left", norm_tok=True, norm_byte=True, norm_out=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        mot.embed_mix(toks, Et, Eb, out=out, **kw)          # warm-up on the capture stream (allocates the workspace)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        mot.embed_mix(toks, Et, Eb, out=out, **kw)
    toks.copy_(dev(gi.fineweb_like_tokens(7905, B, T, vocab=Vt, eot_p=0.01)))     # new batch, same buffers
    Et.mul_(1.5)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, mot.embed_mix(toks, Et, Eb, **kw))


@pytest.mark.parametrize("Dt,Db,bpt", [(512, 32, 16), (24, 8, 8)])
def test_backward_is_capturable_in_a_hip_graph(mot, Dt, Db, bpt):
    Vt, B, T = 1024, 4, 300
    Et, Eb = dev(f32(gi.normal_table(7951, Vt, Dt))), dev(f32(gi.normal_table(7952, gi.BYTE_VOCAB, Db)))
    rs = np.random.RandomState(7953)
    toks = dev(gi.fineweb_like_tokens(7954, B, T, vocab=Vt, eot_p=0.01))
    ids = dev(rs.randint(0, gi.BYTE_VOCAB, (B, T * bpt)).astype(np.int64))
    g = dev(f32(rs.standard_normal((B, T, Dt + bpt * Db))))
    into = {"tok_table": torch.zeros_like(Et), "byte_table": torch.zeros_like(Eb)}
    kw = dict(mode="concat", bpt=bpt, ids_a=ids, norm_out=True, norm_byte=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        mot.functional.embed_mix_backward(g, toks, Et, Eb, into=into, **kw)     # warm-up: allocates the workspace
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        into["tok_table"].zero_(); into["byte_table"].zero_()
        mot.functional.embed_mix_backward(g, toks, Et, Eb, into=into, **kw)
    toks.copy_(dev(gi.fineweb_like_tokens(7955, B, T, vocab=Vt, eot_p=0.01)))
    ids.copy_(dev(rs.randint(0, gi.BYTE_VOCAB, (B, T * bpt)).astype(np.int64)))
    g.copy_(dev(f32(rs.standard_normal((B, T, Dt + bpt * Db)))))
    graph.replay()
    torch.cuda.synchronize()
    ref = mot.functional.embed_mix_backward(g, toks, Et, Eb, **kw)
    mot.check_status()
    assert rel(host(into["tok_table"]), host(ref["tok_table"])) < 2 * TOL      # two GPU results (atomic order differs)
    assert rel(host(into["byte_table"]), host(ref["byte_table"])) < 2 * TOL


# ------------------------------------------------------------------------------------------------ refusals
def test_functional_refusals(mot):
    toks = torch.zeros((1, 4), dtype=torch.int32, device=DEV)
    ids = torch.zeros((1, 64), dtype=torch.int64, device=DEV)
    Eb = torch.zeros(458, 32, device=DEV)
    with pytest.raises(NotImplementedError, match="tok_dim 30"):      # a 16-byte chunk would straddle the token / byte boundary
        mot.embed_mix(toks, torch.zeros(8, 30, device=DEV), Eb, mode="concat", bpt=16, ids_a=ids, norm_out=True)
    with pytest.raises(NotImplementedError, match="byte_dim 6"):
        mot.embed_mix(toks, torch.zeros(8, 64, device=DEV), torch.zeros(458, 6, device=DEV), mode="concat", bpt=16, ids_a=ids)
    with pytest.raises(NotImplementedError, match="multiples of 8"):  # bf16: 8 elements per 16 bytes
        mot.embed_mix(toks, torch.zeros(8, 64, device=DEV).bfloat16(), torch.zeros(458, 4, device=DEV).bfloat16(), mode="concat", bpt=16, ids_a=ids)
    with pytest.raises(ValueError, match="no weight"):
        mot.embed_mix(toks, torch.zeros(8, 512, device=DEV), Eb, mode="concat", bpt=16, ids_a=ids, weight=torch.zeros(1024, 1024, device=DEV))
    with pytest.raises(ValueError, match="no weight"):
        mot.embed_mix(toks, torch.zeros(8, 512, device=DEV).requires_grad_(True), Eb, mode="concat", bpt=16, ids_a=ids,
                      weight=torch.zeros(1024, 1024, device=DEV))
    with pytest.raises(NotImplementedError, match="> 2048"):
        mot.embed_mix(toks, torch.zeros(8, 2048, device=DEV), Eb, mode="concat", bpt=16, ids_a=ids)
    with pytest.raises(NotImplementedError, match="> 2048"):
        mot.functional.embed_mix_backward(torch.zeros(1, 4, 2560, device=DEV), toks, torch.zeros(8, 2048, device=DEV), Eb, mode="concat", bpt=16,
                                          ids_a=ids)
    # the backward wants the ids the forward produced, as SUM does; the forward-only seam gathers stay forward-only
    x = mot.embed_mix(toks, torch.zeros(8, 512, device=DEV), Eb, mode="concat", bpt=16, ids_a=ids)
    assert x.shape == (1, 4, 1024) and not x.any()
