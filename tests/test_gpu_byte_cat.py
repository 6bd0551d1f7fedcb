"""-m gpu: the bytes-only front-end and the byte value embeddings (functional.byte_cat, mot_byte_cat_fwd / _bwd;
modded-nanogpt/runs/5_bytes-in_bytes-valemb.py:225-232, 248, 305, 314), forward and backward, against the reference's own runs
(tests/golden/byte_cat.npz) and the float64 restatement of tests/byte_cat_ref.py evaluated on the device.

Bars, all the project's existing ones for the gather + norm family (copied from tests/test_gpu_pure_concat.py):
  * rows without a norm: the bits of table[ids];
  * fp32 forward: |hip - ref| <= 1e-6 + 1e-6 |ref| elementwise (util_gpu.assert_close);
  * bf16 forward: at most one bf16 step from the float64 result rounded once (or 2e-6 of the row's largest entry), > 98 % of the
    elements identical;
  * gradients: max|hip - ref64| <= 2e-5 max|ref64| per tensor, fp32 and bf16 (the accumulators are fp32 either way); two GPU results
    whose flush order differs agree within the same bar; a bf16 .grad is the fp32 sum rounded once: 2^-8 on top of the bar
    against float64, and between two runs one bf16 step of the element (two roundings of fp32 sums that differ in their last
    bits land on the same or on neighbouring bf16 values) on top of the bar.
The float64 reference is the restatement with the FLOAT32 epsilon, the one the kernels use for both dtypes: the fixture's float64
run took the float64 epsilon (F.rms_norm(eps=None) on float64 rows), which on the fixture's rows of magnitude 0.02 moves the result
by 1.5e-4; on its unit-variance cases the two agree to 1e-7 and the fixture's float64 arrays are compared as well.
"""
import itertools

import numpy as np
import pytest
import torch

import byte_cat_ref as bc
import golden_inputs as gi
from oracle import oracle as orc
from util_gpu import DEV, assert_close, dev, f32, host, rel

pytestmark = pytest.mark.gpu
TOL = 2e-5
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
FIXTURE = [(n, dt) for n in bc.CASES for dt in DTYPES if dt == "fp32" or bc.CASES[n][0] % 8 == 0]


def ulps(got, ref):
    """Distance in bf16 steps between two arrays of bf16-representable float32 values (as tests/test_gpu_bf16.py counts them)."""
    def ordinal(a):
        b = (np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) >> 16).astype(np.int64)
        return np.where(b & 0x8000, -(b & 0x7FFF), b & 0x7FFF)
    return np.abs(ordinal(got) - ordinal(ref))


@pytest.fixture(scope="module")
def mot():
    import mixture_of_tokenizers_amd as m
    return m


@pytest.fixture(scope="module")
def golden():
    return bc.load_golden()


def tabs_on(tables, dt):
    return [dev(t, DTYPES[dt]) for t in tables]


def ref64(ids, tables, norm, gs, bpt):
    """the float64 restatement on the device, with the kernels' epsilon"""
    return bc.run(ids, tables, norm, gs, bpt=bpt, dtype=torch.float64, device=DEV, eps=bc.F32_EPS)


def check_forward(outs, ids, tables, norm, ref, dt, what=""):
    """outs: device tensors; tables: float64 arrays of bf16 values; ref: float64 outputs."""
    B = outs[0].shape[0]
    for j, (o, tab) in enumerate(zip(outs, tables)):
        assert o.dtype == DTYPES[dt] and tuple(o.shape) == ref[j].shape
        got = host(o.float())
        if not norm[j]:
            clamped = np.where(np.asarray(ids) < tab.shape[0], ids, 0)
            np.testing.assert_array_equal(got, f32(tab)[clamped].reshape(B, -1, got.shape[-1]))      # a copy, bit for bit
        elif dt == "fp32":
            print(f"{what} out{j}: max |hip - float64| {np.abs(got - ref[j]).max():.3e}")
            assert_close(got, ref[j])
        else:
            once = orc.bf16_round(ref[j])
            row_max = np.abs(ref[j]).max(axis=-1, keepdims=True)
            ok = (ulps(got, once) <= 1) | (np.abs(got.astype(np.float64) - ref[j]) <= 2e-6 * row_max)
            print(f"{what} out{j}: identical {(got == once).mean():.4f}, max steps {ulps(got, once).max()}")
            assert ok.all()
            assert (got == once).mean() > 0.98


def check_grads(got, ref, what=""):
    for j, (g, r) in enumerate(zip(got, ref)):
        if r is None:
            assert g is None
            continue
        assert g.dtype == torch.float32
        print(f"{what} d_table{j}: {float(rel(host(g), r)):.3e}")
        assert rel(host(g), r) < TOL


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("name,dt", FIXTURE)
def test_forward_fixture_cases(mot, golden, name, dt):
    Db, bpt, B, T, Vt, norm, std, seed = bc.CASES[name]
    toks, padded, pulled = (golden[bc.key(name, k)] for k in ("tokens", "ids_padded", "ids_pulled"))
    tables, gs = bc.case_tables(name)
    tabs = tabs_on(tables, dt)
    given = mot.byte_cat(tabs, bpt=bpt, norm=norm, ids=dev(pulled.astype(np.int64)))
    cnt, cnt_sum = torch.zeros(4, dtype=torch.int64, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV)
    outs, ids_padded, ids_pulled = mot.functional._byte_cat_fwd(tabs, bpt=bpt, norm=norm, tokens=dev(toks), ttb=dev(bc.case_ttb(name)), pull="left",
                                                                return_ids=True, counters=cnt)
    mot.check_status()
    assert len(given) == len(outs) == len(norm)
    for a, b in zip(given, outs):
        assert torch.equal(a, b)                                   # the two id sources give the same bits
    # ids and counters: the reference's, and what SUM writes for the same tokens
    np.testing.assert_array_equal(host(ids_pulled), pulled)
    np.testing.assert_array_equal(host(ids_padded), padded)
    s = mot.embed_mix(dev(toks), torch.zeros(Vt, bpt * Db, device=DEV), dev(f32(tables[0])), mode="sum", bpt=bpt, ttb=dev(bc.case_ttb(name)),
                      pull="left", return_ids=True, counters=cnt_sum)
    assert torch.equal(s.ids_padded, ids_padded) and torch.equal(s.ids_pulled, ids_pulled)
    assert torch.equal(cnt, cnt_sum) and cnt.tolist()[:2] == [B * T, B * T * bpt]
    r = ref64(pulled, tables, norm, [None] * len(norm), bpt)
    check_forward(outs, pulled, tables, norm, r["out"], dt, f"{name} {dt}")
    for j, nm in enumerate(norm):
        if dt == "fp32":
            assert_close(host(outs[j]), golden[bc.key(name, f"f32/out{j}")])
            if std == 1.0:
                assert_close(host(outs[j]), golden[bc.key(name, f"f64/out{j}")])
        else:
            ref16 = torch.from_numpy(golden[bc.key(name, f"bf16/out{j}")]).view(torch.bfloat16).float().numpy()
            got = host(outs[j].float())
            print(f"{name} out{j}: identical to the reference's bf16 run {(got == ref16).mean():.4f}")
            assert (ulps(got, ref16) <= 1).all() and (got == ref16).mean() > 0.98
    again = mot.byte_cat(tabs, bpt=bpt, norm=norm, tokens=dev(toks), ttb=dev(bc.case_ttb(name)), pull="left")
    for a, b in zip(again, outs):
        assert torch.equal(a, b)                                   # two runs, the same bits


ODD = [
    # bpt, Db, rows per table, norm flags, largest id + 1
    (4, 12, (458,), (True,), 458),                                        # model_dim 48: less than one 64-lane pass
    (16, 48, (458, 458, 458, 458), (True, False, False, False), 458),     # slot boundaries inside a wave-load
    (16, 128, (458, 458), (True, False), 458),                            # model_dim 2048, the limit
    (16, 48, (458, 300, 64, 5), (True, False, True, False), 5),           # tables with different row counts in one call
    (8, 8, (458,), (False,), 458),
    (8, 8, (458, 458, 458), (False, True, False), 458),
] + [(8, 8, (458, 458), nm, 458) for nm in itertools.product((False, True), repeat=2)]


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("bpt,Db,rows,norm,top", ODD)
def test_forward_odd_shapes_vs_float64(mot, bpt, Db, rows, norm, top, dt):
    """B = 3 rows of T = 1, 15, 17, 37, 65 tokens: no multiple of the 16-token unit, and a 64-token window longer than the row."""
    if dt == "bf16" and Db % 8:
        Db = 2 * Db                                                 # bf16 takes 16-byte multiples of 8 elements: 4 x 24 instead of 4 x 12
    Vt, B, seed = 300, 3, 5100 + bpt + Db + len(rows)
    tables, _ = bc.make_inputs(seed, rows, Db, bpt, 1, 1)
    tabs = tabs_on(tables, dt)
    ttb = gi.synth_ttb(seed + 1, Vt, bpt, "left")
    for T in (1, 15, 17, 37, 65):
        toks = gi.edge_tokens(seed + T, B, T, Vt, eot_p=0.08)
        padded = orc.tokens_to_bytes(toks, ttb.astype(np.float32))
        pulled = orc.pull_from_left(padded, bpt, gi.PAD, gi.EOT)
        if top < 458:   # ids every table holds: given, not pulled
            ids = np.random.RandomState(seed + T).randint(0, top, (B, T * bpt)).astype(np.int64)
            outs = mot.byte_cat(tabs, bpt=bpt, norm=norm, ids=dev(ids))
        else:
            ids = pulled
            outs, _, got_ids = mot.byte_cat(tabs, bpt=bpt, norm=norm, tokens=dev(toks), ttb=dev(ttb), pull="left", return_ids=True)
            np.testing.assert_array_equal(host(got_ids), pulled)
        mot.check_status()
        r = ref64(ids, tables, norm, [None] * len(rows), bpt)
        check_forward(outs, ids, tables, norm, r["out"], dt, f"{bpt}x{Db} T={T} {dt}")


def test_out_of_range_id_in_one_table_is_flagged_and_reads_row_0(mot):
    bpt, Db, rows, norm = 8, 8, (458, 300), (True, False)
    tables, _ = bc.make_inputs(5200, rows, Db, bpt, 1, 1)
    tabs = tabs_on(tables, "fp32")
    ids = np.random.RandomState(5201).randint(0, 300, (2, 20 * bpt)).astype(np.int64)
    ids[1, 37] = 300                                                # == rows of table 1, inside table 0
    outs = mot.byte_cat(tabs, bpt=bpt, norm=norm, ids=dev(ids))
    torch.cuda.synchronize()
    with pytest.raises(IndexError, match="byte id"):
        mot.check_status()
    r = ref64(ids, tables[:1], norm[:1], [None], bpt)
    assert_close(host(outs[0]), r["out"][0])                         # table 0 holds the id
    ids0 = ids.copy()
    ids0[1, 37] = 0
    np.testing.assert_array_equal(host(outs[1]), f32(tables[1])[ids0].reshape(2, 20, bpt * Db))
    # the backward clamps and flags the same way
    g = [None, dev(f32(np.ones((2, 20, bpt * Db))))]
    d = mot.functional.byte_cat_backward(g, tabs, bpt=bpt, norm=norm, ids=dev(ids))
    torch.cuda.synchronize()
    with pytest.raises(IndexError, match="byte id"):
        mot.check_status()
    want = ref64(ids0, tables, norm, [None, np.ones((2, 20, bpt * Db))], bpt)["d_table"][1]
    assert rel(host(d[1]), want) < TOL


# ------------------------------------------------------------------------------------------------ gradients
@pytest.mark.parametrize("name,dt", FIXTURE)
def test_backward_fixture_cases(mot, golden, name, dt):
    Db, bpt, B, T, Vt, norm, std, seed = bc.CASES[name]
    pulled = golden[bc.key(name, "ids_pulled")].astype(np.int64)
    tables, gs = bc.case_tables(name)
    ref = ref64(pulled, tables, norm, gs, bpt)
    got = mot.functional.byte_cat_backward([dev(g, DTYPES[dt]) for g in gs], tabs_on(tables, dt), bpt=bpt, norm=norm, ids=dev(pulled))
    mot.check_status()
    check_grads(got, ref["d_table"], f"{name} {dt}")
    if std == 1.0:
        check_grads(got, [golden[bc.key(name, f"f64/d_table{j}")] for j in range(len(norm))], f"{name} {dt} fixture")
    # and loss.backward() through the autograd node, ids pulled in-kernel
    params = [t.requires_grad_(True) for t in tabs_on(tables, dt)]
    outs = mot.byte_cat(params, bpt=bpt, norm=norm, tokens=dev(golden[bc.key(name, "tokens")]), ttb=dev(bc.case_ttb(name)), pull="left")
    torch.autograd.backward(list(outs), [dev(g, DTYPES[dt]) for g in gs])
    mot.check_status()
    for j, p in enumerate(params):
        assert p.grad.dtype == DTYPES[dt]
        assert rel(host(p.grad.float()), ref["d_table"][j]) < (TOL if dt == "fp32" else 2.0 ** -8 + TOL)


GRAD_SHAPES = {
    # bpt, Db, rows, norm, B, T, how the ids are drawn
    "equal_ids": (16, 64, (458, 458), (True, False), 3, 200, "equal"),            # one row takes every add
    "big_table": (8, 8, (4096, 4096), (True, False), 3, 300, "uniform"),          # more rows than any LDS copy holds: the exact path
    "run5": (16, 64, (458, 458, 458, 458), (True, False, False, False), 2, 150, "uniform"),
    "b48": (16, 48, (458, 300), (True, True), 2, 100, "uniform"),                 # column slices of 24
}


def grad_inputs(case, scale=1.0):
    bpt, Db, rows, norm, B, T, how = GRAD_SHAPES[case]
    seed = 5300 + 7 * list(GRAD_SHAPES).index(case)
    tables, gs = bc.make_inputs(seed, rows, Db, bpt, B, T)
    rs = np.random.RandomState(seed + 1)
    ids = np.full((B, T * bpt), 7, dtype=np.int64) if how == "equal" else rs.randint(0, min(rows), (B, T * bpt)).astype(np.int64)
    return bpt, norm, tables, [g * scale for g in gs], ids       # a power-of-two scale keeps bf16 values bf16 values


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("case", list(GRAD_SHAPES))
def test_backward_vs_float64(mot, case, dt):
    bpt, norm, tables, gs, ids = grad_inputs(case)
    ref = ref64(ids, tables, norm, gs, bpt)
    got = mot.functional.byte_cat_backward([dev(g, DTYPES[dt]) for g in gs], tabs_on(tables, dt), bpt=bpt, norm=norm, ids=dev(ids))
    mot.check_status()
    check_grads(got, ref["d_table"], f"{case} {dt}")
    # two runs of the same backward: each within the bar of the exact gradient (the flushes of the workgroups are float atomics)
    again = mot.functional.byte_cat_backward([dev(g, DTYPES[dt]) for g in gs], tabs_on(tables, dt), bpt=bpt, norm=norm, ids=dev(ids))
    for a, b in zip(got, again):
        assert rel(host(a), host(b)) < TOL


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("scale", [2.0 ** 20, 2.0 ** -20])
def test_backward_scaled_upstream_gradients(mot, scale, dt):
    """the fixed-point scale follows the gradient's magnitude"""
    bpt, norm, tables, gs, ids = grad_inputs("run5", scale)
    ref = ref64(ids, tables, norm, gs, bpt)
    got = mot.functional.byte_cat_backward([dev(g, DTYPES[dt]) for g in gs], tabs_on(tables, dt), bpt=bpt, norm=norm, ids=dev(ids))
    mot.check_status()
    check_grads(got, ref["d_table"], f"scale {scale:g} {dt}")


@pytest.mark.parametrize("dt", list(DTYPES))
def test_backward_zero_gradient_gives_exact_zeros(mot, dt):
    bpt, norm, tables, gs, ids = grad_inputs("b48")
    got = mot.functional.byte_cat_backward([dev(np.zeros_like(g), DTYPES[dt]) for g in gs], tabs_on(tables, dt), bpt=bpt, norm=norm, ids=dev(ids))
    mot.check_status()
    for g in got:
        assert not g.any()


@pytest.mark.parametrize("dt", list(DTYPES))
def test_autograd_skips_unused_outputs_and_frozen_tables_and_accumulates(mot, dt):
    bpt, norm, tables, gs, ids = grad_inputs("run5")
    params = tabs_on(tables, dt)
    for j in (0, 1, 3):
        params[j].requires_grad_(True)                              # table 2 is frozen
    ups = [dev(g, DTYPES[dt]) for g in gs]
    bar = TOL if dt == "fp32" else 2.0 ** -8 + TOL

    def step():
        outs = mot.byte_cat(params, bpt=bpt, norm=norm, ids=dev(ids))
        torch.autograd.backward([outs[0], outs[3]], [ups[0], ups[3]])      # nothing depends on output 1

    step()
    mot.check_status()
    ref = ref64(ids, tables, norm, [gs[0], None, None, gs[3]], bpt)["d_table"]
    assert params[1].grad is None and params[2].grad is None
    for j in (0, 3):
        assert rel(host(params[j].grad.float()), ref[j]) < bar
    step()                                                          # a second backward accumulates into .grad
    for j in (0, 3):
        assert rel(host(params[j].grad.float()), 2 * ref[j]) < (bar if dt == "fp32" else 2 * 2.0 ** -8 + TOL)
    # the direct call: a None entry is skipped, `into` is accumulated into
    into = [torch.ones(params[0].shape, device=DEV), None, None, None]
    d = mot.functional.byte_cat_backward([ups[0], None, None, None], [p.detach() for p in params], bpt=bpt, norm=norm, ids=dev(ids), into=into)
    assert d[0] is into[0] and d[1] is None and d[2] is None and d[3] is None
    assert rel(host(d[0]) - 1.0, ref[0]) < TOL


# ------------------------------------------------------------------------------------------------ module
def test_bytes_front_end_forward_and_backward(mot):
    B, T, bpt, Db, V, value_rows = 2, 64, 16, 64, 458, 1000
    seed = 5400
    tables, gs = bc.make_inputs(seed, [V, value_rows, value_rows, value_rows], Db, bpt, B, T)
    ttb = gi.synth_ttb(seed + 1, 300, bpt, "left")
    toks = gi.fineweb_like_tokens(seed + 2, B, T, vocab=300, eot_p=0.02)
    pulled = orc.pull_from_left(orc.tokens_to_bytes(toks, ttb.astype(np.float32)), bpt, gi.PAD, gi.EOT)
    fe = mot.BytesFrontEnd(V, Db, bytes_per_token=bpt, n_value_embeds=3, value_rows=value_rows, ttb=torch.from_numpy(ttb)).to(DEV)
    with torch.no_grad():
        fe.embed_bytes.weight.copy_(dev(f32(tables[0])))
        for e, t in zip(fe.value_embeds_bytes, tables[1:]):
            e.weight.copy_(dev(f32(t)))
    norm = (True, False, False, False)
    ref = ref64(pulled, [tables[0]] + [t[:V] for t in tables[1:]], norm, gs, bpt)
    for byte_inputs in (dev(pulled.astype(np.int64)), None):
        fe.zero_grad(set_to_none=True)
        x0, ve = fe(dev(toks), byte_inputs)
        assert len(ve) == 3
        check_forward([x0] + ve, pulled, [tables[0]] + [t[:V] for t in tables[1:]], norm, ref["out"], "fp32", "BytesFrontEnd")
        torch.autograd.backward([x0] + ve, [dev(f32(g)) for g in gs])
        mot.check_status()
        assert rel(host(fe.embed_bytes.weight.grad), ref["d_table"][0]) < TOL
        for j, e in enumerate(fe.value_embeds_bytes):
            assert tuple(e.weight.grad.shape) == (value_rows, Db)
            assert rel(host(e.weight.grad[:V]), ref["d_table"][1 + j]) < TOL
            assert not e.weight.grad[V:].any()                      # rows no byte id names: exactly zero
    none, ve_only = fe(byte_inputs=dev(pulled.astype(np.int64)), x0=False)       # runs 2 and 8: the value embeddings alone
    assert none is None and all(torch.equal(a, b) for a, b in zip(ve_only, ve))
    x_only, empty = mot.BytesFrontEnd(V, Db, bytes_per_token=bpt).to(DEV)(byte_inputs=dev(pulled[0].astype(np.int64)))   # runs 4 and 6, one sequence
    assert empty == [] and tuple(x_only.shape) == (1, T, bpt * Db)


# ------------------------------------------------------------------------------------------------ hipGraph
@pytest.mark.parametrize("dt", list(DTYPES))
def test_forward_and_backward_replay_from_a_hip_graph(mot, dt):
    """No memset or memcpy node, no allocation by the library, no sync: after an eager warm-up capture forward + backward through
    the autograd node, copy a new batch into the token buffer, replay, compare with an eager run on the new batch."""
    bpt, Db, Vt, B, T, seed = 16, 64, 300, 2, 96, 5500
    norm = (True, False, False, False)
    tables, gs = bc.make_inputs(seed, [458] * 4, Db, bpt, B, T)
    ttb = dev(gi.synth_ttb(seed + 1, Vt, bpt, "left"))
    toks = dev(gi.fineweb_like_tokens(seed + 2, B, T, vocab=Vt, eot_p=0.02))
    params = [t.requires_grad_(True) for t in tabs_on(tables, dt)]
    ups = [dev(g, DTYPES[dt]) for g in gs]

    def step():
        outs = mot.byte_cat(params, bpt=bpt, norm=norm, tokens=toks, ttb=ttb, pull="left")
        torch.autograd.backward(list(outs), ups)
        return outs

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                                      # warm-up on the capture stream: allocates the workspace
        for p in params:
            p.grad = None
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        outs = step()
    toks.copy_(dev(gi.fineweb_like_tokens(seed + 3, B, T, vocab=Vt, eot_p=0.02)))      # a new batch, the same buffer
    graph.replay()
    torch.cuda.synchronize()
    fresh = [p.detach().clone().requires_grad_(True) for p in params]
    want = mot.byte_cat(fresh, bpt=bpt, norm=norm, tokens=toks, ttb=ttb, pull="left")
    torch.autograd.backward(list(want), ups)
    mot.check_status()
    for a, b in zip(outs, want):
        assert torch.equal(a, b)
    for p, q in zip(params, fresh):
        assert q.grad.abs().max() > 0
        a, b = host(p.grad.float()).astype(np.float64), host(q.grad.float()).astype(np.float64)
        print(f"{dt} replayed against eager .grad: {float(rel(a, b)):.3e}")
        if dt == "fp32":
            assert rel(a, b) < TOL
        else:   # one bf16 step of the element (2^-7 of it at most) on top of the bar for the fp32 sums
            assert (np.abs(a - b) <= 2.0 ** -7 * np.abs(b) + TOL * np.abs(b).max()).all()


# ------------------------------------------------------------------------------------------------ refusals
def test_functional_refusals(mot):
    ids = torch.zeros((1, 64), dtype=torch.int64, device=DEV)
    z = lambda r, c, dt=torch.float32: torch.zeros(r, c, device=DEV, dtype=dt)
    with pytest.raises(NotImplementedError, match="byte_dim 6"):
        mot.byte_cat([z(458, 6)], bpt=16, norm=(True,), ids=ids)
    with pytest.raises(NotImplementedError, match="multiple of 8"):
        mot.byte_cat([z(458, 4, torch.bfloat16)], bpt=16, norm=(True,), ids=ids)
    with pytest.raises(NotImplementedError, match="model_dim 4096"):
        mot.byte_cat([z(458, 256)], bpt=16, norm=(True,), ids=ids)
    with pytest.raises(ValueError, match="5 tables"):
        mot.byte_cat([z(458, 4)] * 5, bpt=16, norm=(False,) * 5, ids=ids)
    with pytest.raises(TypeError, match="share one dtype"):
        mot.byte_cat([z(458, 8), z(458, 8, torch.bfloat16)], bpt=8, norm=(True, False), ids=ids)
    (x,) = mot.byte_cat([z(458, 4)], bpt=16, norm=(True,), ids=ids)
    assert x.shape == (1, 4, 64) and not x.any()
