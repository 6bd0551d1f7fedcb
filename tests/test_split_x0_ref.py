"""The plain-torch restatement of run 71081's x0t / x0b / x (tests/split_x0_ref.py) against the reference's own float64, float32 and
bfloat16 runs in tests/golden/split_x0.npz (tools/gen_golden_split_x0.py): float64 outputs and gradients to 1e-12, the float32 and
bfloat16 outputs bit for bit."""
import numpy as np
import pytest
import torch

import golden_inputs as gi
import split_x0_ref as sx

GOLDEN = sx.load_golden()


@pytest.mark.parametrize("name", list(sx.CASES))
def test_restatement_reproduces_the_reference(name):
    D, Db, bpt, B, T, Vt, std, seed, absent = sx.CASES[name]
    toks, ids = GOLDEN[sx.key(name, "tokens")], GOLDEN[sx.key(name, "ids")]
    np.testing.assert_array_equal(toks, sx.case_tokens(name))
    assert ids.shape == (B, T * bpt) and ids.min() >= 0 and ids.max() < gi.BYTE_VOCAB
    inp = sx.case_inputs(name)
    assert (inp["g"]["x0b"] is None) == (absent == "x0b")
    r64 = sx.run(toks, ids, inp, bpt=bpt, dtype=torch.float64)           # eps None: the float64 epsilon, as the reference's run
    r32 = sx.run(toks, ids, inp, bpt=bpt, dtype=torch.float32)
    r16 = sx.run(toks, ids, inp, bpt=bpt, dtype=torch.bfloat16)
    r16e = sx.run(toks, ids, inp, bpt=bpt, dtype=torch.bfloat16, eps=sx.F32_EPS)
    for what in sx.QUANTITIES:
        ref = GOLDEN[sx.key(name, f"f64/{what}")]
        assert r64[what].shape == ref.shape, what
        err = sx.rel_err(r64[what], ref)
        print(f"{name} {what}: restatement vs reference float64 {err:.2e}")
        assert err <= 1e-12, (what, err)
    for what in sx.GRADS:
        assert 0 <= float(GOLDEN[sx.key(name, f"f32err/{what}")]) < (2e-5 if std == 1.0 else 2e-3)
        assert 0 < float(GOLDEN[sx.key(name, f"bf16err/{what}")]) < 2.0 ** -5
    for w in sx.OUTS:
        # the float32 and bfloat16 runs: the same torch operations on the same shapes in the same order, so the same bits
        np.testing.assert_array_equal(r32[w], GOLDEN[sx.key(name, f"f32/{w}")].astype(np.float64))
        ref16 = GOLDEN[sx.key(name, f"bf16/{w}")].astype(np.float64)
        np.testing.assert_array_equal(r16[w], ref16)
        # F.rms_norm(eps=None) on bfloat16 rows takes the float32 epsilon (its fp32 opmath type): what MotSplitX0Desc.eps <= 0 means
        np.testing.assert_array_equal(r16e[w], ref16)
    if std != 1.0:   # and with 2^-7 the small-magnitude rows are off by whole bfloat16 steps
        x16b = sx.run(toks, ids, inp, bpt=bpt, dtype=torch.bfloat16, eps=2.0 ** -7)["x0t"]
        ref16 = GOLDEN[sx.key(name, "bf16/x0t")].astype(np.float64)
        assert np.abs(x16b - ref16).max() > 2.0 ** -6 * np.abs(ref16).max()


def test_the_absent_gradient_is_zero_not_missing():
    """The case without a gradient into x0b equals the same case with a zero one (what a NULL grad_x0b means to the library)."""
    name = "d128_b8_bpt16"
    D, Db, bpt, B, T, Vt, std, seed, absent = sx.CASES[name]
    toks, ids = GOLDEN[sx.key(name, "tokens")], GOLDEN[sx.key(name, "ids")]
    inp = sx.case_inputs(name)
    z = dict(inp, g=dict(inp["g"], x0b=np.zeros((B, T, D))))
    a, b = sx.run(toks, ids, inp, bpt=bpt), sx.run(toks, ids, z, bpt=bpt)
    for what in sx.QUANTITIES:
        np.testing.assert_array_equal(a[what], b[what])


def test_fixture_covers_the_eot_positions_and_stays_small():
    name = "d64_b4_bpt16"
    D, Db, bpt, B, T, Vt, std, seed, absent = sx.CASES[name]
    toks = GOLDEN[sx.key(name, "tokens")]
    e = Vt - 1
    assert toks[0, 0] == e and toks[0, T // 2] == e and toks[B - 1, 3] == e and toks[B - 1, 4] == e
    padded = sx.case_ttb(name)[toks].reshape(B, T * bpt)
    assert (GOLDEN[sx.key(name, "ids")] != padded).any()      # the pull moved bytes
    assert [c[:5] for c in sx.CASES.values()] == [(64, 4, 16, 2, 24), (128, 8, 16, 2, 24), (96, 24, 4, 3, 20), (64, 8, 8, 2, 24), (64, 4, 16, 1, 1)]
    assert sx.CASES["d64_b8_bpt8_small"][6] == 0.02 and sum(c[8] == "x0b" for c in sx.CASES.values()) == 1
    assert sx.S_TOK != sx.S_BYTE and 0.5 not in (sx.S_TOK, sx.S_BYTE)
    assert sx.GOLDEN.stat().st_size < 1_000_000
    assert str(GOLDEN["torch_version"])
