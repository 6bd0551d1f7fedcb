"""CPU checks of the compacted plain head (mot_plain_head_compact_*, functional.plain_head_loss / plain_head_eval with max_kept,
functional.window_kept_bound): the C ABI's new struct and symbols, every refusal before any HIP call, the workspace query's order
and clipping, window_kept_bound against window_targets, and the Python argument errors (no GPU needed)."""
import ctypes as C

import numpy as np
import pytest
import torch

import mixture_of_tokenizers_amd as mot
import plain_head_ref as pr
from mixture_of_tokenizers_amd import _capi as capi
from mixture_of_tokenizers_amd.modules import PlainLMHead
from test_plain_head_capi import REFUSALS, _desc, _err, _out

NAMES = ("mot_plain_head_compact_size", "mot_plain_head_compact_workspace_bytes", "mot_plain_head_compact_fwd", "mot_plain_head_compact_eval")
FWD, EVAL = "mot_plain_head_compact_fwd: ", "mot_plain_head_compact_eval: "


def _compact(max_kept=4096, **kw):
    c = capi.MotPlainHeadCompact()
    c.struct_size, c.reserved, c.max_kept = C.sizeof(capi.MotPlainHeadCompact), 0, max_kept
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _ws(d, c):
    return capi.lib.mot_plain_head_compact_workspace_bytes(C.byref(d), None if c is None else C.byref(c))


def test_surface():
    assert capi.lib.mot_plain_head_compact_size() == C.sizeof(capi.MotPlainHeadCompact) == 16
    for name in NAMES:
        assert name in capi.EXPORTS and hasattr(capi.lib, name), name
    assert capi.ABI_VERSION == 13 == capi.lib.mot_version()   # new symbols only
    assert capi.lib.mot_plain_head_desc_size() == C.sizeof(capi.MotPlainHeadDesc) == 120   # the descriptor's layout is as it was
    assert capi.STATUS_KEPT_OVERFLOW == 8
    assert mot.window_kept_bound is mot.functional.window_kept_bound and "window_kept_bound" in mot.__all__


@pytest.mark.parametrize("kw, want, msg", REFUSALS)
def test_descriptor_refusals_are_those_of_the_plain_call(kw, want, msg):
    d, c = _desc(**kw), _compact()
    assert capi.lib.mot_plain_head_compact_fwd(C.byref(d), C.byref(c), None) == want
    assert _err().startswith(FWD) and msg in _err(), _err()
    assert capi.lib.mot_plain_head_compact_eval(C.byref(d), C.byref(c), C.byref(_out()), None) == want
    assert _err().startswith(EVAL) and msg in _err(), _err()
    assert _ws(d, c) == 0


COMPACT_REFUSALS = [
    (None, capi.MOT_EINVAL, "null compact struct"),
    (dict(struct_size=8), capi.MOT_EINVAL, "compact struct_size 8"),
    (dict(reserved=1), capi.MOT_EINVAL, "reserved 1 must be 0"),
    (dict(max_kept=0), capi.MOT_ESHAPE, "max_kept 0 must be positive"),
    (dict(max_kept=-5), capi.MOT_ESHAPE, "max_kept -5 must be positive"),
]


@pytest.mark.parametrize("kw, want, msg", COMPACT_REFUSALS)
def test_compact_struct_refusals(kw, want, msg):
    d = _desc()
    c = None if kw is None else _compact(**kw)
    cp = None if c is None else C.byref(c)
    assert capi.lib.mot_plain_head_compact_fwd(C.byref(d), cp, None) == want
    assert _err().startswith(FWD) and msg in _err(), _err()
    assert capi.lib.mot_plain_head_compact_eval(C.byref(d), cp, C.byref(_out()), None) == want
    assert _err().startswith(EVAL) and msg in _err(), _err()
    assert _ws(d, c) == 0


def test_null_pointers_workspace_and_the_evaluation_refusals():
    c = _compact(256)
    assert capi.lib.mot_plain_head_compact_fwd(None, C.byref(c), None) == capi.MOT_EINVAL and _err().startswith(FWD + "null descriptor")
    assert capi.lib.mot_plain_head_compact_workspace_bytes(None, C.byref(c)) == 0
    d = _desc()
    need = _ws(d, c)
    assert need > 0
    assert capi.lib.mot_plain_head_compact_fwd(C.byref(d), C.byref(c), None) == capi.MOT_EINVAL and "null x" in _err()
    d.x = d.weight = d.targets = d.loss = 256   # never dereferenced: the workspace check fails first
    assert capi.lib.mot_plain_head_compact_fwd(C.byref(d), C.byref(c), None) == capi.MOT_EWORKSPACE and str(need) in _err()
    d.workspace, d.workspace_bytes = 256, need - 1
    assert capi.lib.mot_plain_head_compact_fwd(C.byref(d), C.byref(c), None) == capi.MOT_EWORKSPACE and str(need) in _err()
    d.workspace, d.workspace_bytes = 264, need
    assert capi.lib.mot_plain_head_compact_fwd(C.byref(d), C.byref(c), None) == capi.MOT_EUNSUPPORTED and "16-byte aligned" in _err()
    fn = capi.lib.mot_plain_head_compact_eval
    assert fn(C.byref(d), C.byref(c), None, None) == capi.MOT_EINVAL and _err().startswith(EVAL + "null out struct")
    assert fn(C.byref(d), C.byref(c), C.byref(_out(reserved=1)), None) == capi.MOT_EINVAL and "reserved" in _err()
    assert fn(C.byref(d), C.byref(c), C.byref(_out(counts=256)), None) == capi.MOT_EINVAL and "counts needs pred" in _err()
    d.dx = 256
    assert fn(C.byref(d), C.byref(c), C.byref(_out()), None) == capi.MOT_EINVAL and "forms no gradients" in _err()
    d.dx, d.n_rows = None, 0
    assert capi.lib.mot_plain_head_compact_fwd(C.byref(d), C.byref(c), None) == capi.MOT_ESHAPE and "no rows" in _err()
    assert _ws(d, c) == 0


def test_workspace_follows_the_bound_and_clips_it():
    plain = lambda **kw: capi.lib.mot_plain_head_workspace_bytes(C.byref(_desc(**kw)))
    ws = lambda max_kept, **kw: _ws(_desc(**kw), _compact(max_kept))
    V, D, N = 50304, 768, 65536
    assert 0 < ws(256, dx=256) < ws(N, dx=256)
    assert ws(N, dx=256) >= plain(dx=256) and ws(N) >= plain()
    assert ws(10 ** 9, dx=256) == ws(N, dx=256) and ws(10 ** 9) == ws(N)   # max_kept above n_rows is clipped, not refused
    # the chunk rule runs over cap: 256 slots are one chunk of 256 rows of logits, the normed rows, u and the per-slot pieces
    assert 256 * V * 4 <= ws(256, dx=256) < 256 * (V + 2 * D) * 4 + (1 << 20)
    assert ws(256, chunk_rows=1024) == ws(256, chunk_rows=256) == ws(256)   # a given chunk is clipped to cap
    assert ws(4119) == ws(4119, chunk_rows=2560)                            # the library's choice at 50 304 x 768 in fp32
    assert ws(256, chunk_rows=128) < ws(256)
    assert ws(256, dtype=capi.BF16) < ws(256)
    assert ws(256, group_rows=1024, ignore_index=7) == ws(256)
    for b in (ws(256, dx=256), ws(4119, dx=256, dtype=capi.BF16), ws(N)):
        assert b % 256 == 0   # every piece of the carve starts on 256 bytes


def test_window_kept_bound_is_what_window_targets_keeps():
    rng = np.random.default_rng(77)
    for T in (1, 16, 37):
        for B in (1, 5, 64):
            r = rng.integers(-T, 2 * T + 1, (B, 2))   # empty, reversed and out-of-range windows among them
            r[0] = (0, T)
            if B > 1:
                r[1] = (T, 0)
            y = torch.from_numpy(rng.integers(0, 128, (B, T)))
            ranges = torch.from_numpy(r)
            want = int((mot.window_targets(y, ranges.clamp_min(0)) != -100).sum())
            # window_targets takes a negative start as it stands (no position lies below 0): the clip changes nothing it keeps
            assert int((mot.window_targets(y, ranges) != -100).sum()) == want
            for form in (ranges, ranges.int(), r.tolist(), [tuple(p) for p in r.tolist()]):
                got = mot.window_kept_bound(form, T)
                assert isinstance(got, int) and got == want, (T, B, got, want)
    assert mot.window_kept_bound([], 16) == 0 and mot.window_kept_bound([(3, 3), (9, 2)], 16) == 0
    _, _, y, idx = pr.case_inputs("math", 128)
    assert mot.window_kept_bound(idx, pr.T) == int((mot.window_targets(y, idx) != -100).sum())
    with pytest.raises(TypeError, match="window_kept_bound: ranges must be host data"):
        mot.window_kept_bound(torch.empty(0, 2, dtype=torch.int64, device="meta"), 16)


@pytest.mark.parametrize("bad", [0, -3, 2.0, "7", True])
def test_python_argument_errors_come_before_the_device_check(bad):
    x, w, y, _ = pr.case_inputs("math", 128)   # CPU tensors: a valid max_kept gets as far as the device check
    with pytest.raises(ValueError, match="plain_head_loss: max_kept"):
        mot.plain_head_loss(x, w, y, max_kept=bad)
    with pytest.raises(ValueError, match="plain_head_eval: max_kept"):
        mot.plain_head_eval(x, w, y, max_kept=bad)
    head = PlainLMHead(torch.nn.Linear(pr.DIM, 128, bias=False))
    with pytest.raises(ValueError, match="plain_head_loss: max_kept"):
        head.loss(x, y, max_kept=bad)
    with pytest.raises(ValueError, match="plain_head_eval: max_kept"):
        head.evaluate(x, y, group_rows=pr.T, max_kept=bad)


def test_valid_max_kept_reaches_the_device_check():
    x, w, y, _ = pr.case_inputs("math", 128)
    for mk in (1, 64, np.int64(9)):
        with pytest.raises(RuntimeError, match="HIP device only"):
            mot.plain_head_loss(x, w, y, max_kept=mk)
        with pytest.raises(RuntimeError, match="HIP device only"):
            mot.plain_head_eval(x, w, y, max_kept=mk)
    with pytest.raises(RuntimeError, match="HIP device only"):
        PlainLMHead(torch.nn.Linear(pr.DIM, 128, bias=False)).loss(x, y, max_kept=8)
