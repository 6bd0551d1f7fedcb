"""CPU-side checks of the generation step (mot_next_token): the struct, every refusal with its code in the call and in the size query
(all of them come before any HIP call), the no-op, the float64 restatement of tests/next_token_ref.py against what the reference's
own statements computed (tests/golden/next_token.npz, written by tools/gen_golden_next_token.py), the restatement's tie rule, and the
refusal of CPU tensors."""
import ctypes as C
import math
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
from next_token_ref import next_token_ref, strictly_larger_mass  # noqa: E402

import mixture_of_tokenizers_amd as mot  # noqa: E402
from mixture_of_tokenizers_amd import _capi as capi  # noqa: E402

FAKE = 4096   # an aligned address that is never dereferenced: every refusal comes first


def desc(**kw):
    d = capi.MotNextTokenDesc()
    d.struct_size = C.sizeof(capi.MotNextTokenDesc)
    d.dtype, d.norm_in, d.greedy, d.n_rows, d.x_stride, d.model_dim, d.vocab = capi.F32, 0, 0, 2, 64, 64, 256
    d.eps, d.temperature, d.top_k, d.top_p, d.n_top, d.reserved = 0.0, 1.0, 0, 1.0, 0, 0
    d.x = d.weight = d.u = d.token = FAKE
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_struct_and_exports():
    assert capi.lib.mot_next_token_desc_size() == C.sizeof(capi.MotNextTokenDesc)
    header = (REPO / "include" / "mot.h").read_text()
    body = re.search(r"typedef struct MotNextTokenDesc \{(.*?)\} MotNextTokenDesc;", header, re.S).group(1)
    fields = re.findall(r"^\s*(?:const\s+)?\w+\s+\*?(\w+);", body, re.M)
    assert fields == [f[0] for f in capi.MotNextTokenDesc._fields_]
    for name in ("mot_next_token_desc_size", "mot_next_token_workspace_bytes", "mot_next_token"):
        assert name in capi.EXPORTS
    assert capi.ABI_VERSION == 13 and capi.lib.mot_version() == 13
    assert capi.STATUS_LOGIT_NONFINITE == 16 and "#define MOT_STATUS_LOGIT_NONFINITE 16u" in header
    assert mot.next_token is mot.functional.next_token and "next_token" in mot.__all__ and "NextToken" in mot.__all__


REFUSALS = [
    (dict(struct_size=8), capi.MOT_EINVAL, b"struct_size"),
    (dict(dtype=7), capi.MOT_EUNSUPPORTED, b"dtype"),
    (dict(vocab=200), capi.MOT_EUNSUPPORTED, b"vocab"),
    (dict(vocab=262144 + 128), capi.MOT_EUNSUPPORTED, b"vocab"),
    (dict(model_dim=24, x_stride=24), capi.MOT_EUNSUPPORTED, b"model_dim"),
    (dict(model_dim=2064, x_stride=2064), capi.MOT_EUNSUPPORTED, b"model_dim"),
    (dict(x_stride=66), capi.MOT_EUNSUPPORTED, b"x_stride"),                  # rows 8 bytes off a 16-byte boundary
    (dict(dtype=capi.BF16, x_stride=68), capi.MOT_EUNSUPPORTED, b"x_stride"),
    (dict(x=FAKE + 4), capi.MOT_EUNSUPPORTED, b"aligned"),
    (dict(weight=FAKE + 8), capi.MOT_EUNSUPPORTED, b"aligned"),
    (dict(logits=FAKE + 4), capi.MOT_EUNSUPPORTED, b"aligned"),
    (dict(temperature=0.0), capi.MOT_EINVAL, b"temperature"),
    (dict(temperature=-1.0), capi.MOT_EINVAL, b"temperature"),
    (dict(temperature=math.inf), capi.MOT_EINVAL, b"temperature"),
    (dict(temperature=math.nan), capi.MOT_EINVAL, b"temperature"),
    (dict(top_k=-1), capi.MOT_EINVAL, b"top_k"),
    (dict(top_p=0.0), capi.MOT_EINVAL, b"top_p"),
    (dict(top_p=-0.5), capi.MOT_EINVAL, b"top_p"),
    (dict(top_p=math.nan), capi.MOT_EINVAL, b"top_p"),
    (dict(n_top=-1), capi.MOT_EINVAL, b"n_top"),
    (dict(n_top=9), capi.MOT_EINVAL, b"n_top"),
    (dict(u=None), capi.MOT_EINVAL, b"null u"),
    (dict(x=None), capi.MOT_EINVAL, b"null x"),
    (dict(weight=None), capi.MOT_EINVAL, b"null x"),
    (dict(token=None), capi.MOT_EINVAL, b"null x"),
    (dict(reserved=1), capi.MOT_EINVAL, b"reserved"),
    (dict(n_rows=-1), capi.MOT_ESHAPE, b"n_rows"),
    (dict(x_stride=48), capi.MOT_ESHAPE, b"x_stride"),
]


@pytest.mark.parametrize("kw,code,word", REFUSALS, ids=[f"{i}-{'-'.join(k)}" for i, (k, _, _) in enumerate(REFUSALS)])
def test_refusals_come_before_any_hip_call(kw, code, word):
    d = desc(**kw)
    assert capi.lib.mot_next_token(C.byref(d), None) == code
    msg = capi.lib.mot_last_error()
    assert msg.startswith(b"mot_next_token:") and word in msg, msg
    assert capi.lib.mot_next_token_workspace_bytes(C.byref(d)) == 0


def test_null_descriptor_workspace_and_no_op():
    assert capi.lib.mot_next_token(None, None) == capi.MOT_EINVAL
    assert capi.lib.mot_next_token_workspace_bytes(None) == 0
    d = desc()
    need = capi.lib.mot_next_token_workspace_bytes(C.byref(d))
    assert need >= 2 * 256 * 4
    assert capi.lib.mot_next_token(C.byref(d), None) == capi.MOT_EWORKSPACE   # none given
    d.workspace, d.workspace_bytes = FAKE, need - 1
    assert capi.lib.mot_next_token(C.byref(d), None) == capi.MOT_EWORKSPACE
    assert capi.lib.mot_next_token_workspace_bytes(C.byref(desc(greedy=1, u=None))) == need   # greedy needs no u
    # bf16 logits take half the room; 17 rows and more carry the rows of x as the heads' product takes them
    assert capi.lib.mot_next_token_workspace_bytes(C.byref(desc(dtype=capi.BF16))) < need
    assert capi.lib.mot_next_token_workspace_bytes(C.byref(desc(n_rows=17))) > 17 * 256 * 4
    # no rows: a no-op that touches nothing, after the same checks
    d0 = desc(n_rows=0)
    assert capi.lib.mot_next_token_workspace_bytes(C.byref(d0)) == 0
    assert capi.lib.mot_next_token(C.byref(d0), None) == capi.MOT_OK
    assert capi.lib.mot_next_token(C.byref(desc(n_rows=0, top_k=-1)), None) == capi.MOT_EINVAL


def test_restatement_reproduces_the_reference_on_the_fixture():
    g = np.load(REPO / "tests" / "golden" / "next_token.npz")
    logits = torch.from_numpy(g["logits"])
    assert logits.shape == (3, 256) and len(g["configs"]) == 24
    assert all(torch.unique(row).numel() == 256 for row in logits)
    for (t, k, p), probs in zip(g["configs"], g["probs"]):
        probs = torch.from_numpy(probs)
        r = next_token_ref(logits, temperature=float(t), top_k=int(k), top_p=float(p), greedy=True)
        assert torch.equal(probs > 0, r.keep), (t, k, p)                        # the same support
        assert float((probs - r.probs).abs().max()) <= 1e-12, (t, k, p)
        assert torch.equal(r.kept, r.keep.sum(1))
    assert 0 < float(g["err32"].max()) < 1e-5   # the reference's own float32 run, for scale


def test_restatement_tie_rule():
    # masses 1, e^-1 (three times), e^-2, e^-3, then nothing: Z = 2.2888
    row = torch.tensor([[2.0, 1.0, 1.0, 1.0, 0.0, -1.0] + [-60.0] * 122])
    g = strictly_larger_mass(row.double(), torch.exp(row.double() - 2.0))
    assert torch.equal(g[0, 1:4], g[0, 1:2].expand(3)) and float(g[0, 0]) == 0.0 and abs(float(g[0, 1]) - 1.0) < 1e-15
    # top-p 0.6: the mass above the tie group is 0.437 <= 0.6, so the WHOLE group stays although its second member crosses 0.6
    r = next_token_ref(row, top_p=0.6, greedy=True)
    assert r.keep[0, :6].tolist() == [True, True, True, True, False, False] and int(r.kept) == 4 and int(r.token) == 0
    # top-p 0.4: the group's strictly larger mass exceeds it: only the maximum stays
    assert int(next_token_ref(row, top_p=0.4, greedy=True).kept) == 1
    # top-k 2 lands inside the group: ties with the k-th value all stay
    r = next_token_ref(row, top_k=2, u=torch.tensor([0.99]), n_top=5)
    assert int(r.kept) == 4 and int(r.token) == 3 and r.top_cls.tolist() == [[0, 1, 2, 3, -1]] and float(r.top_prob[0, 4]) == 0.0
    # u = 0 takes the first kept class, u = 1 is clamped and takes the last; NaN counts as 0
    assert next_token_ref(row, top_k=2, u=torch.tensor([0.0])).token.tolist() == [0]
    assert next_token_ref(row, top_k=2, u=torch.tensor([1.0])).token.tolist() == [3]
    assert next_token_ref(row, top_k=2, u=torch.tensor([math.nan])).token.tolist() == [0]
    # a row of equal logits: everything stays, greedy returns class 0; -0 ties with +0
    r = next_token_ref(torch.zeros(1, 128) * torch.tensor([-1.0, 1.0]).repeat(64), top_k=5, top_p=0.3, greedy=True)
    assert int(r.kept) == 128 and int(r.token) == 0
    # NaN and +inf rows
    bad = torch.zeros(3, 128)
    bad[0, 5], bad[2, 7] = math.nan, math.inf
    r = next_token_ref(bad, greedy=True, n_top=2)
    assert r.token.tolist() == [-1, 0, -1] and r.kept.tolist() == [0, 128, 0] and math.isnan(float(r.prob[0])) and r.top_cls[0].tolist() == [-1, -1]


def test_cpu_tensors_are_refused():
    x, w = torch.zeros(2, 64), torch.zeros(256, 64)
    with pytest.raises(RuntimeError, match="HIP device only"):
        mot.next_token(x, w, greedy=True)
    with pytest.raises(RuntimeError, match="HIP device only"):
        mot.PlainLMHead(torch.nn.Linear(64, 256, bias=False), norm_in=False).next_token(x[None], greedy=True)
    with pytest.raises(TypeError):
        mot.next_token(x.half(), w, greedy=True)
    with pytest.raises(ValueError):
        mot.next_token(x, torch.zeros(256, 32), greedy=True)
