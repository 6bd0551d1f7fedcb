"""CPU-side checks of the decode step's feed-forward (mot_ffn_step): the struct against include/mot.h, every refusal with its code
in the call and in the size query (all of them come before any HIP call), the workspace size that include/mot.h states, the exports,
and the float64 restatement of tests/ffn_step_ref.py against the eager mirror classes."""
import ctypes as C
import re
import sys
from pathlib import Path

import pytest
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
from ffn_step_ref import ffn_step_ref, reference_module  # noqa: E402

import mixture_of_tokenizers_amd as mot  # noqa: E402
from mixture_of_tokenizers_amd import _capi as capi  # noqa: E402

FAKE = 4096   # an aligned address that is never dereferenced: every refusal comes first
PTRS = ("h", "norm_w", "w1", "w3", "w2", "out")


def desc(**kw):
    d = capi.MotFfnStepDesc()
    d.struct_size = C.sizeof(capi.MotFfnStepDesc)
    d.dtype, d.n_rows, d.dim, d.inter, d.norm_eps = capi.F32, 2, 256, 512, 1e-5
    for p in PTRS:
        setattr(d, p, FAKE)
    d.out = FAKE + (1 << 20)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_struct_and_exports():
    assert capi.lib.mot_ffn_step_desc_size() == C.sizeof(capi.MotFfnStepDesc)
    header = (REPO / "include" / "mot.h").read_text()
    body = re.search(r"typedef struct MotFfnStepDesc \{(.*?)\} MotFfnStepDesc;", header, re.S).group(1)
    fields = re.findall(r"^\s*(?:const\s+)?\w+\s+\*?(\w+);", body, re.M)
    assert fields == [f[0] for f in capi.MotFfnStepDesc._fields_]
    for name in ("mot_ffn_step_desc_size", "mot_ffn_step_workspace_bytes", "mot_ffn_step"):
        assert name in capi.EXPORTS
    assert capi.ABI_VERSION == 13 and capi.lib.mot_version() == 13        # new symbols only
    assert mot.char_ffn_step is mot.functional.char_ffn_step and "char_ffn_step" in mot.__all__
    assert callable(mot.modules.TokenMixByCharBMMBlock.ffn_step)


REFUSALS = [
    (dict(struct_size=8), capi.MOT_EINVAL, b"struct_size"),
    (dict(dtype=7), capi.MOT_EINVAL, b"dtype"),
    (dict(reserved0=1), capi.MOT_EINVAL, b"reserved"),
    (dict(reserved1=1), capi.MOT_EINVAL, b"reserved"),
    (dict(reserved2=1), capi.MOT_EINVAL, b"reserved"),
    (dict(n_rows=17), capi.MOT_EUNSUPPORTED, b"FeedForward"),
    (dict(n_rows=0), capi.MOT_EUNSUPPORTED, b"FeedForward"),
    (dict(n_rows=-1), capi.MOT_EUNSUPPORTED, b"FeedForward"),
    (dict(dim=258), capi.MOT_ESHAPE, b"dim"),
    (dict(dim=0), capi.MOT_ESHAPE, b"dim"),
    (dict(inter=514), capi.MOT_ESHAPE, b"inter"),
    (dict(dtype=capi.BF16, dim=260), capi.MOT_EUNSUPPORTED, b"multiples of 8"),
    (dict(dtype=capi.BF16, inter=516), capi.MOT_EUNSUPPORTED, b"multiples of 8"),
    (dict(n_rows=16, dim=4096), capi.MOT_EUNSUPPORTED, b"LDS"),                      # 16 x 4096 fp32 rows: 256 KiB
    (dict(n_rows=9, dim=2052), capi.MOT_EUNSUPPORTED, b"LDS"),                       # staged as 16 rows
    (dict(dtype=capi.BF16, n_rows=16, dim=4104), capi.MOT_EUNSUPPORTED, b"LDS"),
    (dict(out=FAKE), capi.MOT_EINVAL, b"overlaps"),
    (dict(out=FAKE + 2 * 256 * 4 - 16), capi.MOT_EINVAL, b"overlaps"),              # the last 16 bytes of h
    (dict(h=FAKE + (1 << 20) + 16), capi.MOT_EINVAL, b"overlaps"),
] + [(dict([(p, None)]), capi.MOT_EINVAL, b"non-null") for p in PTRS] \
  + [(dict([(p, (FAKE if p != "out" else FAKE + (1 << 20)) + 4)]), capi.MOT_EUNSUPPORTED, b"aligned") for p in PTRS]


@pytest.mark.parametrize("kw,code,word", REFUSALS, ids=[f"{i}-{'-'.join(k)}" for i, (k, _, _) in enumerate(REFUSALS)])
def test_refusals_come_before_any_hip_call(kw, code, word):
    d = desc(**kw)
    assert capi.lib.mot_ffn_step(C.byref(d), None) == code
    msg = capi.lib.mot_last_error()
    assert msg.startswith(b"mot_ffn_step:") and word in msg, msg
    assert capi.lib.mot_ffn_step_workspace_bytes(C.byref(d)) == 0


def test_null_descriptor_and_the_workspace_of_the_header():
    assert capi.lib.mot_ffn_step(None, None) == capi.MOT_EINVAL
    assert capi.lib.mot_ffn_step_workspace_bytes(None) == 0
    al = lambda n: (n + 255) // 256 * 256
    for dt, e in ((capi.F32, 4), (capi.BF16, 2)):
        for n, dim, inter in ((1, 2048, 8192), (8, 2048, 8192), (16, 2048, 8192), (3, 256, 512), (5, 264, 1384), (16, 8, 1024), (2, 8, 1032)):
            need = capi.lib.mot_ffn_step_workspace_bytes(C.byref(desc(dtype=dt, n_rows=n, dim=dim, inter=inter)))
            assert need == al(n * inter * e) + al(-(-inter // 1024) * n * dim * 4), (dt, n, dim, inter, need)
            assert dim < 256 or need < inter * dim * 2                        # smaller than one bf16 copy of a weight
    # the edges that are still served: 128 KiB of staged rows exactly
    assert capi.lib.mot_ffn_step_workspace_bytes(C.byref(desc(n_rows=16, dim=2048, inter=8192))) > 0
    assert capi.lib.mot_ffn_step_workspace_bytes(C.byref(desc(dtype=capi.BF16, n_rows=16, dim=4096, inter=8192))) > 0
    assert capi.lib.mot_ffn_step_workspace_bytes(C.byref(desc(out=FAKE + 2 * 256 * 4))) > 0        # out right behind h
    d = desc()
    need = capi.lib.mot_ffn_step_workspace_bytes(C.byref(d))
    assert capi.lib.mot_ffn_step(C.byref(d), None) == capi.MOT_EWORKSPACE       # none given
    d.workspace, d.workspace_bytes = FAKE, need - 1
    assert capi.lib.mot_ffn_step(C.byref(d), None) == capi.MOT_EWORKSPACE
    assert capi.lib.mot_last_error().startswith(b"mot_ffn_step:")


def test_restatement_is_the_mirror_module_and_silu_stays_finite():
    m = reference_module(torch.float64, dim=64, inter=136, seed=3)
    nw, w1, w2, w3 = m.weights()
    h = torch.randn(5, 64, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    h[2] = 0
    ref = ffn_step_ref(h, nw, w1, w2, w3)
    assert torch.allclose(ref, m(h), rtol=1e-6, atol=1e-6) and not ref[2].any()      # (RMSNorm forms its quotient in fp32)
    big = ffn_step_ref(h, nw, w1 * 2000, w2, w3)                               # pre-activations far beyond +-120
    assert torch.isfinite(big).all()
    r16 = ffn_step_ref(h.bfloat16(), nw, w1.bfloat16(), w2.bfloat16(), w3.bfloat16(), round_bf16=True)
    assert torch.equal(r16, r16.bfloat16().double())                           # a bf16-valued result


def test_cpu_tensors_are_refused():
    z = torch.zeros
    with pytest.raises(RuntimeError, match="HIP device only"):
        mot.char_ffn_step(z(1, 64), z(64), z(128, 64), z(64, 128), z(128, 64), norm_eps=1e-5)
