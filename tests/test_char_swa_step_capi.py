"""CPU-side checks of the character mixer's decode step (mot_char_swa_step): the struct against include/mot.h, every refusal with
its code in the call and in the size query (all of them come before any HIP call), the workspace bound that shows no weight or table
copy is made per step, CharTokenizer.token_char_table against a literal restatement of inference/inference.py:79-96, and the ring /
pos restatement of tests/char_swa_step_ref.py against the float64 oracle and functional.char_swa_state."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
from char_swa_step_ref import RingRef, case  # noqa: E402

import mixture_of_tokenizers_amd as mot  # noqa: E402
from mixture_of_tokenizers_amd import _capi as capi  # noqa: E402
from mixture_of_tokenizers_amd.data_creation import CharTokenizer  # noqa: E402
from oracle import oracle as orc  # noqa: E402

FAKE = 4096   # an aligned address that is never dereferenced: every refusal comes first
PTRS = ("tokens", "tok_chars", "tok_table", "char_table", "attn_norm_w", "wq", "wo", "kv_tables", "ring", "pos", "out")


def desc(**kw):
    d = capi.MotCharSwaStepDesc()
    d.struct_size = C.sizeof(capi.MotCharSwaStepDesc)
    d.dtype, d.n_rows, d.c_v, d.window, d.n_heads, d.head_dim, d.dim, d.version, d.char_rows = capi.F32, 2, 8, 8, 4, 64, 256, capi.SWA_TWO_RESIDUAL, 132
    d.tok_rows, d.norm_eps = 700, 1e-5
    for p in PTRS:
        setattr(d, p, FAKE)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_struct_and_exports():
    assert capi.lib.mot_char_swa_step_desc_size() == C.sizeof(capi.MotCharSwaStepDesc)
    header = (REPO / "include" / "mot.h").read_text()
    body = re.search(r"typedef struct MotCharSwaStepDesc \{(.*?)\} MotCharSwaStepDesc;", header, re.S).group(1)
    fields = re.findall(r"^\s*(?:const\s+)?\w+\s+\*?(\w+);", body, re.M)
    assert fields == [f[0] for f in capi.MotCharSwaStepDesc._fields_]
    for name in ("mot_char_swa_step_desc_size", "mot_char_swa_step_workspace_bytes", "mot_char_swa_step"):
        assert name in capi.EXPORTS
    assert capi.ABI_VERSION == 13 and capi.lib.mot_version() == 13        # new symbols only
    for name in ("char_swa_step", "char_swa_state", "CharSwaState"):
        assert getattr(mot, name) is getattr(mot.functional, name) and name in mot.__all__
    for name in ("set_token_chars", "decode_state", "step"):
        assert callable(getattr(mot.modules.CharMixerFrontEnd, name))


REFUSALS = [
    (dict(struct_size=8), capi.MOT_EINVAL, b"struct_size"),
    (dict(dtype=7), capi.MOT_EINVAL, b"dtype"),
    (dict(reserved0=1), capi.MOT_EINVAL, b"reserved"),
    (dict(reserved1=1), capi.MOT_EINVAL, b"reserved"),
    (dict(n_rows=17), capi.MOT_EUNSUPPORTED, b"mot_char_swa_fwd"),
    (dict(n_rows=-1), capi.MOT_ESHAPE, b"n_rows"),
    (dict(head_dim=32), capi.MOT_EUNSUPPORTED, b"head_dim"),
    (dict(head_dim=256), capi.MOT_EUNSUPPORTED, b"head_dim"),
    (dict(window=9), capi.MOT_EUNSUPPORTED, b"keys per query"),         # 9 x 8 = 72 keys
    (dict(c_v=0), capi.MOT_EUNSUPPORTED, b"keys per query"),
    (dict(dim=258), capi.MOT_ESHAPE, b"dim"),
    (dict(dtype=capi.BF16, dim=260), capi.MOT_EUNSUPPORTED, b"multiple of 8"),
    (dict(version=3), capi.MOT_EINVAL, b"version"),
    (dict(n_rows=16, dim=4096), capi.MOT_EUNSUPPORTED, b"LDS"),         # 16 x 4096 fp32 rows: 256 KiB
    (dict(kv_tables=None), capi.MOT_EINVAL, b"kv_tables"),
    (dict(char_ids_new=FAKE), capi.MOT_EINVAL, b"exactly one"),          # both sources
    (dict(tok_chars=None), capi.MOT_EINVAL, b"exactly one"),             # neither
    (dict(wq=FAKE + 4), capi.MOT_EUNSUPPORTED, b"aligned"),
] + [(dict([(p, None)]), capi.MOT_EINVAL, b"non-null") for p in PTRS if p not in ("tok_chars", "kv_tables")]


@pytest.mark.parametrize("kw,code,word", REFUSALS, ids=[f"{i}-{'-'.join(k)}" for i, (k, _, _) in enumerate(REFUSALS)])
def test_refusals_come_before_any_hip_call(kw, code, word):
    d = desc(**kw)
    assert capi.lib.mot_char_swa_step(C.byref(d), None) == code
    msg = capi.lib.mot_last_error()
    assert msg.startswith(b"mot_char_swa_step:") and word in msg, msg
    assert capi.lib.mot_char_swa_step_workspace_bytes(C.byref(d)) == 0


def test_null_descriptor_workspace_bound_and_no_op():
    assert capi.lib.mot_char_swa_step(None, None) == capi.MOT_EINVAL
    assert capi.lib.mot_char_swa_step_workspace_bytes(None) == 0
    # the bound of the issue: n_rows * (dim + 2 * hdim) * 4 bytes plus alignment -- no room for a copy of a weight or a table
    for dt in (capi.F32, capi.BF16):
        for n, dim, H, hd in ((1, 2048, 32, 64), (8, 2048, 32, 64), (16, 2048, 32, 64), (3, 256, 4, 64), (16, 512, 4, 128), (5, 128, 8, 128)):
            d = desc(dtype=dt, n_rows=n, dim=dim, n_heads=H, head_dim=hd)
            need = capi.lib.mot_char_swa_step_workspace_bytes(C.byref(d))
            assert 0 < need <= n * (dim + 2 * H * hd) * 4 + 2 * 256, (dt, n, dim, H, hd, need)
            assert need < H * hd * dim * 2                                   # smaller than one bf16 copy of wq
    d = desc()
    need = capi.lib.mot_char_swa_step_workspace_bytes(C.byref(d))
    assert capi.lib.mot_char_swa_step(C.byref(d), None) == capi.MOT_EWORKSPACE   # none given
    d.workspace, d.workspace_bytes = FAKE, need - 1
    assert capi.lib.mot_char_swa_step(C.byref(d), None) == capi.MOT_EWORKSPACE
    # char_ids_new instead of the table is the same call
    assert capi.lib.mot_char_swa_step_workspace_bytes(C.byref(desc(tok_chars=None, char_ids_new=FAKE))) == need
    # no rows: a no-op that touches nothing, after the same checks
    d0 = desc(n_rows=0)
    assert capi.lib.mot_char_swa_step_workspace_bytes(C.byref(d0)) == 0
    assert capi.lib.mot_char_swa_step(C.byref(d0), None) == capi.MOT_OK
    assert capi.lib.mot_char_swa_step(C.byref(desc(n_rows=0, head_dim=32)), None) == capi.MOT_EUNSUPPORTED


# ---------------------------------------------------------------------------------------------- token -> character rows
class _ReferenceRows:
    """inference/inference.py:56-67 and 79-96, restated literally (the tokenizer's three constants as attributes)."""

    def __init__(self, max_char, leading_space_ind, bos, eos):
        self.max_char, self.leading_space_ind, self.bos, self.eos = max_char, leading_space_ind, bos, eos

    def chr_tokenize(self, x):
        ind = ord(x)
        if ind <= 127:
            return ind
        if ind == self.leading_space_ind:
            return 128
        if ind == self.bos:
            return 129
        if ind == self.eos:
            return 130
        else:
            return 131

    def create_char_matrix(self, char_tokens, seq_len):
        mat = torch.zeros(seq_len, self.max_char) + 2
        for row, sublist in enumerate(char_tokens):
            if row >= seq_len:
                break
            ind = 0
            for char in sublist:
                if ind >= self.max_char:
                    break
                mat[row][ind] = char
                ind += 1
            if ind < self.max_char:
                mat[row][ind] = 130
        return mat


@pytest.mark.parametrize("max_char", [8, 3])
def test_token_char_table_is_create_char_matrix_per_token(max_char):
    ct = CharTokenizer(num_char_positions=max_char)
    ref = _ReferenceRows(max_char, ct.leading_space_ind, ct.bos_token_id, ct.eos_token_id)
    sp, bos, eos = chr(ct.leading_space_ind), chr(ct.bos_token_id), chr(ct.eos_token_id)
    strings = ["", "a", "sevench", "eightchr", "ninechars", sp + "there", sp, "naïve", "中文", bos, eos, bos + "x" + eos,
               sp + "é" * 9, "\x00\x7f", None, "1234567" + sp, "12345678" + eos]
    assert [len(s) for s in strings[:5]] == [0, 1, 7, 8, 9]
    tab = ct.token_char_table(strings)
    assert tab.dtype == torch.int32 and tab.shape == (len(strings), max_char) and tab.device.type == "cpu"
    for v, s in enumerate(strings):
        want = ref.create_char_matrix([[ref.chr_tokenize(c) for c in (s or "")]], seq_len=1).long()[0]
        assert torch.equal(tab[v].long(), want), (s, tab[v], want)
    assert tab[0].tolist() == [130] + [2] * (max_char - 1) and tab[14].tolist() == tab[0].tolist()      # empty and None
    if max_char == 8:
        assert tab[3].tolist() == [ord(c) for c in "eightchr"]              # eight characters: no room for 130
        assert tab[4].tolist() == [ord(c) for c in "ninechar"]              # truncated
        assert tab[5].tolist() == [128] + [ord(c) for c in "there"] + [130, 2]
        assert tab[9].tolist() == [129, 130] + [2] * 6 and tab[10].tolist() == [130, 130] + [2] * 6
        assert tab[7].tolist() == [ord("n"), ord("a"), 131, ord("v"), ord("e"), 130, 2, 2]


# ---------------------------------------------------------------------------------------------- the ring restatement
@pytest.mark.parametrize("c_v,window", [(8, 8), (5, 6)])
def test_ring_slice_gives_the_full_sequence_row(c_v, window):
    B, T, d, H, hd = 2, 21, 64, 2, 64
    c = case(51 + c_v, B, T, c_v, d, H, hd, 90, 132)
    kw = dict(n_heads=H, head_dim=hd, window=window, norm_eps=1e-5, version="two_residual", lambda_tok=0.8, lambda_char=1.3)
    args = lambda toks, cid: (toks, cid, c["Et"], c["Ec"], c["wa"], c["wc"], c["wq"], c["wk"], c["wv"], c["wo"])
    full = orc.char_swa(*args(c["toks"], c["cid"]), **kw)
    scale = np.abs(full).max()
    ring = RingRef(B, window, c_v)
    for t in range(T):
        for b, (lo, cid) in enumerate(ring.step(c["cid"][:, t])):
            assert lo == max(0, t - window + 1) and cid.shape == (t - lo + 1, c_v) and np.array_equal(cid, c["cid"][b, lo:t + 1])
            row = orc.char_swa(*args(c["toks"][b:b + 1, lo:t + 1], cid[None]), **kw)[0, -1]
            assert np.abs(row - full[b, t]).max() <= 1e-12 * scale, (b, t)
    # the state after T steps is the state of the whole character matrix as a prompt
    st = mot.char_swa_state(torch.from_numpy(c["cid"]), window=window, c_v=c_v)
    assert st.ring.dtype == torch.int32 and st.pos.dtype == torch.int64
    assert np.array_equal(st.ring.numpy(), ring.ring) and np.array_equal(st.pos.numpy(), ring.pos) and ring.pos.tolist() == [T] * B
    # a prompt shorter than the window leaves the untouched slots at 0; no prompt: the empty state
    st3 = mot.char_swa_state(torch.from_numpy(c["cid"][:, :3]), window=window, c_v=c_v)
    short = RingRef(B, window, c_v)
    for t in range(3):
        short.step(c["cid"][:, t])
    assert np.array_equal(st3.ring.numpy(), short.ring) and st3.pos.tolist() == [3] * B
    e = mot.char_swa_state(None, n_rows=B, window=window, c_v=c_v)
    assert e.ring.shape == (B, window, c_v) and not e.ring.any() and e.pos.tolist() == [0] * B


def test_cpu_tensors_are_refused():
    st = mot.char_swa_state(None, n_rows=1, window=8, c_v=8)
    z = torch.zeros
    with pytest.raises(RuntimeError, match="HIP device only"):
        mot.char_swa_step(z(1, dtype=torch.int64), st, z(10, 64), z(132, 64), tok_chars=z(10, 8, dtype=torch.int32), attn_norm_w=z(64),
                          char_norm_w=z(64), wq=z(64, 64), wk=z(64, 64), wv=z(64, 64), wo=z(64, 64), n_heads=1, head_dim=64, kv_cache={})
