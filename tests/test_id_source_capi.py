"""CPU checks of what the four descriptor front-ends with a byte-id source share (mot_byte_fc_mix_*, mot_byte_cat_*, mot_value_mix_*,
mot_splitx_*; csrc/mot_desc.hpp): ONE table of id-source and workspace faults, run over every front-end, forward and backward, with
fake pointers (the argument checks run before any HIP call, so no GPU is needed).  For each refusal the return code and the FULL
mot_last_error() text are compared with literals that were recorded from the library as it was before the checks were shared: the
front-ends keep their messages, their codes, the order of their checks and the differences between them (byte_cat's "tokens / ttb
missing", value_mix's single out_ids, the workspace size split_x0 reports for a null workspace)."""
import ctypes as C

import pytest

from mixture_of_tokenizers_amd import _capi as capi

PTR = 64   # never dereferenced: validation fails first
TTB = dict(id_source=capi.IDS_FROM_TTB, ids=None, ttb=PTR, ttb_rows=100, ttb_elem_bytes=2, pull_dir=capi.PULL_LEFT)


def _byte_fc():
    d = capi.MotByteFcMixDesc()
    d.tokens = d.tok_table = d.byte_table = d.byte_fc = d.out = d.out_row_rnorm = PTR
    d.tok_rows, d.tok_dim, d.model_dim, d.byte_rows, d.byte_dim, d.norm_out = 100, 1024, 1024, 458, 64, 1
    g = capi.MotByteFcMixGrads()
    g.grad_out = g.d_tok = g.d_byte = g.d_byte_fc = PTR
    return d, g


def _byte_cat():
    d = capi.MotByteCatDesc()
    d.tokens, d.byte_dim, d.n_out = PTR, 64, 4
    g = capi.MotByteCatGrads()
    for j in range(4):
        d.slot[j].table, d.slot[j].rows, d.slot[j].out, d.slot[j].norm, d.slot[j].dtype = PTR, 458, PTR, int(j == 0), capi.F32
        g.slot[j].grad_out = g.slot[j].d_table = PTR
    return d, g


def _value_mix():
    d = capi.MotValueMixDesc()
    d.tokens = PTR
    d.tok_rows, d.byte_rows, d.token_dim, d.byte_dim, d.out_dim, d.n_slots, d.norm_out = 100, 458, 1024, 64, 1024, 3, 1
    g = capi.MotValueMixGrads()
    for j in range(3):
        s, q = d.slot[j], g.slot[j]
        s.tok_table = s.byte_table = s.weight = s.out = s.out_row_rnorm = q.grad_out = q.d_tok = q.d_byte = q.d_weight = PTR
    return d, g


def _split_x0():
    d = capi.MotSplitX0Desc()
    d.tokens = d.tok_table = d.byte_table = d.scale_tok = d.scale_byte = d.out_x0t = d.out_x0b = d.out_x = PTR
    d.tok_rows, d.byte_rows, d.model_dim, d.byte_dim = 100, 458, 1024, 64
    g = capi.MotSplitX0Grads()
    g.grad_x0t = g.grad_x0b = g.grad_x = g.d_tok_table = g.d_byte_table = g.d_scale_tok = g.d_scale_byte = PTR
    return d, g


L = capi.lib
# front-end -> (descriptor and gradients of a valid call, forward, backward, size query of a direction)
FRONT_ENDS = {
    "byte_fc_mix": (_byte_fc, L.mot_byte_fc_mix_fwd, L.mot_byte_fc_mix_bwd,
                    lambda p, bwd: (L.mot_byte_fc_mix_bwd_workspace_bytes if bwd else L.mot_byte_fc_mix_workspace_bytes)(p)),
    "byte_cat": (_byte_cat, L.mot_byte_cat_fwd, L.mot_byte_cat_bwd,
                 lambda p, bwd: (L.mot_byte_cat_bwd_workspace_bytes if bwd else L.mot_byte_cat_workspace_bytes)(p)),
    "value_mix": (_value_mix, L.mot_value_mix_fwd, L.mot_value_mix_bwd, lambda p, bwd: L.mot_value_mix_workspace_bytes(p, int(bwd))),
    "split_x0": (_split_x0, L.mot_splitx_fwd, L.mot_splitx_bwd, lambda p, bwd: L.mot_splitx_workspace_bytes(p, int(bwd))),
}
# fault -> the fields it sets on the valid descriptor (ids given, an EMPTY batch: what passes the checks returns MOT_OK without a
# launch).  "out_ids*" name the id outputs, of which value_mix has one; "workspace_*" take a batch of 2 x 64 tokens and the size the
# library asks for, so they are the last check of a call.
FAULTS = {
    "bad_id_source": dict(id_source=7),
    "ttb_elem_bytes_3": dict(TTB, ttb_elem_bytes=3),
    "pull_dir_7": dict(TTB, pull_dir=7),
    "ttb_rows_0": dict(TTB, ttb_rows=0),
    "null_ttb": dict(TTB, ttb=None),
    "null_ids": dict(ids=None),
    "out_ids_padded_with_given_ids": dict(out_ids_padded=PTR),
    "out_ids_pulled_with_given_ids": dict(out_ids_pulled=PTR),
    "from_ttb_in_the_backward": dict(TTB),
    "bpt_0": dict(bpt=0),
    "bpt_above_max": dict(bpt=capi.MAX_BPT + 1),
    "workspace_null": "null",
    "workspace_too_small": "small",
    "workspace_misaligned": "misaligned",
}


def observe(front_end, fault, backward):
    """(return code, mot_last_error() text) of one call."""
    make, fwd, bwd, query = FRONT_ENDS[front_end]
    d, g = make()
    d.struct_size, g.struct_size = C.sizeof(d), C.sizeof(g)
    d.dtype, d.n_rows, d.tokens_per_row, d.bpt, d.id_source, d.ids = capi.F32, 0, 4, 16, capi.IDS_GIVEN, PTR
    fields = FAULTS[fault]
    if isinstance(fields, str):
        d.n_rows, d.tokens_per_row = 2, 64
        need = query(C.byref(d), backward)
        d.workspace, d.workspace_bytes = {"null": (None, need), "small": (PTR, need - 16), "misaligned": (PTR + 8, need)}[fields]
        fields = {}
    for k, v in fields.items():
        if front_end == "value_mix" and k.startswith("out_ids"):
            k = "out_ids"
        setattr(d, k, v)
    rc = bwd(C.byref(d), C.byref(g), None) if backward else fwd(C.byref(d), None)
    return rc, L.mot_last_error().decode()


# Recorded from the library before the front-ends shared these checks (the same table run against a build of that commit); a
# combination that build does not refuse is not listed.  (front-end, fault, backward) -> (code, text)
EXPECTED = {
    ('byte_fc_mix', 'bad_id_source', False): (-1, 'byte_fc_mix: bad id_source 7'),
    ('byte_fc_mix', 'bad_id_source', True): (-1, 'byte_fc_mix: bad id_source 7'),
    ('byte_fc_mix', 'ttb_elem_bytes_3', False): (-1, 'byte_fc_mix: ttb_elem_bytes must be 2 or 4'),
    ('byte_fc_mix', 'ttb_elem_bytes_3', True): (-1, 'byte_fc_mix: ttb_elem_bytes must be 2 or 4'),
    ('byte_fc_mix', 'pull_dir_7', False): (-1, 'byte_fc_mix: bad pull_dir 7'),
    ('byte_fc_mix', 'pull_dir_7', True): (-1, 'byte_fc_mix: bad pull_dir 7'),
    ('byte_fc_mix', 'ttb_rows_0', False): (-1, 'byte_fc_mix: ttb missing'),
    ('byte_fc_mix', 'ttb_rows_0', True): (-1, 'byte_fc_mix: ttb missing'),
    ('byte_fc_mix', 'null_ttb', False): (-1, 'byte_fc_mix: ttb missing'),
    ('byte_fc_mix', 'null_ttb', True): (-3, 'byte_fc_mix_bwd: pass the byte ids the forward used (MOT_IDS_GIVEN)'),
    ('byte_fc_mix', 'null_ids', False): (-1, 'byte_fc_mix: ids missing'),
    ('byte_fc_mix', 'null_ids', True): (-1, 'byte_fc_mix: ids missing'),
    ('byte_fc_mix', 'out_ids_padded_with_given_ids', False): (-1, 'byte_fc_mix: out_ids_* need MOT_IDS_FROM_TTB'),
    ('byte_fc_mix', 'out_ids_padded_with_given_ids', True): (-1, 'byte_fc_mix: out_ids_* need MOT_IDS_FROM_TTB'),
    ('byte_fc_mix', 'out_ids_pulled_with_given_ids', False): (-1, 'byte_fc_mix: out_ids_* need MOT_IDS_FROM_TTB'),
    ('byte_fc_mix', 'out_ids_pulled_with_given_ids', True): (-1, 'byte_fc_mix: out_ids_* need MOT_IDS_FROM_TTB'),
    ('byte_fc_mix', 'from_ttb_in_the_backward', True): (-3, 'byte_fc_mix_bwd: pass the byte ids the forward used (MOT_IDS_GIVEN)'),
    ('byte_fc_mix', 'bpt_0', False): (-3, 'byte_fc_mix: bytes_per_token 0 outside [1, 64]'),
    ('byte_fc_mix', 'bpt_0', True): (-3, 'byte_fc_mix: bytes_per_token 0 outside [1, 64]'),
    ('byte_fc_mix', 'bpt_above_max', False): (-3, 'byte_fc_mix: bytes_per_token 65 outside [1, 64]'),
    ('byte_fc_mix', 'bpt_above_max', True): (-3, 'byte_fc_mix: bytes_per_token 65 outside [1, 64]'),
    ('byte_fc_mix', 'workspace_null', False): (-5, 'byte_fc_mix: needs 524288 16-byte aligned workspace bytes, got 524288'),
    ('byte_fc_mix', 'workspace_null', True): (-5, 'byte_fc_mix_bwd: needs 1575424 16-byte aligned workspace bytes, got 1575424'),
    ('byte_fc_mix', 'workspace_too_small', False): (-5, 'byte_fc_mix: needs 524288 16-byte aligned workspace bytes, got 524272'),
    ('byte_fc_mix', 'workspace_too_small', True): (-5, 'byte_fc_mix_bwd: needs 1575424 16-byte aligned workspace bytes, got 1575408'),
    ('byte_fc_mix', 'workspace_misaligned', False): (-5, 'byte_fc_mix: needs 524288 16-byte aligned workspace bytes, got 524288'),
    ('byte_fc_mix', 'workspace_misaligned', True): (-5, 'byte_fc_mix_bwd: needs 1575424 16-byte aligned workspace bytes, got 1575424'),
    ('byte_cat', 'bad_id_source', False): (-1, 'byte_cat: bad id_source 7'),
    ('byte_cat', 'bad_id_source', True): (-1, 'byte_cat: bad id_source 7'),
    ('byte_cat', 'ttb_elem_bytes_3', False): (-1, 'byte_cat: ttb_elem_bytes must be 2 or 4'),
    ('byte_cat', 'ttb_elem_bytes_3', True): (-1, 'byte_cat: ttb_elem_bytes must be 2 or 4'),
    ('byte_cat', 'pull_dir_7', False): (-1, 'byte_cat: bad pull_dir 7'),
    ('byte_cat', 'pull_dir_7', True): (-1, 'byte_cat: bad pull_dir 7'),
    ('byte_cat', 'ttb_rows_0', False): (-1, 'byte_cat: ttb missing'),
    ('byte_cat', 'ttb_rows_0', True): (-1, 'byte_cat: ttb missing'),
    ('byte_cat', 'null_ttb', False): (-1, 'byte_cat: tokens / ttb missing'),
    ('byte_cat', 'null_ttb', True): (-3, 'byte_cat_bwd: pass the byte ids the forward used (MOT_IDS_GIVEN)'),
    ('byte_cat', 'null_ids', False): (-1, 'byte_cat: ids missing'),
    ('byte_cat', 'null_ids', True): (-1, 'byte_cat: ids missing'),
    ('byte_cat', 'out_ids_padded_with_given_ids', False): (-1, 'byte_cat: out_ids_* need MOT_IDS_FROM_TTB'),
    ('byte_cat', 'out_ids_padded_with_given_ids', True): (-1, 'byte_cat: out_ids_* need MOT_IDS_FROM_TTB'),
    ('byte_cat', 'out_ids_pulled_with_given_ids', False): (-1, 'byte_cat: out_ids_* need MOT_IDS_FROM_TTB'),
    ('byte_cat', 'out_ids_pulled_with_given_ids', True): (-1, 'byte_cat: out_ids_* need MOT_IDS_FROM_TTB'),
    ('byte_cat', 'from_ttb_in_the_backward', True): (-3, 'byte_cat_bwd: pass the byte ids the forward used (MOT_IDS_GIVEN)'),
    ('byte_cat', 'bpt_0', False): (-3, 'byte_cat: bytes_per_token 0 outside [1, 64]'),
    ('byte_cat', 'bpt_0', True): (-3, 'byte_cat: bytes_per_token 0 outside [1, 64]'),
    ('byte_cat', 'bpt_above_max', False): (-3, 'byte_cat: bytes_per_token 65 outside [1, 64]'),
    ('byte_cat', 'bpt_above_max', True): (-3, 'byte_cat: bytes_per_token 65 outside [1, 64]'),
    ('byte_cat', 'workspace_null', True): (-5, 'byte_cat_bwd: needs 1024 16-byte aligned workspace bytes, got 1024'),
    ('byte_cat', 'workspace_too_small', True): (-5, 'byte_cat_bwd: needs 1024 16-byte aligned workspace bytes, got 1008'),
    ('byte_cat', 'workspace_misaligned', True): (-5, 'byte_cat_bwd: needs 1024 16-byte aligned workspace bytes, got 1024'),
    ('value_mix', 'bad_id_source', False): (-1, 'value_mix: bad id_source 7'),
    ('value_mix', 'bad_id_source', True): (-1, 'value_mix: bad id_source 7'),
    ('value_mix', 'ttb_elem_bytes_3', False): (-1, 'value_mix: ttb_elem_bytes must be 2 or 4'),
    ('value_mix', 'ttb_elem_bytes_3', True): (-1, 'value_mix: ttb_elem_bytes must be 2 or 4'),
    ('value_mix', 'pull_dir_7', False): (-1, 'value_mix: bad pull_dir 7'),
    ('value_mix', 'pull_dir_7', True): (-1, 'value_mix: bad pull_dir 7'),
    ('value_mix', 'ttb_rows_0', False): (-1, 'value_mix: ttb missing'),
    ('value_mix', 'ttb_rows_0', True): (-1, 'value_mix: ttb missing'),
    ('value_mix', 'null_ttb', False): (-1, 'value_mix: ttb missing'),
    ('value_mix', 'null_ttb', True): (-3, 'value_mix_bwd: pass the byte ids the forward used (MOT_IDS_GIVEN)'),
    ('value_mix', 'null_ids', False): (-1, 'value_mix: ids missing'),
    ('value_mix', 'null_ids', True): (-1, 'value_mix: ids missing'),
    ('value_mix', 'out_ids_padded_with_given_ids', False): (-1, 'value_mix: out_ids needs MOT_IDS_FROM_TTB'),
    ('value_mix', 'out_ids_padded_with_given_ids', True): (-1, 'value_mix: out_ids needs MOT_IDS_FROM_TTB'),
    ('value_mix', 'out_ids_pulled_with_given_ids', False): (-1, 'value_mix: out_ids needs MOT_IDS_FROM_TTB'),
    ('value_mix', 'out_ids_pulled_with_given_ids', True): (-1, 'value_mix: out_ids needs MOT_IDS_FROM_TTB'),
    ('value_mix', 'from_ttb_in_the_backward', True): (-3, 'value_mix_bwd: pass the byte ids the forward used (MOT_IDS_GIVEN)'),
    ('value_mix', 'bpt_0', False): (-3, 'value_mix: bytes_per_token 0 outside [1, 64]'),
    ('value_mix', 'bpt_0', True): (-3, 'value_mix: bytes_per_token 0 outside [1, 64]'),
    ('value_mix', 'bpt_above_max', False): (-3, 'value_mix: bytes_per_token 65 outside [1, 64]'),
    ('value_mix', 'bpt_above_max', True): (-3, 'value_mix: bytes_per_token 65 outside [1, 64]'),
    ('value_mix', 'workspace_null', False): (-5, 'value_mix: needs 1048576 16-byte aligned workspace bytes, got 1048576'),
    ('value_mix', 'workspace_null', True): (-5, 'value_mix_bwd: needs 2640896 16-byte aligned workspace bytes, got 2640896'),
    ('value_mix', 'workspace_too_small', False): (-5, 'value_mix: needs 1048576 16-byte aligned workspace bytes, got 1048560'),
    ('value_mix', 'workspace_too_small', True): (-5, 'value_mix_bwd: needs 2640896 16-byte aligned workspace bytes, got 2640880'),
    ('value_mix', 'workspace_misaligned', False): (-5, 'value_mix: needs 1048576 16-byte aligned workspace bytes, got 1048576'),
    ('value_mix', 'workspace_misaligned', True): (-5, 'value_mix_bwd: needs 2640896 16-byte aligned workspace bytes, got 2640896'),
    ('split_x0', 'bad_id_source', False): (-1, 'split_x0: bad id_source 7'),
    ('split_x0', 'bad_id_source', True): (-1, 'split_x0: bad id_source 7'),
    ('split_x0', 'ttb_elem_bytes_3', False): (-1, 'split_x0: ttb_elem_bytes must be 2 or 4'),
    ('split_x0', 'ttb_elem_bytes_3', True): (-1, 'split_x0: ttb_elem_bytes must be 2 or 4'),
    ('split_x0', 'pull_dir_7', False): (-1, 'split_x0: bad pull_dir 7'),
    ('split_x0', 'pull_dir_7', True): (-1, 'split_x0: bad pull_dir 7'),
    ('split_x0', 'ttb_rows_0', False): (-1, 'split_x0: ttb missing'),
    ('split_x0', 'ttb_rows_0', True): (-1, 'split_x0: ttb missing'),
    ('split_x0', 'null_ttb', False): (-1, 'split_x0: ttb missing'),
    ('split_x0', 'null_ttb', True): (-3, 'split_x0_bwd: pass the byte ids the forward used (MOT_IDS_GIVEN)'),
    ('split_x0', 'null_ids', False): (-1, 'split_x0: ids missing'),
    ('split_x0', 'null_ids', True): (-1, 'split_x0: ids missing'),
    ('split_x0', 'out_ids_padded_with_given_ids', False): (-1, 'split_x0: out_ids_* need MOT_IDS_FROM_TTB'),
    ('split_x0', 'out_ids_padded_with_given_ids', True): (-1, 'split_x0: out_ids_* need MOT_IDS_FROM_TTB'),
    ('split_x0', 'out_ids_pulled_with_given_ids', False): (-1, 'split_x0: out_ids_* need MOT_IDS_FROM_TTB'),
    ('split_x0', 'out_ids_pulled_with_given_ids', True): (-1, 'split_x0: out_ids_* need MOT_IDS_FROM_TTB'),
    ('split_x0', 'from_ttb_in_the_backward', True): (-3, 'split_x0_bwd: pass the byte ids the forward used (MOT_IDS_GIVEN)'),
    ('split_x0', 'bpt_0', False): (-3, 'split_x0: bytes_per_token 0 outside [1, 64]'),
    ('split_x0', 'bpt_0', True): (-3, 'split_x0: bytes_per_token 0 outside [1, 64]'),
    ('split_x0', 'bpt_above_max', False): (-3, 'split_x0: bytes_per_token 65 outside [1, 64]'),
    ('split_x0', 'bpt_above_max', True): (-3, 'split_x0: bytes_per_token 65 outside [1, 64]'),
    ('split_x0', 'workspace_null', False): (-5, 'split_x0: needs 2048 16-byte aligned workspace bytes, got 0'),
    ('split_x0', 'workspace_null', True): (-5, 'split_x0_bwd: needs 1070336 16-byte aligned workspace bytes, got 0'),
    ('split_x0', 'workspace_too_small', False): (-5, 'split_x0: needs 2048 16-byte aligned workspace bytes, got 2032'),
    ('split_x0', 'workspace_too_small', True): (-5, 'split_x0_bwd: needs 1070336 16-byte aligned workspace bytes, got 1070320'),
    ('split_x0', 'workspace_misaligned', False): (-5, 'split_x0: needs 2048 16-byte aligned workspace bytes, got 2048'),
    ('split_x0', 'workspace_misaligned', True): (-5, 'split_x0_bwd: needs 1070336 16-byte aligned workspace bytes, got 1070336'),
}


@pytest.mark.parametrize("front_end, fault, backward", sorted(EXPECTED))
def test_refusal_code_and_text(front_end, fault, backward):
    assert observe(front_end, fault, backward) == EXPECTED[(front_end, fault, backward)]


def test_table_covers_every_fault_for_every_front_end():
    for fe in FRONT_ENDS:
        for fault in FAULTS:
            if fe == "byte_cat" and fault.startswith("workspace"):
                assert (fe, fault, False) not in EXPECTED and (fe, fault, True) in EXPECTED   # its forward takes no workspace
            else:
                assert any((fe, fault, b) in EXPECTED for b in (False, True)), (fe, fault)
        assert (fe, "from_ttb_in_the_backward", False) not in EXPECTED                          # a valid forward
    assert all(rc != capi.MOT_OK and text for rc, text in EXPECTED.values())
