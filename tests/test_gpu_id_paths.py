"""The three places the byte ids of a front-end call can live, for the two front-ends that make them with the index kernels
(byte_fc_mix, value_mix; csrc/mot_desc.hpp, launch_ids_from_ttb), float32 (the composed path) and bfloat16:

  (a) ids from the token->byte table under torch.no_grad(): they stay in the call's workspace;
  (b) the same with the ids returned / saved: they are written into the caller's tensors;
  (c) the ids of (b) passed back as `ids`.

The same kernels read the same ids, so the three outputs are the same BITS (a condition, not a tolerance), and the ids of (b) are
what the oracle's tokens_to_bytes and pull_from_left / pull_from_right give (the restatement every id test here compares with).
B = 2, T = 33: ragged against the 16- and the 32-token units and one token past a tile edge; the table has pad entries, every row of
tokens has EOT tokens (the last table row), one of them first in its row."""
import functools

import numpy as np
import pytest
import torch

import golden_inputs as gi
from oracle import oracle as orc
from util_gpu import DEV, dev, host

pytestmark = pytest.mark.gpu

B, T, BPT, DB, VT = 2, 33, 4, 8, 61
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


@functools.lru_cache(maxsize=None)
def problem(pull):
    """Tokens, table and the oracle's ids: computed once per pull direction and shared; no test writes to them."""
    tab = gi.synth_ttb(7, VT, BPT, "right" if pull == "right" else "left")
    toks = gi.edge_tokens(11, B, T, VT)
    toks[0, 0] = toks[0, 17] = toks[1, 16] = toks[1, 32] = VT - 1   # EOT first in a row, either side of the 16-token edge, last in a row
    assert (tab == gi.PAD).any() and (toks == VT - 1).any(axis=1).all()
    padded = orc.tokens_to_bytes(toks, tab.astype(np.float32))
    pulled = {"left": orc.pull_from_left, "right": orc.pull_from_right}[pull](padded, BPT, gi.PAD, gi.EOT) if pull else padded
    return toks, tab, padded, pulled


def tables(seed, dt, *shapes):
    return [dev(gi.normal_table(seed + j, *s), DTYPES[dt]) for j, s in enumerate(shapes)]


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("pull", ["left", "right", None])
@pytest.mark.parametrize("front_end", ["byte_fc_mix", "value_mix"])
def test_three_id_paths_give_the_same_bits(front_end, pull, dt):
    import mixture_of_tokenizers_amd as mot
    toks, tab, padded, pulled = problem(pull)
    tk, tb = dev(toks), dev(tab)
    if front_end == "byte_fc_mix":   # model_dim 32
        Et, Eb, W = tables(20, dt, (VT, 32), (gi.BYTE_VOCAB, DB), (32, BPT * DB))
        with torch.no_grad():
            a = (mot.byte_fc_mix(tk, Et, Eb, W, bpt=BPT, ttb=tb, pull=pull),)
            r = mot.byte_fc_mix(tk, Et, Eb, W, bpt=BPT, ttb=tb, pull=pull, return_ids=True)
            b, ids_b = (r.x,), r.ids_pulled
            np.testing.assert_array_equal(host(r.ids_padded), padded)
            c = (mot.byte_fc_mix(tk, Et, Eb, W, bpt=BPT, ids=ids_b),)
    else:                            # token_dim 16, out_dim 32, 2 slots
        Vt, Vb = tables(30, dt, (VT, 16), (VT, 16)), tables(40, dt, (gi.BYTE_VOCAB, DB), (gi.BYTE_VOCAB, DB))
        W = tables(50, dt, (32, 16 + BPT * DB), (32, 16 + BPT * DB))
        with torch.no_grad():
            a = mot.value_mix(tk, Vt, Vb, W, bpt=BPT, ttb=tb, pull=pull)
            b, ids_b, _ = mot.functional._value_mix_fwd(tk, Vt, Vb, W, bpt=BPT, ttb=tb, pull=pull, save=True)
            c = mot.value_mix(tk, Vt, Vb, W, bpt=BPT, ids=ids_b)
    mot.check_status()
    np.testing.assert_array_equal(host(ids_b), pulled)
    assert len(a) == len(b) == len(c)
    for xa, xb, xc in zip(a, b, c):
        assert xa.dtype == DTYPES[dt] and tuple(xa.shape) == (B, T, 32) and bool(torch.isfinite(xa.float()).all())
        assert torch.equal(xa, xb), "ids in the workspace vs ids in the caller's tensors"
        assert torch.equal(xb, xc), "ids made by the call vs the same ids given"
