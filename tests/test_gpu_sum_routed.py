"""-m gpu: the routed SUM forward (index pre-pass + token rows bucketed by id over the XCDs; fp32 tables from 131 072 tokens on) computes
exactly what the fused kernel computes: one routed launch against the same rows run as launches below the routing threshold,
compared with torch.equal, with the counters and the out-of-range status bits."""
import numpy as np
import pytest
import torch

import golden_inputs as gi
from util_gpu import DEV, dev, f32

pytestmark = pytest.mark.gpu
ROUTE_MIN = 131072          # mot_embed.hip kRouteMinTokens


@pytest.fixture(scope="module")
def mot():
    import mixture_of_tokenizers_amd as m
    return m


def status_of(mot):
    try:
        mot.check_status()
    except IndexError as e:
        return str(e)
    return None


def split_vs_routed(mot, toks, Et, Eb, bpt, **kw):
    """(routed output, counters, status) and the same from launches of fewer than ROUTE_MIN tokens each."""
    B, T = toks.shape
    assert B * T >= ROUTE_MIN
    status_of(mot)
    cnt = torch.zeros(4, dtype=torch.int64, device=DEV)
    x = mot.embed_mix(toks, Et, Eb, mode="sum", bpt=bpt, counters=cnt, **kw)
    st = status_of(mot)
    rows = max(1, (ROUTE_MIN - 1) // T)
    cnt2 = torch.zeros(4, dtype=torch.int64, device=DEV)
    parts = [mot.embed_mix(toks[r:r + rows].contiguous(), Et, Eb, mode="sum", bpt=bpt, counters=cnt2, **kw) for r in range(0, B, rows)]
    st2 = status_of(mot)
    return (x, cnt, st), (torch.cat(parts), cnt2, st2)


def assert_same(a, b):
    assert torch.equal(a[0], b[0])
    assert torch.equal(a[1], b[1])
    assert a[2] == b[2]


def c4_inputs(vocab=50257, D=768, Db=48, bpt=16):
    g = torch.Generator(device=DEV).manual_seed(5)
    Et = torch.randn((vocab, D), generator=g, device=DEV)
    Eb = torch.randn((gi.BYTE_VOCAB, Db), generator=g, device=DEV)
    tab = dev(gi.synth_ttb(6, vocab, bpt, "left"))
    return Et, Eb, tab


def test_routed_c4_size(mot):
    """The bench's shape: 256 x 2048 FineWeb-shaped ids, pull-left, output norm."""
    Et, Eb, tab = c4_inputs()
    toks = dev(gi.fineweb_like_tokens(7, 256, 2048, vocab=50257))
    a, b = split_vs_routed(mot, toks, Et, Eb, 16, ttb=tab, pull="left", norm_out=True)
    assert_same(a, b)
    assert a[2] is None


VARIANTS = [
    dict(pull="left", norm_out=True),
    dict(pull="right", norm_tok=True, norm_out=True),
    dict(pull=None, norm_byte=True),
    dict(pull="left", add_padded=True, norm_tok=True, norm_out=True),
    dict(pull="right", add_padded=True, scaled=True),
    dict(pull="left", scaled=True, norm_out=True),
]


@pytest.mark.parametrize("kw", VARIANTS, ids=lambda k: "-".join(f"{a}={v}" for a, v in k.items()))
def test_routed_variants_odd_T(mot, kw):
    """T = 2000 is not a multiple of the 32-token unit: the last unit of every row is short."""
    kw = dict(kw)
    Vt, bpt = 4096, 16
    Et, Eb, _ = c4_inputs(Vt)
    tab = dev(gi.synth_ttb(8, Vt, bpt, kw["pull"] or "left"))
    toks = dev(gi.fineweb_like_tokens(9, 67, 2000, vocab=Vt, eot_p=0.01))
    if kw.pop("scaled", False):
        kw.update(scale_tok=torch.tensor(1.3, device=DEV), scale_byte=torch.tensor(0.6, device=DEV))
    a, b = split_vs_routed(mot, toks, Et, Eb, bpt, ttb=tab, **kw)
    assert_same(a, b)


@pytest.mark.parametrize("ids", ["one_bucket", "one_id"])
def test_routed_skewed_ids(mot, ids):
    """Every token in one bucket, or one repeated id: the other buckets are empty and their workgroups steal every item."""
    Vt, bpt = 4096, 16
    Et, Eb, _ = c4_inputs(Vt)
    tab = dev(gi.synth_ttb(12, Vt, bpt, "left"))
    t = gi.fineweb_like_tokens(13, 64, 2048, vocab=Vt, eot_p=0.0)
    t = (t & ~7) + 3 if ids == "one_bucket" else np.full_like(t, 1234)
    a, b = split_vs_routed(mot, dev(t.astype(np.int32)), Et, Eb, bpt, ttb=tab, pull="left", norm_out=True)
    assert_same(a, b)


def test_routed_counters_and_status(mot):
    """Counters add up once per position; a token id past the tables and a byte id past the byte table set the same status
    bits as the fused kernel."""
    Vt, bpt = 4096, 16
    Et, Eb, _ = c4_inputs(Vt)
    tab = gi.synth_ttb(14, Vt, bpt, "left")
    tab[5, -1] = 999
    t = gi.edge_tokens(15, 64, 2048, Vt)
    t[3, 100] = 5
    t[7, 7] = Vt + 3
    a, b = split_vs_routed(mot, dev(t), Et, Eb, bpt, ttb=dev(tab), pull="left", norm_out=True)
    assert_same(a, b)
    assert "token id" in a[2] and "byte id" in a[2]
    assert a[1][0].item() == 64 * 2048


def test_routed_hip_graph_replay(mot):
    """The pre-pass and the routed kernel are one capturable sequence: capture, change the batch in place, replay, compare with
    an eager launch."""
    Vt, bpt, B, T, D = 4096, 16, 64, 2048, 768
    Et, Eb, _ = c4_inputs(Vt)
    tab = dev(gi.synth_ttb(16, Vt, bpt, "left"))
    toks = dev(gi.fineweb_like_tokens(17, B, T, vocab=Vt, eot_p=0.01))
    out = torch.empty((B, T, D), device=DEV)
    kw = dict(mode="sum", bpt=bpt, ttb=tab, pull="left", norm_byte=True, norm_out=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        mot.embed_mix(toks, Et, Eb, out=out, **kw)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        mot.embed_mix(toks, Et, Eb, out=out, **kw)
    toks.copy_(dev(gi.fineweb_like_tokens(18, B, T, vocab=Vt, eot_p=0.01)))
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    ref = mot.embed_mix(toks, Et, Eb, **kw)
    assert torch.equal(out, ref)
    rows = (ROUTE_MIN - 1) // T
    split = torch.cat([mot.embed_mix(toks[r:r + rows].contiguous(), Et, Eb, **kw) for r in range(0, B, rows)])
    assert torch.equal(out, split)
