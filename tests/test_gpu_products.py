"""-m gpu: the six shared matrix-product launchers of csrc/mot_internal.hpp, called directly through the test-only probe
library (tests/native/libmot_probe.so) at the shapes of tests/gemm_cases.py, route by route, against float64 numpy on the
exact operand values (bf16 operands are drawn bf16-representable, so only the fp32 accumulation is under test).

Two bars, both required, because each misses what the other catches.  Per element, |got - ref| <= (K + 2) 2^-24 (|A|.|B|
+ |bias| + |C0|), the worst case of fp32 summation in any order, plus half a bf16 step of |ref| with bf16 output: it holds
for every element, so a wrong edge tile, a dropped bias or one missing reduction step in a few rows fails it however small
those rows are against the largest output element.  Whole tensor, max|got - ref| <= 2 max(max|peer - ref|, 1e-6 max|ref|)
with `peer` the same product in fp32 on the CPU (the bar assert_gemm_close uses for the concat product): the worst-case bound
is loose, and this one catches a kernel that loses blocked summation.  Every output buffer has a guard row above and below
and at least 4 guard columns; plain stores run on a NaN-filled C, C += launches on a seeded C0, and every guard element must
come back bit for bit.  Operands sit inside larger NaN-filled buffers, so a read past a logical edge stays inside the
allocation and poisons the result.  Products with 65 536 rows and more are checked on a seeded sample of rows (the first
and last 300, every 128- and 256-row panel boundary +-1, 512 random rows)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import gemm_cases as gc
from util_gpu import DEV

pytestmark = pytest.mark.gpu
U32 = 2.0 ** -24
HALF_BF16_STEP = 2.0 ** -8   # relative to |value|
NAN32, NAN16 = 0x7FC0DEAD, 0x7FC5   # the bit patterns a plain-store output starts from
LEAD, TAIL = 64, 256   # NaN-filled elements in front of and behind every operand
# whole-tensor factor over the CPU fp32 peer, for every launcher: the atomic C += launchers need no more either (largest ratio
# measured on an MI355X: 1.52 of the floor, tn-768x1536x65536, whose 15 reduction slices are unblocked fp32 chains of 4384 rows)
PEER_FACTOR = 2.0


@pytest.fixture(scope="module")
def probe():
    import mixture_of_tokenizers_amd  # noqa: F401
    return gc.load_probe()


def last_error():
    from mixture_of_tokenizers_amd import _capi
    return _capi.lib.mot_last_error().decode()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bf16_values(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy()


@functools.lru_cache(maxsize=4)
def operands(kind, rows, cols, inner, bf16, seed):
    """Seeded logical operands in fp32 (bf16-representable when `bf16`): X rows x inner, Y cols x inner (kind 'rows': C = X Y^T)
    or X inner x rows, Y inner x cols (kind 'tn': C = X^T Y)."""
    g = np.random.default_rng(seed)
    shx, shy = ((rows, inner), (cols, inner)) if kind == "rows" else ((inner, rows), (inner, cols))
    x, y = g.standard_normal(shx, dtype=np.float32), g.standard_normal(shy, dtype=np.float32)
    return (bf16_values(x), bf16_values(y)) if bf16 else (x, y)


def sample_rows(n, seed):
    if n < 65536:
        return np.arange(n)
    b = np.concatenate([np.arange(0, n, 128), np.arange(0, n, 256)])
    picks = [np.arange(300), np.arange(n - 300, n), b - 1, b, b + 1, np.random.default_rng(seed).integers(0, n, 512)]
    s = np.unique(np.concatenate(picks))
    return s[(s >= 0) & (s < n)]


@functools.lru_cache(maxsize=4)
def reference(kind, rows, cols, inner, bf16, seed, sample_seed):
    """(sampled rows, float64 product, float64 |X|.|Y|, CPU fp32 peer) of the logical product on the sampled output rows."""
    x, y = operands(kind, rows, cols, inner, bf16, seed)
    sel = sample_rows(rows, sample_seed)
    xs = torch.from_numpy(x[sel] if kind == "rows" else np.ascontiguousarray(x.T[sel]))
    yt = torch.from_numpy(y.T.copy() if kind == "rows" else y)
    ref = (xs.double() @ yt.double()).numpy()
    ab = (xs.double().abs() @ yt.double().abs()).numpy()
    peer = (xs @ yt).numpy()
    return sel, ref, ab, peer


def placed(vals, ld, dtype, off=0):
    """`vals` (rows x cols) on the GPU with leading dimension `ld`, first element `off` elements into the buffer's data, inside
    a NaN-filled buffer with LEAD elements in front and TAIL behind.  Returns (buffer, device address of element 0)."""
    rows, cols = vals.shape
    buf = torch.full((LEAD + off + rows * ld + TAIL,), float("nan"), dtype=dtype, device=DEV)
    body = buf[LEAD + off:LEAD + off + rows * ld].view(rows, ld)
    body[:, :cols] = torch.from_numpy(np.ascontiguousarray(vals)).to(DEV, dtype)
    return buf, buf.data_ptr() + (LEAD + off) * buf.element_size()


def output_buffer(rows, cols, ldc, bf16, c0):
    """C with a guard row above and below the logical rows and ldc - cols guard columns: NaN bits, or C0 everywhere."""
    if c0 is not None:
        buf = torch.from_numpy(c0).to(DEV, copy=True)
    elif bf16:
        buf = torch.full((rows + 2, ldc), NAN16, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    else:
        buf = torch.full((rows + 2, ldc), NAN32, dtype=torch.int32, device=DEV).view(torch.float32)
    return buf, buf.data_ptr() + ldc * buf.element_size()


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32).clone()


def check_guards(after, before, rows, cols, what):
    a, b = bits(after), before
    guard = torch.ones_like(a, dtype=torch.bool)
    guard[1:rows + 1, :cols] = False
    moved = (a != b) & guard
    assert not bool(moved.any()), f"{what}: {int(moved.sum())} guard elements changed, first at {moved.nonzero()[0].tolist()}"


def check_product(c, got, sel, ref, ab, peer, K, extra, out_bf16=False):
    """Both bars on the sampled rows: `extra` holds |bias| + |C0| per element (float64), `peer` the CPU fp32 result."""
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(got).all(), f"{c['id']}: {int((~np.isfinite(got)).sum())} non-finite outputs (unwritten or poisoned)"
    err = np.abs(got - ref)
    tol = (K + 2) * U32 * (ab + extra)
    if out_bf16:
        tol = tol * (1 + HALF_BF16_STEP) + HALF_BF16_STEP * np.abs(ref)
    over = err > tol
    if over.any():
        i = np.unravel_index(int(np.argmax(err - tol)), err.shape)
        row = int(sel[i[0]])
        raise AssertionError(f"{c['id']}: {int(over.sum())} of {err.size} elements over the per-element bound; worst at row {row} col {i[1]}: "
                             f"got {got[i]!r} ref {ref[i]!r} |err| {err[i]:.3e} bound {tol[i]:.3e}")
    e_got = float(err.max())
    e_peer = float(np.abs(np.asarray(peer, dtype=np.float64) - ref).max())
    floor = max(e_peer, 1e-6 * float(np.abs(ref).max()))
    ratio = e_got / floor
    print(f"{c['id']}: max err {e_got:.3e}, peer {e_peer:.3e}, ratio to the peer bar {ratio:.2f}")
    assert e_got <= PEER_FACTOR * floor, (f"{c['id']}: max|got - ref| {e_got:.3e} is {ratio:.2f} x max(max|peer - ref| {e_peer:.3e}, "
                                          f"1e-6 max|ref|); the bar is {PEER_FACTOR}")


def rows_case(probe, c, seed=0):
    n, R, Nc, L = c["n"], c["R"], c["Nc"], c["launcher"]
    bf16 = L == "bf16"
    out_bf16 = bool(c.get("out_bf16"))
    op_t = torch.bfloat16 if bf16 else torch.float32
    A, Bl = operands("rows", n, Nc, R, bf16, seed)
    Ab, a_ptr = placed(A, c["lda"], op_t, c["a_off"])
    Bb, b_ptr = placed(Bl if c["bt"] else Bl.T, c["ldb"], op_t)
    assert gc.route_of(probe, c, a_ptr, b_ptr) == c["route"], c["id"]
    g = np.random.default_rng(seed + 1)
    ldc = Nc + 4 + (3 if L == "rows" else 0)
    bias = bf16_values(g.standard_normal(Nc, dtype=np.float32)) if c["bias"] else None
    bias_d = placed(bias[None, :], Nc, op_t)[0] if c["bias"] else None
    bias_ptr = bias_d.data_ptr() + LEAD * bias_d.element_size() if c["bias"] else None
    c0 = g.standard_normal((n + 2, ldc), dtype=np.float32) if c["acc"] else None
    addend = g.standard_normal((n, ldc), dtype=np.float32) if c.get("addend") else None
    Cb, c_ptr = output_buffer(n, Nc, ldc, out_bf16, c0)
    before = bits(Cb)
    add_d = torch.from_numpy(addend).to(DEV) if addend is not None else None
    s = stream()
    if L == "rows":
        rc = probe.probe_gemm_rows(a_ptr, c["lda"], n, b_ptr, c["ldb"], R, Nc, c_ptr, ldc, c["bt"], bias_ptr, c["acc"], s)
    elif L == "f32_256":
        rc = probe.probe_gemm_rows_f32_256(a_ptr, c["lda"], n, b_ptr, c["ldb"], R, Nc, c_ptr, ldc, bias_ptr, c["acc"], s)
    else:
        rc = probe.probe_gemm_rows_bf16(a_ptr, c["lda"], n, b_ptr, c["ldb"], R, Nc, c_ptr, ldc, int(out_bf16), bias_ptr, c["acc"],
                                        add_d.data_ptr() if add_d is not None else None, s)
    torch.cuda.synchronize()
    assert rc == 0, f"{c['id']}: status {rc}: {last_error()}"
    check_guards(Cb, before, n, Nc, c["id"])
    sel, ref, ab, peer = reference("rows", n, Nc, R, bf16, seed, seed + 2)
    got = Cb[1:n + 1, :Nc][torch.from_numpy(sel).to(DEV)].float().cpu().numpy()
    ref, peer, extra = ref.copy(), peer.copy(), np.zeros_like(ref)
    for t in (bias[None, :] if bias is not None else None, c0[1:n + 1, :Nc][sel] if c0 is not None else None,
              addend[:, :Nc][sel] if addend is not None else None):
        if t is not None:   # (in the kernels' order: product, + bias, + C0 or addend)
            ref += t
            peer = (peer + t).astype(np.float32)
            extra += np.abs(t)
    if out_bf16:
        peer = bf16_values(peer)
    check_product(c, got, sel, ref, ab, peer, R, extra, out_bf16)


def sliced_case(probe, c, seed=0):
    n, R, Nc = c["n"], c["R"], c["Nc"]
    A, Bl = operands("rows", n, Nc, R, False, seed)
    Abuf, a_ptr = placed(A, c["lda"], torch.float32)
    Bbuf, b_ptr = placed(Bl if c["bt"] else Bl.T, c["ldb"], torch.float32)
    assert gc.route_of(probe, c, a_ptr, b_ptr) == c["route"], c["id"]
    pf = gc.sliced_part_floats(probe, c)
    part = torch.full((pf + TAIL,), float("nan"), device=DEV)
    part_tail = bits(part[pf:])
    ldc = Nc + 5
    outs = []
    for _ in range(2):   # the header's promise: the same bits on every run
        Cb, c_ptr = output_buffer(n, Nc, ldc, False, None)
        before = bits(Cb)
        rc = probe.probe_gemm_rows_sliced(a_ptr, c["lda"], n, b_ptr, c["ldb"], R, Nc, c_ptr, ldc, c["bt"], part.data_ptr(), pf, stream())
        torch.cuda.synchronize()
        assert rc == 0, f"{c['id']}: status {rc}: {last_error()}"
        check_guards(Cb, before, n, Nc, c["id"])
        assert torch.equal(bits(part[pf:]), part_tail), f"{c['id']}: the launch wrote past the partial-block floats it was given"
        outs.append(Cb)
    del Abuf, Bbuf
    assert torch.equal(bits(outs[0]), bits(outs[1])), f"{c['id']}: two runs differ"
    sel, ref, ab, peer = reference("rows", n, Nc, R, False, seed, seed + 2)
    check_product(c, outs[0][1:n + 1, :Nc].cpu().numpy()[sel], sel, ref, ab, peer, R, np.zeros_like(ref))


def tn_case(probe, c, seed=0):
    M, Nc, n, L = c["M"], c["Nc"], c["n"], c["launcher"]
    bf16 = L == "tn_bf16"
    op_t = torch.bfloat16 if bf16 else torch.float32
    A, B = operands("tn", M, Nc, n, bf16, seed)
    Ab, a_ptr = placed(A, c["lda"], op_t)
    Bb, b_ptr = placed(B, c["ldb"], op_t)
    ldc = Nc + 4 + (1 if L == "tn" else 0)
    c0 = np.random.default_rng(seed + 1).standard_normal((M + 2, ldc), dtype=np.float32)
    Cb, c_ptr = output_buffer(M, Nc, ldc, False, c0)
    before = bits(Cb)
    fn = probe.probe_gemm_tn_bf16 if bf16 else probe.probe_gemm_tn
    rc = fn(a_ptr, c["lda"], M, b_ptr, c["ldb"], Nc, n, c_ptr, ldc, stream())
    torch.cuda.synchronize()
    assert rc == 0, f"{c['id']}: status {rc}: {last_error()}"
    check_guards(Cb, before, M, Nc, c["id"])
    sel, ref, ab, peer = reference("tn", M, Nc, n, bf16, seed, seed + 2)
    t = c0[1:M + 1, :Nc]
    check_product(c, Cb[1:M + 1, :Nc].cpu().numpy(), sel, ref + t, ab, (t + peer).astype(np.float32), n, np.abs(t))


@pytest.mark.parametrize("case", gc.CASES, ids=lambda c: c["id"])
def test_product(probe, case):
    if case["launcher"] == "sliced":
        sliced_case(probe, case)
    elif case["launcher"] in ("tn", "tn_bf16"):
        tn_case(probe, case)
    else:
        rows_case(probe, case)


@pytest.mark.parametrize("case", gc.REFUSALS, ids=lambda c: c["id"])
def test_refusal_leaves_the_output_untouched(probe, case):
    """Shapes outside a launcher's contract: MOT_EUNSUPPORTED before any launch, every element of C as it was."""
    e_t = torch.bfloat16
    rows_a = case["n"]
    A, a_ptr = placed(np.ones((rows_a, case["lda"]), np.float32), case["lda"], e_t, case["a_off"])
    B, b_ptr = placed(np.ones((case["n"] if case["launcher"] == "tn_bf16" else case["Nc"], case["ldb"]), np.float32), case["ldb"], e_t,
                      case["b_off"])
    out_rows = case["M"] if case["launcher"] == "tn_bf16" else case["n"]
    ldc = case["Nc"] + 4
    c0 = np.random.default_rng(5).standard_normal((out_rows + 2, ldc), dtype=np.float32)
    Cb, c_ptr = output_buffer(out_rows, case["Nc"], ldc, False, c0)
    if case.get("out_bf16"):
        Cb, c_ptr = output_buffer(out_rows, case["Nc"], ldc, True, None)
    before = bits(Cb)
    if case["launcher"] == "bf16":
        rc = probe.probe_gemm_rows_bf16(a_ptr, case["lda"], case["n"], b_ptr, case["ldb"], case["R"], case["Nc"], c_ptr, ldc, case["out_bf16"], None,
                                        case["acc"], None, stream())
    else:
        rc = probe.probe_gemm_tn_bf16(a_ptr, case["lda"], case["M"], b_ptr, case["ldb"], case["Nc"], case["n"], c_ptr, ldc, stream())
    torch.cuda.synchronize()
    assert rc == gc.MOT_EUNSUPPORTED, f"{case['id']}: status {rc}"
    assert torch.equal(bits(Cb), before), f"{case['id']}: C changed"
