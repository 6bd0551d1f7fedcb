"""-m gpu: the three launchers the linear front-ends share (csrc/mot_lincore.hpp) -- launch_rows_finish / _tok, the forward's last
pass; launch_rows_norm_bwd, the way back through its norm; launch_count_pads, the id statistics -- called directly through the
test-only probe library (tests/native/libmot_probe.so, entries in mot_probe_rows.cpp), the route tests/test_gpu_products.py
takes for the matrix products.

Reference: float64 numpy on seeded standard-normal inputs, rounded to bf16 first for the bf16 cases.  Shapes are the smallest
that reach each branch of the kernels: one 16-byte chunk, a row that is no whole number of chunks (the element-wise path), 65
chunks (lane 0 holds two, every other lane one), 2048 columns (every chunk a lane can hold), and 64 chunks one element past an
aligned address (the element-wise path by alignment); 1 row and 5 (the second workgroup has one live wave of four).

Bars.  fp32 outputs and the factors: util_gpu.assert_close as it stands, 1e-6 + 1e-6 |ref| (the outputs are O(1): normalised
rows and gradients of standard-normal rows).  bf16 outputs: within one bf16 step, 2^-8 |ref|, of the float64 result -- fp32
arithmetic and one rounding at the store; the reference applies the s = bf16(tok + y) rounding of the token-row form itself.
Every output sits in a buffer of NaN bits with a guard row above and below and guard columns behind a strided row; the guards
must come back bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import gemm_cases as gc
from util_gpu import DEV, assert_close

pytestmark = pytest.mark.gpu
F32, BF16 = 0, 1                      # MotDType
STATUS_TOKEN_OOR, STATUS_BYTE_OOR = 1, 2
BF16_STEP = 2.0 ** -8                 # relative to |ref|
LEAD = 64                             # elements in front of every operand: keeps a 16-byte aligned start for both dtypes
EPS = {F32: 2.0 ** -23, BF16: 2.0 ** -7}   # the eps <= 0 defaults of the fp32 and the bf16 front-ends
TORCH_T = {F32: torch.float32, BF16: torch.bfloat16}
ROWS = (1, 5)


def dims(dtype):
    """(dim, offset of the base in elements past an aligned address)"""
    vec = 8 if dtype == BF16 else 4
    return [(vec, 0), (vec * 3 // 2, 0), (64 * vec + vec, 0), (2048, 0), (64 * vec, 1)]


CASES = [pytest.param(dt, dim, off, id=f"{'bf16' if dt else 'f32'}-dim{dim}{'-misaligned' if off else ''}") for dt in (F32, BF16) for dim, off in dims(dt)]


@pytest.fixture(scope="module")
def probe():
    import mixture_of_tokenizers_amd  # noqa: F401
    lib = gc.load_probe()
    vp, i, i64, f = C.c_void_p, C.c_int, C.c_int64, C.c_float
    lib.probe_rows_finish.argtypes = [vp, i64, i, i, f, vp, i, vp]
    lib.probe_rows_finish_tok.argtypes = [vp, vp, vp, i64, i64, i, i, f, vp, vp, i, vp]
    lib.probe_rows_norm_bwd.argtypes = [vp, vp, vp, i64, i, i, vp, i64, vp, i64, i, vp]
    lib.probe_count_pads.argtypes = [vp, vp, i64, i64, i64, vp, vp]
    for name in ("probe_rows_finish", "probe_rows_finish_tok", "probe_rows_norm_bwd", "probe_count_pads"):
        getattr(lib, name).restype = i
    return lib


def run(fn, *args):
    from mixture_of_tokenizers_amd import _capi
    rc = fn(*args, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0, f"status {rc}: {_capi.lib.mot_last_error().decode()}"


def values(shape, dtype, seed):
    """seeded standard-normal values as float64, bf16-representable for the bf16 cases"""
    a = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    return as_dtype(a, dtype)


def as_dtype(a, dtype):
    """float64 values of `a` rounded to fp32, and to bf16 behind that for the bf16 cases (the order the kernels round in)"""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return (t.to(torch.bfloat16).float() if dtype == BF16 else t).numpy().astype(np.float64)


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32).clone()


class Placed:
    """rows x cols of `torch_t` with row stride ld, row 0 `off` elements past an aligned address, inside a buffer of NaN bits
    that has LEAD elements in front, a guard row above and below and ld - cols guard columns.  vals None: all NaN bits."""

    def __init__(self, rows, cols, torch_t, off=0, ld=None, vals=None):
        self.rows, self.cols, self.ld = rows, cols, ld or cols
        self.buf = torch.full((LEAD + off + (rows + 2) * self.ld,), float("nan"), dtype=torch_t, device=DEV)
        self.grid = self.buf[LEAD + off:].view(rows + 2, self.ld)
        if vals is not None:
            self.grid[1:rows + 1, :cols] = torch.from_numpy(np.ascontiguousarray(vals)).to(DEV, torch_t)
        self.guard = torch.ones_like(self.buf, dtype=torch.bool)
        self.guard[LEAD + off:].view(rows + 2, self.ld)[1:rows + 1, :cols] = False
        self.ptr = self.grid[1].data_ptr()
        self.before = bits(self.buf)

    def result(self):
        """the logical values as float64, after checking that nothing around them moved"""
        moved = (bits(self.buf) != self.before) & self.guard
        assert not bool(moved.any()), f"{int(moved.sum())} guard elements changed, first at {moved.nonzero()[0].tolist()}"
        return self.grid[1:self.rows + 1, :self.cols].double().cpu().numpy()


def check(got, ref, bf16_out):
    if not bf16_out:
        return assert_close(got, ref)
    assert np.isfinite(got).all()
    excess = np.abs(got - ref) - BF16_STEP * np.abs(ref)
    assert (excess <= 0).all(), f"max excess over one bf16 step {excess.max():.3e} at {np.unravel_index(excess.argmax(), excess.shape)}"


def finish_ref(s, norm, eps):
    r = 1.0 / np.sqrt((s * s).mean(axis=1) + eps) if norm else np.ones(s.shape[0])
    return s * r[:, None], r


@pytest.mark.parametrize("norm", (1, 0), ids=("norm", "plain"))
@pytest.mark.parametrize("dtype,dim,off", CASES)
def test_rows_finish(probe, dtype, dim, off, norm):
    for rows in ROWS:
        y = values((rows, dim), dtype, seed=rows)
        ref, r = finish_ref(y, norm, EPS[dtype])
        for with_factor in (True, False):
            out = Placed(rows, dim, TORCH_T[dtype], off, vals=y)
            fac = Placed(1, rows, torch.float32)
            run(probe.probe_rows_finish, out.ptr, rows, dim, norm, EPS[dtype], fac.ptr if with_factor else None, dtype)
            check(out.result(), ref, dtype == BF16)
            if with_factor:
                assert_close(fac.result()[0], r)
            else:
                fac.result()   # untouched


@pytest.mark.parametrize("norm", (1, 0), ids=("norm", "plain"))
@pytest.mark.parametrize("dtype,dim,off", CASES)
def test_rows_finish_with_the_token_row(probe, dtype, dim, off, norm):
    """s = bf16(tok + y) for bf16 (fp32: tok + y); with 5 rows one token id is out of range: row 0 is used and the token bit is
    raised beside the bit the status word already held.  byte_fc_mix only sends chunked dims; the element-wise ones are here too
    because the kernel has that path in this form as well."""
    tok_rows = 7
    table = values((tok_rows, dim), dtype, seed=11)
    for rows in ROWS:
        y = values((rows, dim), dtype, seed=rows)
        tokens = np.random.default_rng(rows + 20).integers(0, tok_rows, rows).astype(np.int32)
        if rows > 1:
            tokens[3] = tok_rows
        used = np.where((tokens >= 0) & (tokens < tok_rows), tokens, 0)
        ref, r = finish_ref(as_dtype(table[used] + y, dtype), norm, EPS[dtype])
        out = Placed(rows, dim, TORCH_T[dtype], off, vals=y)
        tab = Placed(tok_rows, dim, TORCH_T[dtype], off, vals=table)
        fac = Placed(1, rows, torch.float32)
        tok_d = torch.from_numpy(tokens).to(DEV)
        status = torch.full((1,), STATUS_BYTE_OOR, dtype=torch.int32, device=DEV)
        run(probe.probe_rows_finish_tok, out.ptr, tok_d.data_ptr(), tab.ptr, tok_rows, rows, dim, norm, EPS[dtype], fac.ptr, status.data_ptr(), dtype)
        check(out.result(), ref, dtype == BF16)
        assert_close(fac.result()[0], r)
        tab.result()
        assert int(status.item()) == STATUS_BYTE_OOR | (STATUS_TOKEN_OOR if rows > 1 else 0)


@pytest.mark.parametrize("norm", (1, 0), ids=("norm", "plain"))
@pytest.mark.parametrize("dtype,dim,off", CASES)
def test_rows_norm_bwd(probe, dtype, dim, off, norm):
    """x and rnorm are what the forward saves: a normalised standard-normal row (rounded to the dtype) and its fp32 factor.
    Output stride dim and dim + 8; the output in the dtype alone, the fp32 output alone, and both together."""
    for rows in ROWS:
        y = np.random.default_rng(rows + 40).standard_normal((rows, dim))
        x, r = finish_ref(y, 1, EPS[dtype])
        x, r = as_dtype(x, dtype), as_dtype(r, F32)
        g = values((rows, dim), dtype, seed=rows + 50)
        ref = r[:, None] * (g - x * (g * x).mean(axis=1)[:, None]) if norm else g
        g_d, x_d = Placed(rows, dim, TORCH_T[dtype], off, vals=g), Placed(rows, dim, TORCH_T[dtype], off, vals=x)
        r_d = torch.from_numpy(r.astype(np.float32)).to(DEV)
        for ld in (dim, dim + 8):
            for typed, f32 in ((True, False), (False, True), (True, True)):
                dy = Placed(rows, dim, TORCH_T[dtype], off, ld)
                dy32 = Placed(rows, dim, torch.float32, off, ld)
                run(probe.probe_rows_norm_bwd, g_d.ptr, x_d.ptr if norm else None, r_d.data_ptr() if norm else None, rows, dim, norm,
                    dy.ptr if typed else None, ld, dy32.ptr if f32 else None, ld, dtype)
                for p, used, bf16_out in ((dy, typed, dtype == BF16), (dy32, f32, False)):
                    got = p.result()
                    if used:
                        check(got, ref, bf16_out)
                    else:
                        assert np.isnan(got).all()
        g_d.result(), x_d.result()


@pytest.mark.parametrize("with_padded", (True, False), ids=("padded", "ids_given"))
@pytest.mark.parametrize("n_slots", (1, 256 * 16 + 1))
def test_count_pads(probe, n_slots, with_padded):
    """tokens, byte slots and -- with the ids before the pull given -- the pads before and after it, added onto what the counters
    held; 256 * 16 + 1 slots are the first count that takes a second workgroup."""
    pad, n_tokens = 456, 17
    g = np.random.default_rng(n_slots)
    padded, after = g.integers(454, 458, n_slots), g.integers(454, 458, n_slots)
    start = np.array([3, 5, 7, 11], dtype=np.int64)
    counters = torch.from_numpy(start.copy()).to(DEV)
    p_d, a_d = torch.from_numpy(padded).to(DEV), torch.from_numpy(after).to(DEV)
    run(probe.probe_count_pads, p_d.data_ptr() if with_padded else None, a_d.data_ptr(), n_slots, pad, n_tokens, counters.data_ptr())
    want = start + np.array([n_tokens, n_slots, (padded == pad).sum() if with_padded else 0, (after == pad).sum() if with_padded else 0])
    assert counters.cpu().numpy().tolist() == want.tolist()
