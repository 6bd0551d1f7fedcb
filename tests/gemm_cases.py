"""The shape table of the shared matrix-product launchers (csrc/mot_internal.hpp) and the test-only probe library that calls
them (tests/native/libmot_probe.so, built by csrc/Makefile).  tests/test_gpu_products.py runs every case against a float64
reference; tests/test_gemm_routes.py checks on the CPU that each case still takes the route it names, and that every
launcher's cases reach both sides of each of its route predicates.

A case is a dict: `launcher`, `id`, `route` and the shape.  Products of rows (`rows`, `sliced`, `f32_256`, `bf16`):
C[n][c] = sum_r A[n][r] * B[c][r] with A n x R (leading dimension lda, first element `a_off` elements past an aligned
address) and B Nc x R when `bt` (else R x Nc).  Transposed products (`tn`, `tn_bf16`): C[m][k] += sum_i A[i][m] * B[i][k]
with A n x M and B n x Nc."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

PROBE_PATH = Path(__file__).resolve().parent / "native" / "libmot_probe.so"
MOT_EUNSUPPORTED = -3
FAKE_BASE = 1 << 20   # an aligned stand-in address for the host-only route predicates (never dereferenced)
_vp, _i, _i64, _sz = C.c_void_p, C.c_int, C.c_int64, C.c_size_t


def load_probe():
    lib = C.CDLL(str(PROBE_PATH))
    sig = {
        "probe_gemm_rows": [_vp, _i, _i64, _vp, _i, _i, _i, _vp, _i, _i, _vp, _i, _vp],
        "probe_gemm_rows_sliced": [_vp, _i, _i64, _vp, _i, _i, _i, _vp, _i, _i, _vp, _sz, _vp],
        "probe_gemm_rows_f32_256": [_vp, _i, _i64, _vp, _i, _i, _i, _vp, _i, _vp, _i, _vp],
        "probe_gemm_rows_bf16": [_vp, _i, _i64, _vp, _i, _i, _i, _vp, _i, _i, _vp, _i, _vp, _vp],
        "probe_gemm_tn": [_vp, _i, _i, _vp, _i, _i, _i64, _vp, _i, _vp],
        "probe_gemm_tn_bf16": [_vp, _i, _i, _vp, _i, _i, _i64, _vp, _i, _vp],
        "probe_gemm_rows_f32_256_usable": [_vp, _i, _i64, _vp, _i, _i, _i],
        "probe_gemm_rows_bf16_256_usable": [_vp, _i, _i64, _vp, _i, _i, _i],
        "probe_gemm_rows_sliced_floats": [_i64, _i, _i],
    }
    for name, args in sig.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = _sz if name == "probe_gemm_rows_sliced_floats" else _i
    return lib


def _rows(launcher, n, R, Nc, **kw):
    c = dict(launcher=launcher, n=n, R=R, Nc=Nc, lda=kw.pop("lda", R), a_off=kw.pop("a_off", 0), bt=kw.pop("bt", 1), bias=kw.pop("bias", 0),
             acc=kw.pop("acc", 0), sample=n >= 65536)
    c.update(kw)
    c["ldb"] = c["R"] if c["bt"] else c["Nc"]
    return c


def _tn(launcher, M, Nc, n, **kw):
    c = dict(launcher=launcher, M=M, Nc=Nc, n=n, lda=kw.pop("lda", M), ldb=kw.pop("ldb", Nc), sample=False)
    c.update(kw)
    return c


def _cases():
    out = []
    # launch_gemm_rows: 256 x 128 LDS-DMA kernel (B transposed, Nc % 128, R % 16, n >= 512, 16-byte aligned) or the 128 x 128 kernels
    rows_shapes = [
        ("1x64x64", 1, 64, 64, {}), ("127x17x100", 127, 17, 100, {}), ("129x768x130", 129, 768, 130, {}), ("511x768x768", 511, 768, 768, {}),
        ("512x16x128", 512, 16, 128, {}), ("513x768x768", 513, 768, 768, {}), ("1000x354x768", 1000, 354, 768, {}),
        ("700x768x200", 700, 768, 200, {}), ("2600x768x2048", 2600, 768, 2048, {}),
        ("1000x768x768_lda772", 1000, 768, 768, dict(lda=772)), ("1000x768x768_Aoff1", 1000, 768, 768, dict(a_off=1)),
    ]
    for name, n, R, Nc, kw in rows_shapes:
        for bt in (1, 0):
            for bias in (0, 1):
                for acc in (0, 1):
                    out.append(_rows("rows", n, R, Nc, bt=bt, bias=bias, acc=acc, id=f"rows-{name}-{'bt' if bt else 'nt'}-b{bias}a{acc}", **kw))
    for bt, bias, acc in ((1, 0, 0), (1, 1, 1), (0, 1, 0)):
        out.append(_rows("rows", 65573, 2048, 2048, bt=bt, bias=bias, acc=acc, id=f"rows-65573x2048x2048-{'bt' if bt else 'nt'}-b{bias}a{acc}"))
    for c in out:
        c["route"] = "256" if c["bt"] and c["R"] % 16 == 0 and c["Nc"] % 128 == 0 and c["n"] >= 512 and c["a_off"] == 0 else "128"
    # launch_gemm_rows_sliced: split reduction for few rows (n <= 1024, R >= 256), else launch_gemm_rows
    for name, n, R, Nc, route, part in (("132x2048x2048", 132, 2048, 2048, "sliced", "fit"), ("458x768x768", 458, 768, 768, "sliced", "fit"),
                                        ("132x300x256", 132, 300, 256, "sliced", "fit"), ("1024x256x128", 1024, 256, 128, "sliced", "fit"),
                                        ("1025x256x128", 1025, 256, 128, "fallback", "fit"),
                                        ("458x768x768_small_part", 458, 768, 768, "fallback", "short")):
        for bt in (1, 0):
            out.append(_rows("sliced", n, R, Nc, bt=bt, part=part, route=route, id=f"sliced-{name}-{'bt' if bt else 'nt'}"))
    # launch_gemm_rows_f32_256 called directly (the cross-attention backward's transposed-weight route)
    out.append(_rows("f32_256", 1024, 768, 768, bias=1, acc=1, route="256", id="f32_256-1024x768x768-b1a1"))
    out.append(_rows("f32_256", 777, 512, 384, route="256", id="f32_256-777x512x384-b0a0"))
    # launch_gemm_rows_bf16: 256 x 256 LDS-DMA kernel (Nc % 256, R % 32, n >= 512) or the 128 x 128 kernel
    for name, n, R, Nc, route in (("512x32x256", 512, 32, 256, "256"), ("1100x768x768", 1100, 768, 768, "256"),
                                  ("65541x2048x2048", 65541, 2048, 2048, "256"), ("1x8x8", 1, 8, 8, "128"),
                                  ("511x768x768", 511, 768, 768, "128"), ("600x72x100", 600, 72, 100, "128"), ("700x768x640", 700, 768, 640, "128")):
        for ob, bias, acc, add in ((1, 0, 0, 0), (1, 1, 0, 0), (0, 0, 0, 0), (0, 1, 0, 0), (0, 1, 1, 0), (0, 0, 0, 1)):
            tag = f"{'o16' if ob else 'o32'}-b{bias}" + ("-acc" if acc else "") + ("-addend" if add else "")
            out.append(_rows("bf16", n, R, Nc, out_bf16=ob, bias=bias, acc=acc, addend=add, route=route, id=f"bf16-{name}-{tag}"))
    # launch_gemm_tn: one kernel, reduction split over n in whole 256-row pieces; C += on a non-zero C0
    for name, M, Nc, n, kw in (("1x1x1", 1, 1, 1, {}), ("100x130x15", 100, 130, 15, {}), ("768x768x255", 768, 768, 255, {}),
                               ("768x768x256", 768, 768, 256, {}), ("768x768x257", 768, 768, 257, {}), ("768x1536x65536", 768, 1536, 65536, {}),
                               ("96x100x700_lda97_ldb103", 96, 100, 700, dict(lda=97, ldb=103))):
        out.append(_tn("tn", M, Nc, n, route="tn", id=f"tn-{name}", **kw))
    # launch_gemm_tn_bf16: 8 to 32 reduction slices of at least 4 * 64 rows
    for name, M, Nc, n in (("8x8x1", 8, 8, 1), ("136x264x1000", 136, 264, 1000), ("128x128x200", 128, 128, 200),
                           ("768x768x2000_8slices", 768, 768, 2000), ("128x128x65536_32slices", 128, 128, 65536), ("768x768x65539", 768, 768, 65539)):
        out.append(_tn("tn_bf16", M, Nc, n, route="tn", id=f"tn_bf16-{name}"))
    return out


CASES = _cases()
assert len({c["id"] for c in CASES}) == len(CASES)

# launches each launcher must refuse with MOT_EUNSUPPORTED before touching anything: (id, launcher, shape, operand offsets in elements)
REFUSALS = [
    dict(id="bf16-R12", launcher="bf16", n=64, R=12, Nc=64, lda=16, ldb=16, a_off=0, b_off=0, out_bf16=0, acc=0),
    dict(id="bf16-lda20", launcher="bf16", n=64, R=16, Nc=64, lda=20, ldb=16, a_off=0, b_off=0, out_bf16=0, acc=0),
    dict(id="bf16-A_misaligned", launcher="bf16", n=64, R=16, Nc=64, lda=16, ldb=16, a_off=4, b_off=0, out_bf16=0, acc=0),
    dict(id="bf16-acc_into_bf16", launcher="bf16", n=64, R=16, Nc=64, lda=16, ldb=16, a_off=0, b_off=0, out_bf16=1, acc=1),
    dict(id="tn_bf16-M100", launcher="tn_bf16", M=100, Nc=64, n=64, lda=104, ldb=64, a_off=0, b_off=0),
    dict(id="tn_bf16-Kc60", launcher="tn_bf16", M=64, Nc=60, n=64, lda=64, ldb=64, a_off=0, b_off=0),
    dict(id="tn_bf16-lda68", launcher="tn_bf16", M=64, Nc=64, n=64, lda=68, ldb=64, a_off=0, b_off=0),
    dict(id="tn_bf16-ldb66", launcher="tn_bf16", M=64, Nc=64, n=64, lda=64, ldb=66, a_off=0, b_off=0),
    dict(id="tn_bf16-A_misaligned", launcher="tn_bf16", M=64, Nc=64, n=64, lda=64, ldb=64, a_off=1, b_off=0),
    dict(id="tn_bf16-B_misaligned", launcher="tn_bf16", M=64, Nc=64, n=64, lda=64, ldb=64, a_off=0, b_off=4),
]


def elem_bytes(c) -> int:
    return 2 if c["launcher"] in ("bf16", "tn_bf16") else 4


def sliced_part_floats(probe, c) -> int:
    """The partial-block floats a sliced case passes: what the launcher asks for, or one float short of it."""
    need = probe.probe_gemm_rows_sliced_floats(c["n"], c["R"], c["Nc"])
    return max(need - 1, 0) if c.get("part") == "short" else need


def route_of(probe, c, a_ptr=None, b_ptr=None) -> str:
    """The route the launcher takes for case `c`, from the product's own predicates (device pointers or aligned stand-ins)."""
    a = a_ptr if a_ptr is not None else FAKE_BASE + c.get("a_off", 0) * elem_bytes(c)
    b = b_ptr if b_ptr is not None else FAKE_BASE
    L = c["launcher"]
    if L in ("rows", "f32_256"):
        use = c["R"] > 0 and probe.probe_gemm_rows_f32_256_usable(a, c["lda"], c["n"], b, c["ldb"], c["R"], c["Nc"])
        return "256" if (c["bt"] or L == "f32_256") and use else "128"
    if L == "sliced":
        need = probe.probe_gemm_rows_sliced_floats(c["n"], c["R"], c["Nc"])
        return "sliced" if need > 0 and sliced_part_floats(probe, c) >= need else "fallback"
    if L == "bf16":
        return "256" if probe.probe_gemm_rows_bf16_256_usable(a, c["lda"], c["n"], b, c["ldb"], c["R"], c["Nc"]) else "128"
    return "tn"
