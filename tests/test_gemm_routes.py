"""CPU-side checks of the matrix-product launchers through the test-only probe library (tests/native/libmot_probe.so):

  * route census: every case of the shape table (tests/gemm_cases.py) still takes the route it names according to the
    product's own predicates, and each launcher's cases reach both sides of its predicate -- when a threshold moves, this
    fails instead of tests/test_gpu_products.py quietly testing one route twice;
  * contract refusals: launch_gemm_rows_bf16 and launch_gemm_tn_bf16 return MOT_EUNSUPPORTED for shapes and pointers
    outside their contract before any HIP call, so stand-in addresses that are never dereferenced suffice here."""
import ctypes as C

import pytest

import gemm_cases as gc


@pytest.fixture(scope="module")
def probe():
    import mixture_of_tokenizers_amd  # noqa: F401  (loads libmot_hip.so first, as the GPU tests do)
    return gc.load_probe()


def test_probe_uses_the_product_library(probe):
    from mixture_of_tokenizers_amd import _capi
    with open("/proc/self/maps") as f:
        maps = f.read()
    libs = {line.split()[-1] for line in maps.splitlines() if line.endswith(".so") and "libmot_hip" in line}
    assert libs == {str(_capi.LIB_PATH.resolve())}, libs


def test_every_case_takes_its_route(probe):
    wrong = [(c["id"], c["route"], gc.route_of(probe, c)) for c in gc.CASES if gc.route_of(probe, c) != c["route"]]
    assert not wrong, f"cases whose route moved (id, named, now): {wrong}"


@pytest.mark.parametrize("launcher,routes", [("rows", {"256", "128"}), ("sliced", {"sliced", "fallback"}), ("bf16", {"256", "128"})])
def test_both_sides_of_each_predicate_are_covered(probe, launcher, routes):
    cases = [c for c in gc.CASES if c["launcher"] == launcher]
    assert {gc.route_of(probe, c) for c in cases} == routes
    if launcher == "sliced":   # the predicate itself on both sides too (0 floats: the shape gains nothing from slicing)
        assert {probe.probe_gemm_rows_sliced_floats(c["n"], c["R"], c["Nc"]) > 0 for c in cases} == {True, False}
    if launcher == "rows":     # the 256 kernel's predicate holds for some non-transposed cases, which still take the 128 kernel
        nt = [c for c in cases if not c["bt"]]
        assert {bool(probe.probe_gemm_rows_f32_256_usable(gc.FAKE_BASE, c["lda"], c["n"], gc.FAKE_BASE, c["ldb"], c["R"], c["Nc"])) for c in nt} == {True, False}


def test_direct_256_cases_are_inside_the_kernel_contract(probe):
    for c in gc.CASES:
        if c["launcher"] == "f32_256":
            assert gc.route_of(probe, c) == "256", c["id"]


@pytest.mark.parametrize("case", gc.REFUSALS, ids=lambda c: c["id"])
def test_contract_refusals_without_a_gpu(probe, case):
    from mixture_of_tokenizers_amd import _capi
    e = gc.elem_bytes(case)
    a, b, out = gc.FAKE_BASE + case["a_off"] * e, 2 * gc.FAKE_BASE + case["b_off"] * e, C.c_void_p(3 * gc.FAKE_BASE)
    if case["launcher"] == "bf16":
        rc = probe.probe_gemm_rows_bf16(a, case["lda"], case["n"], b, case["ldb"], case["R"], case["Nc"], out, case["Nc"], case["out_bf16"], None,
                                        case["acc"], None, None)
    else:
        rc = probe.probe_gemm_tn_bf16(a, case["lda"], case["M"], b, case["ldb"], case["Nc"], case["n"], out, case["Nc"], None)
    assert rc == gc.MOT_EUNSUPPORTED, _capi.lib.mot_last_error()
    assert b"gemm_" in _capi.lib.mot_last_error()
