// mot_probe.cpp -- test-only C entry points to the shared matrix-product launchers of libmot_hip.so and their route predicates
// (tests/test_gpu_products.py, tests/test_gemm_routes.py).  Each wrapper forwards its arguments unchanged and returns the
// launcher's status; device pointers arrive as void *.  The product never loads this library: include/mot.h does not declare it.
#include "../../mixture-of-tokenizers_amd/csrc/mot_internal.hpp"

extern "C" {

int probe_gemm_rows(const void *A, int lda, int64_t n, const void *B, int ldb, int R, int Nc, void *C, int ldc, int b_transposed, const void *bias,
                    int accumulate, void *stream) {
    return mot::launch_gemm_rows((const float *)A, lda, n, (const float *)B, ldb, R, Nc, (float *)C, ldc, b_transposed != 0, (hipStream_t)stream,
                                 (const float *)bias, accumulate != 0);
}

int probe_gemm_rows_sliced(const void *A, int lda, int64_t n, const void *B, int ldb, int R, int Nc, void *C, int ldc, int b_transposed, void *part,
                           size_t part_floats, void *stream) {
    return mot::launch_gemm_rows_sliced((const float *)A, lda, n, (const float *)B, ldb, R, Nc, (float *)C, ldc, b_transposed != 0, (float *)part,
                                        part_floats, (hipStream_t)stream);
}

int probe_gemm_rows_f32_256(const void *A, int lda, int64_t n, const void *B, int ldb, int R, int Nc, void *C, int ldc, const void *bias, int accumulate,
                            void *stream) {
    return mot::launch_gemm_rows_f32_256((const float *)A, lda, n, (const float *)B, ldb, R, Nc, (float *)C, ldc, (const float *)bias, accumulate != 0,
                                         (hipStream_t)stream);
}

int probe_gemm_rows_bf16(const void *A, int lda, int64_t n, const void *B, int ldb, int R, int Nc, void *C, int ldc, int out_bf16, const void *bias,
                         int accumulate, const void *addend, void *stream) {
    return mot::launch_gemm_rows_bf16(A, lda, n, B, ldb, R, Nc, C, ldc, out_bf16 != 0, bias, (hipStream_t)stream, accumulate != 0, (const float *)addend);
}

int probe_gemm_tn(const void *A, int lda, int M, const void *B, int ldb, int Nc, int64_t n, void *C, int ldc, void *stream) {
    return mot::launch_gemm_tn((const float *)A, lda, M, (const float *)B, ldb, Nc, n, (float *)C, ldc, (hipStream_t)stream);
}

int probe_gemm_tn_bf16(const void *A, int lda, int M, const void *B, int ldb, int Kc, int64_t rows, void *C, int ldc, void *stream) {
    return mot::launch_gemm_tn_bf16((const __bf16 *)A, lda, M, (const __bf16 *)B, ldb, Kc, rows, (float *)C, ldc, (hipStream_t)stream);
}

int probe_gemm_rows_f32_256_usable(const void *A, int lda, int64_t n, const void *B, int ldb, int R, int Nc) {
    return mot::gemm_rows_f32_256_usable((const float *)A, lda, n, (const float *)B, ldb, R, Nc);
}

int probe_gemm_rows_bf16_256_usable(const void *A, int lda, int64_t n, const void *B, int ldb, int R, int Nc) {
    return mot::gemm_rows_bf16_256_usable(A, lda, n, B, ldb, R, Nc);
}

size_t probe_gemm_rows_sliced_floats(int64_t n, int R, int Nc) { return mot::gemm_rows_sliced_floats(n, R, Nc); }

}  // extern "C"
