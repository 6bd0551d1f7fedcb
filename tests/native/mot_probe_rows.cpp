// mot_probe_rows.cpp -- more test-only C entry points of libmot_probe.so (see mot_probe.cpp): the row passes and the pad count the
// linear front-ends share (csrc/mot_lincore.hpp; tests/test_gpu_rowpass.py).  Each wrapper forwards its arguments unchanged and
// returns the launcher's status; device pointers arrive as they are.
#include "../../mixture-of-tokenizers_amd/csrc/mot_lincore.hpp"

extern "C" {

int probe_rows_finish(void *y, int64_t n, int dim, int norm, float eps, float *row_rnorm, int dtype, void *stream) {
    return mot::launch_rows_finish(y, n, dim, norm, eps, row_rnorm, dtype, (hipStream_t)stream);
}

int probe_rows_finish_tok(void *y, const int32_t *tokens, const void *tok_table, int64_t tok_rows, int64_t n, int dim, int norm, float eps, float *row_rnorm,
                          uint32_t *status, int dtype, void *stream) {
    return mot::launch_rows_finish_tok(y, tokens, tok_table, tok_rows, n, dim, norm, eps, row_rnorm, status, dtype, (hipStream_t)stream);
}

int probe_rows_norm_bwd(const void *g, const void *x, const float *rnorm, int64_t n, int dim, int norm, void *dy, int64_t ld, float *dy32, int64_t ld32,
                        int dtype, void *stream) {
    return mot::launch_rows_norm_bwd(g, x, rnorm, n, dim, norm, dy, ld, dy32, ld32, dtype, (hipStream_t)stream);
}

int probe_count_pads(const int64_t *padded, const int64_t *after, int64_t n_slots, int64_t pad, int64_t n_tokens, int64_t *counters, void *stream) {
    return mot::launch_count_pads(padded, after, n_slots, pad, n_tokens, counters, (hipStream_t)stream);
}

}  // extern "C"
