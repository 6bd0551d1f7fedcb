// mot_lincore.hpp -- what the linear front-ends share (the composed CONCAT_LINEAR path of embed_mix: mot_linear.hip,
// mot_bwd_linear.hip; byte_fc_mix: mot_bytefc.hip; value_mix: mot_valuemix.hip): the row pass that finishes a forward in place, the
// norm's backward, and the pad statistics of the two id tensors.  Each kernel lives once, in mot_lincore.hip, behind the launcher
// declared here; `dtype` is MOT_F32 or MOT_BF16 and says what the void pointers hold.  The products of these front-ends are
// launch_product_nt / _nn / _tn (mot_internal.hpp).
#pragma once
#include "mot_internal.hpp"

namespace mot {

constexpr int kRowMaxDim = 2048;   // columns of a row a wave keeps in registers; longer rows take the scalar path

// In place on n rows of `dim` columns: y <- r y with r = rsqrt(mean(y^2) + eps), or y unchanged and r = 1 without `norm`; r goes to
// row_rnorm[row] unless that is null.  One wave per row, lane l owning the 16-byte chunks l, l + 64, ...; rows whose dim is no
// multiple of the chunk or whose base is not 16-byte aligned are walked element by element.
int launch_rows_finish(void *y, int64_t n, int dim, int norm, float eps, float *row_rnorm, int dtype, hipStream_t stream);
// The same pass with the token row added first: s = tok_table[tokens[row]] + y (bf16: rounded to bf16 before the squares are taken),
// y <- r s.  A token id outside [0, tok_rows) reads row 0 and raises kStatusTokenOor in *status (unless null).
int launch_rows_finish_tok(void *y, const int32_t *tokens, const void *tok_table, int64_t tok_rows, int64_t n, int dim, int norm, float eps,
                           float *row_rnorm, uint32_t *status, int dtype, hipStream_t stream);

// Back through that norm from the saved output x and factors rnorm: dy = r (g - x mean(g x)), or dy = g without `norm` (x and rnorm
// are then not read).  g and x are contiguous [n][dim] in `dtype`; the result goes to dy (in `dtype`, row stride ld) and to dy32
// (fp32, row stride ld32), either of which may be null.
int launch_rows_norm_bwd(const void *g, const void *x, const float *rnorm, int64_t n, int dim, int norm, void *dy, int64_t ld, float *dy32, int64_t ld32,
                         int dtype, hipStream_t stream);

// counters[0] += n_tokens, [1] += n_slots and, with `padded` given, [2] += the slots of padded that hold `pad`, [3] += those of
// `after` (the ids after the pull).
int launch_count_pads(const int64_t *padded, const int64_t *after, int64_t n_slots, int64_t pad, int64_t n_tokens, int64_t *counters, hipStream_t stream);

}  // namespace mot
