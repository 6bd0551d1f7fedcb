// mot_headcore.hpp -- what the output heads (mot_head.hip: the 512-row byte head, mot_tokhead.hip: the token-level head,
// mot_plainhead.hip: the plain cross-entropy head) share: the factor of the row's closing rms-norm with its derivative (device
// inline), the chunk rule, and the launchers of mot_headcore.hip: the row chain for dx, the loss's fixed-order double sum (divided
// by a constant or by the plain head's device count of kept rows) and the evaluation's counts.
// Their products are launch_product_nt / _nn / _tn (mot_internal.hpp).
#pragma once
#include "mot_desc.hpp"   // up256, Arena: the heads' workspace carves

namespace mot {

constexpr float kHeadEps = 1.1920928955078125e-07f;   // F.rms_norm(eps=None): the fp32 opmath epsilon, bf16 inputs included
constexpr int kLossParts = 512;                       // doubles of the loss's partial sums in a head's workspace

// norm(h_L) = c x_row and dc/dm0, for n_layer_out identity layers h <- h + norm(h) = h (1 + r), r = (mean(h^2) + eps)^-1/2:
// each layer scales the row by (1 + r) and its mean square by (1 + r)^2; the derivative is carried forward alongside.
// L = 0 is the plain norm: c = (m0 + eps)^-1/2, dc = -c^3 / 2.
__device__ __forceinline__ void row_scale(float m0, int L, float eps, float &c, float &dc) {
    float m = m0, dm = 1.f;
    c = 1.f;
    dc = 0.f;
    for (int i = 0; i < L; ++i) {
        const float r = rsqrtf(m + eps), dr = -0.5f * r * r * r * dm, a = 1.f + r;
        dc = dc * a + c * dr;
        c *= a;
        dm = dm * a * a + 2.f * m * a * dr;
        m *= a * a;
    }
    const float r = rsqrtf(m + eps);
    dc = dc * r - 0.5f * c * r * r * r * dm;
    c *= r;
}

// (dc/dm0) / c of row_scale, for the row chain: the same recurrence on the logarithm of c, in double.  A row whose mean square lies
// far below eps (a zero row, a row of 2^-60) has r = eps^-1/2 in every layer, so dm grows by (1 + r)^2 = 8.4e6 a layer and dc/dm0
// (1e45 at L = 3) leaves fp32, while its product with x . u in the chain fits.  m0 > 0 keeps every term finite up to L = 64.
__device__ __forceinline__ double row_scale_dlog(double m0, int L, double eps) {
    double m = m0, dm = 1.0, q = 0.0;
    for (int i = 0; i < L; ++i) {
        const double r = 1.0 / sqrt(m + eps), dr = -0.5 * r * r * r * dm, a = 1.0 + r;
        q += dr / a;
        dm = dm * a * a + 2.0 * m * a * dr;
        m *= a * a;
    }
    return q - 0.5 * dm / (m + eps);
}

// The evaluation calls (mot_token_head_eval, mot_byte_head_eval): what a row pass writes per row, each pointer optional
struct HeadEvalRows {
    float *row_loss;
    int32_t *pred, *rank;
    HeadEvalRows at(int64_t first) const { return {row_loss ? row_loss + first : nullptr, pred ? pred + first : nullptr, rank ? rank + first : nullptr}; }
};

// the larger of two (logit, class) pairs, the lower class on equal logits: commutative and associative, so every order of a
// reduction ends at the same pair
__device__ __forceinline__ void argmax_take(float &v, int &i, float ov, int oi) {
    const bool take = ov > v || (ov == v && oi < i);
    v = take ? ov : v;
    i = take ? oi : i;
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ void argmax_dpp(float &v, int &i) {   // lanes outside ROW_MASK meet their own pair
    const float ov = dpp_move<CTRL, ROW_MASK>(v, v);
    const int oi = __builtin_amdgcn_update_dpp(i, i, CTRL, ROW_MASK, 0xf, false);
    argmax_take(v, i, ov, oi);
}
// the wave's pair, wave-uniform, on the DPP steps of wave_max (mot_tile.hpp)
__device__ __forceinline__ void wave_argmax(float &v, int &i) {
    argmax_dpp<kDppQuadXor1, 0xf>(v, i);
    argmax_dpp<kDppQuadXor2, 0xf>(v, i);
    argmax_dpp<kDppRowRor4, 0xf>(v, i);
    argmax_dpp<kDppRowRor8, 0xf>(v, i);
    argmax_dpp<kDppRowBcast15, 0xa>(v, i);
    argmax_dpp<kDppRowBcast31, 0xc>(v, i);
    v = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
    i = __builtin_amdgcn_readlane(i, 63);
}

// rows per chunk: the largest multiple of 256 rows of per_row_bytes of scratch under the budget, at least 256, never more than the rows
inline int64_t head_chunk_rows(int64_t budget_bytes, int64_t per_row_bytes, int64_t rows) {
    int64_t ch = budget_bytes / per_row_bytes / 256 * 256;
    if (ch < 256) ch = 256;
    return rows < ch ? rows : ch;
}

// the `dtype` argument of those products for T = float or __bf16
template <typename T> constexpr int head_dtype = sizeof(T) == 2 ? MOT_BF16 : MOT_F32;

// dx_r = u_r + (dc/dm0) (2 / K) (x_r . u_r / c_r) x_r over n rows with row_scale(L) (norm_in), else dx_r = u_r; float and __bf16
template <typename T>
int launch_head_chain(const T *x, const float *u, int K, int64_t n, int L, int norm_in, float eps, T *dx, hipStream_t stream);
// *loss = inv_m * (sum of term[0, rows)) in a fixed order in double; part: kLossParts doubles
int launch_head_loss(const float *term, int64_t rows, double *part, double inv_m, float *loss, hipStream_t stream);
// the out struct of an evaluation call, checked before any HIP call; `fn` starts the message
int head_eval_check(const char *fn, const MotHeadEvalOut *o);
// counts[0, n_counts) = {rows with a target in [0, vocab), those with pred == target, groups of `per` consecutive rows all of which
// are such} as integer sums per workgroup, then over the workgroups in order; part: the kLossParts doubles of the loss, free by then
int launch_head_eval_counts(const int32_t *pred, const int64_t *tgt, int64_t groups, int per, int vocab, void *part, int64_t *counts, int n_counts,
                            hipStream_t stream, int skip_dropped = 0, int64_t ignore = -1);
// the plain head's: skip_dropped = 1 takes a row with a target outside [0, vocab) or equal to `ignore` out of its group instead of
// failing the group, and a group without a counted row is not all-correct
// *kept = the number of targets in [0, vocab) other than `ignore`, an integer sum on the device; part: the kLossParts doubles
int launch_head_kept(const int64_t *tgt, int64_t rows, int vocab, int64_t ignore, void *part, long long *kept, hipStream_t stream);
// launch_head_loss with the divisor read on the device: *loss = (sum of term[0, rows)) / *kept, NaN at *kept == 0
int launch_head_loss_kept(const float *term, int64_t rows, double *part, const long long *kept, float *loss, hipStream_t stream);

}  // namespace mot
