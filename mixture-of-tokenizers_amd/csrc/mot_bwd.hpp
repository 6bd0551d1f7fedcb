// mot_bwd.hpp -- what the three units of the front-end backward share: mot_backward.hip (the table-gradient scatter, SUM / NOOP /
// CONCAT and the entry launch_embed_mix_bwd), mot_bwd_linear.hip (CONCAT_LINEAR) and mot_bwd_mean.hip (MEAN).  The two
// latter compute their dense parts and hand the table gradients to the scatter through run_scatter().  One unit outside the
// front-end backward includes it: mot_bytefc.hip, whose gradient rows [ds | du] are the split rows of the CONCAT_LINEAR scatter.
#pragma once
#include "mot_mix.hpp"

namespace mot {

// MOT_MIX_CONCAT (x = norm(cat(a, b_*)), runs/711_*.py:224-232) shares the split row layout [token part | byte part] of the
// CONCAT_LINEAR scatter (there the row is du = dy.W) and, like SUM, carries its own output norm: the row IS the mixed row.
constexpr bool split_row(int mode) { return mode == MOT_MIX_CONCAT_LINEAR || mode == MOT_MIX_CONCAT; }
constexpr bool mixes_bytes(int mode) { return mode == MOT_MIX_SUM || mode == MOT_MIX_CONCAT; }   // the byte rows are part of the normed row

struct BwdArgs {
    const int32_t *tokens;
    int64_t n_tokens;
    int bpt;
    const int64_t *ids_a, *ids_b;
    const float *tok_table;
    int64_t tok_rows;
    int D;
    const float *byte_table;
    int64_t byte_rows;
    int Db;
    int norm_tok, norm_byte, norm_out;
    float eps;
    const float *scale_tok, *scale_byte;
    const float *byte_rnorm;
    const float *grad_out;
    float *d_tok, *d_byte, *d_scale_tok, *d_scale_byte;
    uint32_t *status;
    // layout of one gradient row of D elements: token part [tok_lo, tok_lo+Dt), byte part [byte_lo, byte_lo+bpt*Db).
    // SUM: both parts span the whole row (x = a + concat b); CONCAT_LINEAR: they are the two halves of du = dy.W
    int Dt, tok_lo, byte_lo, nbk;
    // byte-table gradient privatised in LDS as 64-bit fixed point: rows [0, priv_lo) and [priv_hi0, byte_rows) have a slot
    // (everything when the table fits; otherwise the raw byte values and the trailing specials such as pad / eot)
    int priv_lo, priv_hi0, priv_rows;
    const int32_t *pos_sorted;  // token positions ordered by token id
    const int32_t *tok_sorted;  // their (clamped) token ids
    int in_bf16;  // tables and grad_out are bf16 (gradients are accumulated and returned in fp32 either way)
    // lane-contiguous kernel only (the two halves of the CONCAT_LINEAR scatter): elements between gradient rows when they are columns of
    // a wider matrix (0: D), and "no token table" (SUM over byte slots only: nothing is read from or added to a token table)
    int g_ld, no_tok;
    int slot0;    // first byte slot of this pass (its ids are ids[n * bpt + slot0 + ...]): the byte part taken in column blocks
    int abl;  // dev-only timing ablations (MOT_DEV_ABLATION builds): 1 no LDS byte adds, 2 no token-row flush, 4 no wave sums
};

// mot_backward.hip: the scatter stage
void fill_bwd_args(BwdArgs &A, const MotEmbedMixDesc &d, const MotEmbedMixGrads &gr);
size_t scatter_ws_ints(const MotEmbedMixDesc &d);   // int32 words of run_scatter's `ws_ints`
// sorts the positions by token id (unless A brings the order) and scatters with the kernel that fits A's row layout;
// mode: MOT_MIX_NOOP, SUM, CONCAT_LINEAR or CONCAT
int run_scatter(int mode, BwdArgs &A, const MotEmbedMixDesc &d, int32_t *ws_ints, float *rnorm_ws, hipStream_t stream);
bool lc_layout(int mode, const BwdArgs &A);   // rows the lane-contiguous kernel takes (mode: MOT_MIX_NOOP or SUM)
// mot_bwd_linear.hip
size_t embed_mix_bwd_linear_workspace_bytes(const MotEmbedMixDesc &d);
int launch_embed_mix_bwd_linear(const MotEmbedMixDesc &d, const MotEmbedMixGrads &gr, hipStream_t stream, const void *w16 = nullptr,
                                char *ws16 = nullptr, const void *g16 = nullptr, const void *x16 = nullptr, const MotEmbedMixDesc *d16 = nullptr);
// mot_bwd_mean.hip
size_t embed_mix_bwd_mean_workspace_bytes(const MotEmbedMixDesc &d);
int launch_embed_mix_bwd_mean(const MotEmbedMixDesc &d, const MotEmbedMixGrads &gr, hipStream_t stream);

}  // namespace mot
