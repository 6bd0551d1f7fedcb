// mot_internal.hpp -- host-side declarations shared by the translation units of libmot_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "../../include/mot.h"

namespace mot {

// Records a thread-local message for mot_last_error() and returns `code`.
int set_error(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
// hipGetLastError() after a launch -> MOT_OK / MOT_EHIP (with the kernel name in the message).
int check_launch(const char *what);

// Raises a kernel's dynamic-LDS limit to 160 KiB once per (kernel, device): `done` is that kernel's per-device bit set
// (a function-local static std::atomic at the call site).  hipFuncSetAttribute is idempotent, so a race costs a second call.
int ensure_max_dyn_lds(const void *kernel, std::atomic<uint64_t> &done, const char *name);

int pick_tile_tokens(int64_t n_rows, int64_t tokens_per_row, int bpt, bool with_ids);

int launch_tokens_to_bytes(const int32_t *tokens, int64_t n_tokens, const void *ttb, int elem, int64_t ttb_rows,
                           int bpt, int64_t *out, uint32_t *status, hipStream_t stream);
int launch_pull_bytes(const int64_t *in, int64_t *out, int64_t B, int64_t tokens_per_row, int bpt, int64_t pad,
                      int64_t eot, int dir, hipStream_t stream);
int launch_create_batch(const int32_t *tokens, int64_t B, int64_t T, const void *ttb_left, const void *ttb_right,
                        int elem, int64_t ttb_rows, int bpt, int32_t pad, int32_t eot, int64_t *out, uint32_t *status,
                        hipStream_t stream);
int launch_char_matrix(const int32_t *codes, const int64_t *tok_off, const int64_t *seq_off, int64_t n_seqs, int64_t seq_len, int max_char,
                       int32_t leading_space, int32_t bos_id, int32_t eos_id, int64_t *out, hipStream_t stream);
int launch_gather_rows(const void *ids_a, const void *ids_b, int ids_elem, int64_t n, const void *table, int64_t rows,
                       int dim, int rms_norm, float eps, const float *scale, void *out, uint32_t *status, int dtype,
                       hipStream_t stream);
// the same gather with row r written at out + (r / group) * out_ld + (r % group) * dim, and the status bit to raise
int launch_gather_rows_placed(const void *ids_a, const void *ids_b, int ids_elem, int64_t n, const void *table, int64_t rows,
                              int dim, int rms_norm, float eps, const float *scale, void *out, int group, int64_t out_ld,
                              uint32_t *status, uint32_t oor_flag, int dtype, hipStream_t stream);
int launch_rows_rnorm(const void *table, int64_t rows, int dim, float eps, float *out, int dtype, hipStream_t stream);
// the concat operand [n, K] of the concat + linear mixin in one kernel (one id tensor, Dt and Db multiples of the 16-byte vector)
int launch_concat_rows(const int32_t *tokens, const int64_t *ids, int64_t n, const void *tok_table, int64_t tok_rows, int Dt, const void *byte_table,
                       int64_t byte_rows, int Db, int bpt, int norm_tok, const float *byte_rnorm, float eps, void *u, int K, int tok_lo, int byte_lo,
                       uint32_t *status, int dtype, hipStream_t stream);
size_t embed_mix_workspace_bytes(const MotEmbedMixDesc &d);
int launch_embed_mix(const MotEmbedMixDesc &d, hipStream_t stream, __bf16 *add16 = nullptr, bool add_out = false);   // SUM / MEAN / NOOP (MixArgs.add16 / add_out)
bool embed_mix_mean_takes_add16(const MotEmbedMixDesc &d);
int launch_embed_mix_linear(const MotEmbedMixDesc &d, hipStream_t stream);  // CONCAT_LINEAR
int launch_embed_mix_linear_ex(const MotEmbedMixDesc &d, const float *wt_prebuilt, int wt_cols, hipStream_t stream);
size_t embed_mix_linear_workspace_bytes(const MotEmbedMixDesc &d);
size_t embed_mix_linear_bf16_workspace_bytes(const MotEmbedMixDesc &d);
int launch_embed_mix_linear_bf16(const MotEmbedMixDesc &d, hipStream_t stream);
// the front-end backward, every mode (mot_backward.hip; CONCAT_LINEAR and MEAN continue in mot_bwd_linear.hip / mot_bwd_mean.hip)
size_t embed_mix_bwd_workspace_bytes(const MotEmbedMixDesc &d);
int launch_embed_mix_bwd(const MotEmbedMixDesc &d, const MotEmbedMixGrads &g, hipStream_t stream);
// the shared fp32 matrix products (mot_gemm_f32.hip)
// C[j][k] += sum_n A[n][j] * B[n][k]  (A: n x M, B: n x Nc; fp32 MFMA, atomic accumulate)
int launch_gemm_tn(const float *A, int lda, int M, const float *B, int ldb, int Nc, int64_t n, float *C, int ldc, hipStream_t stream);
// C[n][c] = sum_r A[n][r] * (b_transposed ? B[c][r] : B[r][c]) (+ bias[c]), fp32 MFMA, plain stores
int launch_gemm_rows(const float *A, int lda, int64_t n, const float *B, int ldb, int R, int Nc, float *C, int ldc, bool b_transposed, hipStream_t stream,
                     const float *bias = nullptr, bool accumulate = false);
// the same product for FEW rows (a 458-row byte table, 132 character rows) over a long reduction: the reduction is cut into slices,
// one workgroup per (output block, slice), whose partial blocks go to `part` (gemm_rows_sliced_floats(n, R, Nc) floats, 0 = the shape
// gains nothing) and are summed in slice order by a second kernel -- the same bits on every run.  Falls back to launch_gemm_rows.
size_t gemm_rows_sliced_floats(int64_t n, int R, int Nc);
int launch_gemm_rows_sliced(const float *A, int lda, int64_t n, const float *B, int ldb, int R, int Nc, float *C, int ldc, bool b_transposed, float *part,
                            size_t part_floats, hipStream_t stream);
// the composed concat + linear forward (index kernels, seam gather, dense MFMA kernel, row norm), fp32 and bf16 (mot_linear.hip)
bool embed_mix_linear_is_composed(const MotEmbedMixDesc &d);
size_t embed_mix_linear_composed_workspace_bytes(const MotEmbedMixDesc &d);
int launch_embed_mix_linear_composed(const MotEmbedMixDesc &d, hipStream_t stream);
// C[n][c] = sum_r A[n][r] * B[c][r] (+ bias[c]) for bf16 A, B (and bias), fp32 accumulation, C bf16 or fp32
// mot_concat16.hip: gather + contraction + bias + output norm of the bf16 concat + linear mixin in one kernel
bool concat16_usable(const MotEmbedMixDesc &d);
bool concat16_norm_in_kernel(const MotEmbedMixDesc &d);   // the byte rows' rms factors need no table from the caller
bool concat16_residual_usable(const MotEmbedMixDesc &d);   // the residual form: the token row (tok_dim == model_dim) added behind the product of the byte part
int launch_concat16(const MotEmbedMixDesc &d, const int32_t *tokens, const int64_t *ids, const uint16_t *ids16, int64_t n, const float *rn_byte,
                    void *out, float *row_rnorm, hipStream_t stream, bool residual = false);
int launch_wave_ids16(const MotEmbedMixDesc &d, uint16_t *ids16, hipStream_t stream);   // ids from the token->byte table, 16-bit, + parity outputs
int launch_gemm_rows_bf16(const void *A, int lda, int64_t n, const void *B, int ldb, int R, int Nc, void *C, int ldc, bool out_bf16,
                          const void *bias, hipStream_t stream, bool accumulate = false, const float *addend = nullptr);   // addend: fp32 [n][ldc] added before the store
bool gemm_rows_bf16_256_usable(const void *A, int lda, int64_t n, const void *B, int ldb, int R, int Nc);   // the launcher's 256 x 256 route
// the 256 x 256 LDS-DMA kernel of mot_gemm_bf16.hip with fp32 operands (B transposed: B[c][r])
bool gemm_rows_f32_256_usable(const float *A, int lda, int64_t n, const float *B, int ldb, int R, int Nc);
int launch_gemm_rows_f32_256(const float *A, int lda, int64_t n, const float *B, int ldb, int R, int Nc, float *C, int ldc, const float *bias, bool accumulate,
                             hipStream_t stream);
// C[m][k] += sum_n A[n][m] * B[n][k]  (bf16 row-major operands, fp32 atomics into C; mot_gemm_bf16.hip); lda / ldb / M / Kc multiples of 8
int launch_gemm_tn_bf16(const __bf16 *A, int lda, int M, const __bf16 *B, int ldb, int Kc, int64_t rows, float *C, int ldc, hipStream_t stream);
// The three products of a linear layer over n rows, on the fp32 or the bf16 launcher above by `dtype` (what A and B hold).
// None says __restrict__: the heads' G aliases their S.
// C[n][c] = sum_r A[n][r] B[c][r] (+ bias[c]; += with accumulate).  C is fp32, or bf16 from bf16 operands when out_bf16.
inline int launch_product_nt(int dtype, const void *A, int lda, int64_t n, const void *B, int ldb, int R, int Nc, void *C, int ldc, bool out_bf16,
                             const void *bias, bool accumulate, hipStream_t stream) {
    if (dtype == MOT_BF16) return launch_gemm_rows_bf16(A, lda, n, B, ldb, R, Nc, C, ldc, out_bf16, bias, stream, accumulate);
    return launch_gemm_rows((const float *)A, lda, n, (const float *)B, ldb, R, Nc, (float *)C, ldc, true, stream, (const float *)bias, accumulate);
}
// C[n][c] = sum_r A[n][r] B[r][c] into fp32.  fp32 takes B [R][ldb] itself, bf16 its k-major copy [Nc][ldb].
inline int launch_product_nn(int dtype, const void *A, int lda, int64_t n, const void *B_or_BT, int ldb, int R, int Nc, float *C, int ldc,
                             hipStream_t stream) {
    if (dtype == MOT_BF16) return launch_gemm_rows_bf16(A, lda, n, B_or_BT, ldb, R, Nc, C, ldc, false, nullptr, stream);
    return launch_gemm_rows((const float *)A, lda, n, (const float *)B_or_BT, ldb, R, Nc, C, ldc, false, stream);
}
// C[m][c] += sum_n A[n][m] B[n][c] into fp32 (atomics)
inline int launch_product_tn(int dtype, const void *A, int lda, int M, const void *B, int ldb, int Nc, int64_t n, float *C, int ldc, hipStream_t stream) {
    if (dtype == MOT_BF16) return launch_gemm_tn_bf16((const __bf16 *)A, lda, M, (const __bf16 *)B, ldb, Nc, n, C, ldc, stream);
    return launch_gemm_tn((const float *)A, lda, M, (const float *)B, ldb, Nc, n, C, ldc, stream);
}
int launch_transpose_f32(const float *src, int rows, int cols, float *dst, hipStream_t stream);                        // dst[c][r] = src[r][c]  (mot_gemm_f32.hip)
// conversions between the fp32 and bf16 sides (mot_convert.hip)
int launch_widen(const void *src_bf16, size_t n, float *dst, hipStream_t stream);                                    // dst[i] = float(src[i])
int launch_narrow(const float *src, int64_t n, void *dst_bf16, hipStream_t stream);                                  // dst[i] = bf16(src[i])
int launch_transpose_bf16(const void *src_bf16, int rows, int cols, void *dst_bf16, hipStream_t stream);             // dst[c][r] = src[r][c]
int launch_narrow_transpose(const float *src, int rows, int cols, void *dst_bf16, hipStream_t stream);               // dst[c][r] = bf16(src[r][c])
// counting sort of positions 0..n-1 by ids[position] (mot_group.hip); ws_ints: group_positions_ws_ints(n, rows) int32
size_t group_positions_ws_ints(int64_t n, int64_t rows);
int launch_group_positions(const int32_t *ids, int64_t n, int64_t rows, int32_t *ws_ints, const int32_t **pos_sorted, const int32_t **id_sorted,
                           uint32_t *status, hipStream_t stream);
// what launch_group_positions leaves in its buffer, which is also what mot_token_order hands out:
// [counts: rows][starts: rows][rank: n][pos_sorted: n][id_sorted: n].  Groups are complete; the order inside a group is the sort's own.
struct GroupedPositions { const int32_t *counts, *starts, *pos_sorted, *id_sorted; };
inline GroupedPositions grouped_positions_view(const int32_t *ws_ints, int64_t n, int64_t rows) {
    return {ws_ints, ws_ints + rows, ws_ints + 2 * rows + n, ws_ints + 2 * rows + 2 * n};
}
// zero n 32-bit words with a kernel (not hipMemsetAsync: a memset node aborts on graph replay with this runtime; mot_group.hip)
int launch_zero_words(void *p, int64_t n_words, hipStream_t stream);
size_t cross_attn_bwd_workspace_bytes(const MotCrossAttnDesc &d);
int launch_cross_attn_bwd(const MotCrossAttnDesc &d, const MotCrossAttnGrads &g, hipStream_t stream);
size_t char_swa_workspace_bytes(const MotCharSwaDesc &d);
int launch_char_swa(const MotCharSwaDesc &d, hipStream_t stream);
// one decode step of the character mixer (mot_swa_step.hip): its own validation, every refusal before any HIP call
size_t char_swa_step_workspace_bytes(const MotCharSwaStepDesc *d);   // 0 for a descriptor the call would refuse
int launch_char_swa_step(const MotCharSwaStepDesc *d, hipStream_t stream);
// the feed-forward behind that step (mot_ffn_step.hip): likewise
size_t ffn_step_workspace_bytes(const MotFfnStepDesc *d);   // 0 for a descriptor the call would refuse
int launch_ffn_step(const MotFfnStepDesc *d, hipStream_t stream);
size_t cross_attn_workspace_bytes(const MotCrossAttnDesc &d);
int launch_cross_attn(const MotCrossAttnDesc &d, hipStream_t stream);
// the byte output head (mot_head.hip): validation before any HIP call, then the launches
int byte_head_check(const MotByteHeadDesc *d);
size_t byte_head_workspace_bytes(const MotByteHeadDesc &d);
int launch_byte_head_fwd(const MotByteHeadDesc &d, hipStream_t stream);
int launch_byte_head_bwd(const MotByteHeadDesc &d, const float *grad_loss, void *dx, float *dW, hipStream_t stream);
int launch_byte_head_eval(const MotByteHeadDesc *d, const MotHeadEvalOut *out, hipStream_t stream);   // its own validation, every refusal before any HIP call
// the split-mode training step in one call (mot_headstep.hip): its own validation, every refusal before any HIP call
size_t byte_head_step_workspace_bytes(const MotByteHeadDesc *d);   // 0 for a descriptor the call would refuse
int launch_byte_head_step(const MotByteHeadDesc *d, void *dx, float *dW, hipStream_t stream);
// the token-level output head (mot_tokhead.hip): validation before any HIP call, then the launches of loss, dx and dW
int token_head_check(const MotTokenHeadDesc *d);
size_t token_head_workspace_bytes(const MotTokenHeadDesc &d);
int launch_token_head_fwd(const MotTokenHeadDesc &d, hipStream_t stream);
int launch_token_head_eval(const MotTokenHeadDesc *d, const MotHeadEvalOut *out, hipStream_t stream);   // likewise
// the plain cross-entropy head (mot_plainhead.hip): its own validation, every refusal before any HIP call
size_t plain_head_workspace_bytes(const MotPlainHeadDesc *d);   // 0 for a descriptor the call would refuse
int launch_plain_head_fwd(const MotPlainHeadDesc *d, hipStream_t stream);
int launch_plain_head_eval(const MotPlainHeadDesc *d, const MotHeadEvalOut *out, hipStream_t stream);
size_t plain_head_compact_workspace_bytes(const MotPlainHeadDesc *d, const MotPlainHeadCompact *c);   // 0 for what the calls would refuse
int launch_plain_head_compact_fwd(const MotPlainHeadDesc *d, const MotPlainHeadCompact *c, hipStream_t stream);
int launch_plain_head_compact_eval(const MotPlainHeadDesc *d, const MotPlainHeadCompact *c, const MotHeadEvalOut *out, hipStream_t stream);
// the generation step (mot_nexttoken.hip): its own validation, every refusal before any HIP call
size_t next_token_workspace_bytes(const MotNextTokenDesc *d);   // 0 for a descriptor the call would refuse
int launch_next_token(const MotNextTokenDesc *d, hipStream_t stream);
// byte self-attention of the concat mixin (mot_bsa.hip); the descriptor is validated in mot_capi.hip
size_t byte_self_attn_saved_bytes(const MotByteSelfAttnDesc &d);
size_t byte_self_attn_workspace_bytes(const MotByteSelfAttnDesc &d);
int launch_byte_self_attn_fwd(const MotByteSelfAttnDesc &d, hipStream_t stream);
int launch_byte_self_attn_bwd(const MotByteSelfAttnDesc &d, const MotByteSelfAttnGrads &g, hipStream_t stream);
// the linear-on-bytes mixin (mot_bytefc.hip): validation before any HIP call (g: backward only), then the launches
int byte_fc_check(const MotByteFcMixDesc *d, const MotByteFcMixGrads *g, bool backward);
size_t byte_fc_mix_workspace_bytes(const MotByteFcMixDesc *d);       // 0 for a descriptor the call would refuse
size_t byte_fc_mix_bwd_workspace_bytes(const MotByteFcMixDesc *d);   // likewise
int launch_byte_fc_mix_fwd(const MotByteFcMixDesc &d, hipStream_t stream);
int launch_byte_fc_mix_bwd(const MotByteFcMixDesc &d, const MotByteFcMixGrads &g, hipStream_t stream);
// the bytes-only front-end and the byte value embeddings (mot_bytecat.hip): validation before any HIP call (g: backward only), then the launches
int byte_cat_check(const MotByteCatDesc *d, const MotByteCatGrads *g, bool backward);
size_t byte_cat_workspace_bytes(const MotByteCatDesc *d);       // 0: the forward needs none
size_t byte_cat_bwd_workspace_bytes(const MotByteCatDesc *d);   // 0 for a descriptor the call would refuse
int launch_byte_cat_fwd(const MotByteCatDesc &d, hipStream_t stream);
int launch_byte_cat_bwd(const MotByteCatDesc &d, const MotByteCatGrads &g, hipStream_t stream);
// token value embeddings (mot_values.hip): validation before any HIP call (g: backward only), then the launches
int value_embeds_check(const MotValueEmbedsDesc *d, const MotValueEmbedsGrads *g, bool backward);
size_t value_embeds_bwd_workspace_bytes(const MotValueEmbedsDesc *d);   // 0 for a descriptor the call would refuse
int launch_value_embeds_fwd(const MotValueEmbedsDesc &d, hipStream_t stream);
int launch_value_embeds_bwd(const MotValueEmbedsDesc &d, const MotValueEmbedsGrads &g, hipStream_t stream);
// one table's gradient from fp32 rows with a row stride, written once in `dtype` (mot_values.hip: the value embeddings' order, canon,
// slices and rows kernels).  ws: token_sums_ws_bytes; prepare = false reuses the order and canon an earlier call left there
size_t token_sums_ws_bytes(int64_t n, int64_t rows, int dim, int dtype);
int launch_token_sums_f32(const int32_t *tokens, int64_t n, int64_t rows, int dim, int dtype, const float *g, int g_ld, void *d_table,
                          const int32_t *order, bool prepare, char *ws, uint32_t *status, hipStream_t stream);
// the two ends of those sums for a unit that forms the slice sums itself (mot_once.hip), over the same workspace: the order (unless
// the caller brings one) and the canonical positions, then the closing rows kernel over the pieces at V.part ([slice][head, tail][dim])
struct TokenSumsView { const int32_t *counts, *starts, *pos_sorted, *id_sorted; int32_t *canon; float *part; };
int launch_token_canon(const int32_t *tokens, int64_t n, int64_t rows, int dim, int dtype, const int32_t *order, char *ws, uint32_t *status,
                       hipStream_t stream, TokenSumsView *V);
int launch_token_rows_close(const TokenSumsView &V, int64_t n, int64_t rows, int dim, int dtype, void *d_table, hipStream_t stream);
// the write-once backward of the fused front-end (mot_once.hip): validation before any HIP call, then the launches
int embed_mix_bwd_once_check(const MotEmbedMixDesc *d, const MotEmbedMixGradsOnce *g);
size_t embed_mix_bwd_once_workspace_bytes(const MotEmbedMixDesc *d);   // 0 for a descriptor the call would refuse
int launch_embed_mix_bwd_once(const MotEmbedMixDesc &d, const MotEmbedMixGradsOnce &g, hipStream_t stream);
// mixture-of-tokenizers value embeddings (mot_valuemix.hip): validation before any HIP call (g: backward only), then the launches
int value_mix_check(const MotValueMixDesc *d, const MotValueMixGrads *g, bool backward);
size_t value_mix_workspace_bytes(const MotValueMixDesc *d, bool backward);   // 0 for a descriptor the call would refuse
int launch_value_mix_fwd(const MotValueMixDesc &d, hipStream_t stream);
int launch_value_mix_bwd(const MotValueMixDesc &d, const MotValueMixGrads &g, hipStream_t stream);
// the three input streams of run 71081 (mot_splitx0.hip): validation before any HIP call (g: backward only), then the launches
int split_x0_check(const MotSplitX0Desc *d, const MotSplitX0Grads *g, bool backward);
size_t split_x0_workspace_bytes(const MotSplitX0Desc *d, bool backward);   // 0 for a descriptor refused on its shape (the query sees no pointers)
int launch_split_x0_fwd(const MotSplitX0Desc &d, hipStream_t stream);
int launch_split_x0_bwd(const MotSplitX0Desc &d, const MotSplitX0Grads &g, hipStream_t stream);
// the gather-GEMM of mot_concat16.hip for up to four (token table, byte table, W, out) sets over one token and id stream in ONE launch
struct Concat16Slots { int n; const void *tok_table[4], *byte_table[4], *weight[4]; void *out[4]; float *row_rnorm[4]; };
int launch_concat16_slots(const MotEmbedMixDesc &d, const Concat16Slots &S, const int32_t *tokens, const int64_t *ids, int64_t n, hipStream_t stream);

}  // namespace mot
