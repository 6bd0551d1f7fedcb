// mot_bwd_linear.hip -- backward of the CONCAT_LINEAR mixin (x = rms_norm?(W.cat(a, b_*) + bias)): dy by the shared norm backward
// (mot_lincore.hip), dbias, dW and du as dense products (mot_gemm_f32.hip, mot_gemm_bf16.hip; bf16 operands widened or narrowed by mot_convert.hip), then the table gradients
// from du through the scatter stage of mot_backward.hip (run_scatter, mot_bwd.hpp).  Called by launch_embed_mix_bwd only.
#include <stdlib.h>

#include "mot_bwd.hpp"
#include "mot_lincore.hpp"

namespace mot {

// ==========================================================================================
// CONCAT_LINEAR backward:  x = rms_norm?(y), y = W u + bias, u = cat(a, b_*)
//   dy = r_y (g - x mean(g x))                      launch_rows_norm_bwd (mot_lincore.hip; fp32, or bf16 from bf16 g and x)
//   du = dy . W          (N x Dm) @ (Dm x K)        the forward MFMA kernel with dy as dense "token rows";
//                                                   W in nn.Linear layout IS the k-major operand it wants
//   dW += dy^T . u       (Dm x N) @ (N x K)         gemm_tn_kernel: split over tokens, fp32 MFMA, atomic accumulate;
//                                                   u = the seam tensors (gather_rows with the norms/scales applied)
//   dbias += colsum(dy)                             colsum_kernel
//   table gradients: the scatter stage (run_scatter) on du (row layout = the concat layout)
// ==========================================================================================
__global__ __launch_bounds__(kThreads) void colsum_kernel(const float *__restrict__ a, int64_t n, int cols, float *__restrict__ out) {
    // each workgroup sums a strip of rows for every column, then one atomic per column
    const int64_t rows_per = (n + gridDim.x - 1) / gridDim.x, lo = blockIdx.x * rows_per, hi = min(n, lo + rows_per);
    for (int c = threadIdx.x; c < cols; c += kThreads) {
        float s = 0.f;
        for (int64_t r = lo; r < hi; ++r) s += a[r * cols + c];
        if (lo < hi) atomicAdd(out + c, s);
    }
}

__global__ __launch_bounds__(kThreads) void iota_kernel(int32_t *p, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) p[i] = (int32_t)i;
}

// out[n] = ids[n * bpt + k] as int32 (out-of-range ids flagged and clamped to 0, as the forward does): one byte slot's ids as the
// "tokens" of a plain embedding backward (the slot-wise scatter of wide concat rows, below)
__global__ __launch_bounds__(kThreads) void ids_column_i32_kernel(const int64_t *__restrict__ ids, int64_t n, int bpt, int k, int64_t rows, int32_t *__restrict__ out,
                                                                  uint32_t *status) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        int64_t v = ids[i * bpt + k];
        if ((uint64_t)v >= (uint64_t)rows) { if (status) atomicOr(status, kStatusByteOor); v = 0; }
        out[i] = (int32_t)v;
    }
}

// workspace of the CONCAT backward, in floats unless noted:
//   [rnorm: byte_rows][dy: N*Dm][du: N*K][u_tok: N*Dt][u_byte: N*bpt*Db][Wk: Dm16*K128][byte0: 4][iota: N int32][zero ids: 0]
//   [sort ints: 3*tok_rows + N]
struct LinBwdLayout { size_t rnorm, dy, du, utok, ubyte, wk, byte0, iota, sort, total; int Kp, Dmp; };
static LinBwdLayout lin_bwd_layout(const MotEmbedMixDesc &d) {
    LinBwdLayout L;
    const size_t N = (size_t)(d.n_rows * d.tokens_per_row), K = (size_t)d.tok_dim + (size_t)d.bpt * d.byte_dim;
    L.Kp = (int)((K + 127) / 128 * 128);            // output columns of the du GEMM, padded as the MFMA kernel pads them
    if (L.Kp > 512 && L.Kp <= 768) L.Kp = 768; else if (L.Kp > 768) L.Kp = 1024;
    L.Dmp = (d.model_dim + 15) / 16 * 16;
    Arena ar{0, 4};   // counts floats
    L.rnorm = ar.take(d.byte_rows); L.dy = ar.take(N * d.model_dim); L.du = ar.take(N * K); L.utok = ar.take(N * d.tok_dim);
    L.ubyte = ar.take(N * d.bpt * d.byte_dim); L.wk = ar.take((size_t)L.Dmp * L.Kp); L.byte0 = ar.take(4); L.iota = ar.take(N);
    L.sort = ar.take(scatter_ws_ints(d)); L.total = ar.o;
    return L;
}

// bf16 CONCAT_LINEAR backward: the operands are widened once into fp32 workspace copies and the fp32 pipeline
// above runs on them (fp32 MFMA and fp32 accumulation throughout -- never less precise than bf16 autograd;
// the bf16-MFMA version of the three GEMMs is the open item).  Layout in floats, in front of LinBwdLayout.
struct UpLayout { size_t tok, byte, w, bias, g, x, total; };
static UpLayout up_layout(const MotEmbedMixDesc &d) {
    UpLayout U;
    const size_t N = (size_t)(d.n_rows * d.tokens_per_row), K = (size_t)d.tok_dim + (size_t)d.bpt * d.byte_dim;
    Arena ar{0, 4};   // counts floats
    U.tok = ar.take((size_t)d.tok_rows * d.tok_dim); U.byte = ar.take((size_t)d.byte_rows * d.byte_dim); U.w = ar.take((size_t)d.model_dim * K);
    U.bias = ar.take(d.bias ? d.model_dim : 0); U.g = ar.take(N * d.model_dim); U.x = ar.take(d.norm_out ? N * d.model_dim : 0);
    U.total = ar.o;
    return U;
}

// du = dy . W of the bf16 backward on the bf16 MFMA (what autograd does for bf16 parameters): dy rounded to bf16,
// W^T as the [K, Dm] "weight" of the forward bf16 kernel in dense-row mode, du widened back for the scatter stage.
// Scratch behind the fp32 layouts, in bytes: [dy16: N*Dm*2][wt16: K*Dm*2][u16: N*K*2].
struct Du16Layout { size_t dy16, wt16, uT, total; };
static Du16Layout du16_layout(const MotEmbedMixDesc &d) {
    Du16Layout U;
    const size_t N = (size_t)(d.n_rows * d.tokens_per_row), K = (size_t)d.tok_dim + (size_t)d.bpt * d.byte_dim, Dm = (size_t)d.model_dim;
    Arena ar;
    U.dy16 = ar.take(N * Dm * 2); U.wt16 = ar.take(K * Dm * 2);
    U.uT = ar.take(N * K * 2);   // the concat operand in bf16, row-major (dW)
    U.total = ar.o;
    return U;
}
static bool du16_usable(const MotEmbedMixDesc &d) {
    const int K = d.tok_dim + d.bpt * d.byte_dim;
    return d.dtype == MOT_BF16 && (d.model_dim & 7) == 0 && (K & 7) == 0 && K <= 4096 && ((d.n_rows * d.tokens_per_row) & 7) == 0 &&
           !(d.flags & MOT_FLAG_BWD_DU_FP32);
}

size_t embed_mix_bwd_linear_workspace_bytes(const MotEmbedMixDesc &d) {
    return (lin_bwd_layout(d).total + (d.dtype == MOT_BF16 ? up_layout(d).total : 0)) * 4 + 256 + (du16_usable(d) ? du16_layout(d).total : 0);
}

// `w16` / `ws16` (optional): the bf16 weight and the Du16Layout scratch -- then du and dW run on the bf16 MFMA; `g16` / `x16`
// (optional with them): the bf16 upstream gradient and forward output -- then dy is produced in bf16 directly and
// gr.grad_out / d.out (fp32) are never read; `d16`: the caller's descriptor with the bf16 tables (the concat operand of dW is then
// gathered from them directly, as the forward's was)
int launch_embed_mix_bwd_linear(const MotEmbedMixDesc &d, const MotEmbedMixGrads &gr, hipStream_t stream, const void *w16, char *ws16, const void *g16,
                                const void *x16, const MotEmbedMixDesc *d16) {
    if (d.id_source != MOT_IDS_GIVEN) return set_error(MOT_EUNSUPPORTED, "embed_mix_bwd: pass the byte ids the forward returned (MOT_IDS_GIVEN)");
    if (!gr.d_weight) return set_error(MOT_EINVAL, "embed_mix_bwd concat_linear: d_weight missing");
    if (d.norm_out && (!d.out || !d.out_row_rnorm)) return set_error(MOT_EINVAL, "embed_mix_bwd concat_linear: needs the forward's out and out_row_rnorm");
    const int64_t N = d.n_rows * d.tokens_per_row;
    const int Dm = d.model_dim, Dt = d.tok_dim, nbk = d.bpt * d.byte_dim, K = Dt + nbk;
    // rows wider than 1024 (mathblations' defaults: 768 + 3 x 768, model.py:21-24, 256-268) only where the table gradients can be
    // scattered part by part on the lane-contiguous kernel: token part and every byte slot a multiple of 256 columns, <= 1024 each
    // (rows up to 2048 columns: the strided kernels take them whole; wider ones -- the reference's dimension sweeps reach 1024 + 16 x
    //  128 = 3072, experiments100_000steps.sh, mathblations' defaults 768 + 3 x 768 -- only where the part-wise scatter below applies)
    if (Dm > 2048) return set_error(MOT_EUNSUPPORTED, "embed_mix_bwd concat_linear: model_dim %d > 2048", Dm);
    const LinBwdLayout L = lin_bwd_layout(d);
    if (d.dtype == MOT_BF16) {
        const UpLayout U = up_layout(d);
        if (!d.workspace || d.workspace_bytes < (U.total + L.total) * 4)
            return set_error(MOT_EWORKSPACE, "embed_mix_bwd: needs %zu workspace bytes, got %zu", (U.total + L.total) * 4, d.workspace_bytes);
        float *up = (float *)d.workspace;
        const size_t Nn = (size_t)N * Dm;
        int rc;
        if ((rc = launch_widen(d.tok_table, (size_t)d.tok_rows * Dt, up + U.tok, stream))) return rc;
        if ((rc = launch_widen(d.byte_table, (size_t)d.byte_rows * d.byte_dim, up + U.byte, stream))) return rc;
        if ((rc = launch_widen(d.weight, (size_t)Dm * K, up + U.w, stream))) return rc;
        if (d.bias && (rc = launch_widen(d.bias, Dm, up + U.bias, stream))) return rc;
        const bool route16 = du16_usable(d);
        const bool dy_in_bf16 = route16 && !d.bias && Dm <= 4096;   // the bias gradient is a column sum of an fp32 dy
        if (!dy_in_bf16) {
            if ((rc = launch_widen(gr.grad_out, Nn, up + U.g, stream))) return rc;
            if (d.norm_out && (rc = launch_widen(d.out, Nn, up + U.x, stream))) return rc;
        }
        MotEmbedMixDesc d32 = d;
        MotEmbedMixGrads g32 = gr;
        d32.dtype = MOT_F32;
        d32.tok_table = up + U.tok; d32.byte_table = up + U.byte; d32.weight = up + U.w; d32.bias = d.bias ? up + U.bias : nullptr;
        d32.out = d.norm_out ? (void *)(up + U.x) : nullptr;
        d32.eps = d.eps > 0.f ? d.eps : kBf16Eps;   // the forward normalised with the bf16 epsilon
        d32.workspace = up + U.total; d32.workspace_bytes = d.workspace_bytes - U.total * 4;
        g32.grad_out = up + U.g;
        if (route16) {
            const size_t off = ((U.total + L.total) * 4 + 255) & ~(size_t)255;
            if (d.workspace_bytes < off + du16_layout(d).total)
                return set_error(MOT_EWORKSPACE, "embed_mix_bwd: needs %zu workspace bytes, got %zu", off + du16_layout(d).total, d.workspace_bytes);
            return launch_embed_mix_bwd_linear(d32, g32, stream, d.weight, (char *)d.workspace + off, dy_in_bf16 ? gr.grad_out : nullptr,
                                               dy_in_bf16 ? d.out : nullptr, &d);
        }
        return launch_embed_mix_bwd_linear(d32, g32, stream);
    }
    if (!d.workspace || d.workspace_bytes < L.total * 4)
        return set_error(MOT_EWORKSPACE, "embed_mix_bwd: needs %zu workspace bytes, got %zu", L.total * 4, d.workspace_bytes);
    float *ws = (float *)d.workspace;
    float *rn = ws + L.rnorm, *dy = ws + L.dy, *du = ws + L.du, *utok = ws + L.utok, *ubyte = ws + L.ubyte, *wk = ws + L.wk, *byte0 = ws + L.byte0;
    int32_t *iota = (int32_t *)(ws + L.iota), *sort_ints = (int32_t *)(ws + L.sort);
    (void)wk; (void)byte0; (void)ubyte;   // slots of the layout the fp32 du product no longer uses (u is built in place: utok .. ubyte)
    const float eps = d.eps > 0.f ? d.eps : FLT_EPSILON;
    int rc;
    // 1. dy
    const float *dyp = (const float *)gr.grad_out;
    const __bf16 *dy16p = nullptr;   // bf16 route with bf16 inputs: dy exists in bf16 only
    if (g16) {
        const Du16Layout U = du16_layout(d);
        dy16p = (const __bf16 *)g16;
        if (d.norm_out) {
            __bf16 *dy16 = (__bf16 *)(ws16 + U.dy16);
            if ((rc = launch_rows_norm_bwd(g16, x16, d.out_row_rnorm, N, Dm, 1, dy16, Dm, nullptr, 0, MOT_BF16, stream))) return rc;
            dy16p = dy16;
        }
        dyp = nullptr;
    } else if (d.norm_out) {
        if ((rc = launch_rows_norm_bwd(gr.grad_out, d.out, d.out_row_rnorm, N, Dm, 1, dy, Dm, nullptr, 0, MOT_F32, stream))) return rc;
        dyp = dy;
    }
    if (gr.d_bias) {
        hipLaunchKernelGGL(colsum_kernel, dim3(256), dim3(kThreads), 0, stream, dyp, N, Dm, (float *)gr.d_bias);
        if ((rc = check_launch("colsum_kernel"))) return rc;
    }
    // 2. u = the seam tensors (norms and scalars applied), and dW += dy^T u
    const int64_t blk = 2048;
    (void)blk;
    const int tok_lo = d.bytes_first ? nbk : 0, byte_lo = d.bytes_first ? 0 : Dt;
    float *dW = (float *)gr.d_weight;
    // (w16: the concat operand goes straight to bf16, below)
    if (!w16) {  // fp32: the concat operand u [N, K] itself, in the two (adjacent) scratch regions, so dW is ONE contraction
        if ((rc = launch_gather_rows_placed(d.tokens, nullptr, 4, N, d.tok_table, d.tok_rows, Dt, d.norm_tok, eps, d.scale_tok, utok + tok_lo, 1, K,
                                            d.status, kStatusTokenOor, MOT_F32, stream))) return rc;
        if ((rc = launch_gather_rows_placed(d.ids_a, d.ids_b, 8, N * d.bpt, d.byte_table, d.byte_rows, d.byte_dim, d.norm_byte, eps, d.scale_byte,
                                            utok + byte_lo, d.bpt, K, d.status, kStatusByteOor, MOT_F32, stream))) return rc;
        if ((rc = launch_gemm_tn(dyp, Dm, Dm, utok, K, K, N, dW, K, stream))) return rc;
    } else {
        // 2'. dW on the bf16 MFMA: dy [N, Dm] and u [N, K] in bf16, ROW-major as they are, contracted over the tokens by
        // gemm_tn_bf16_kernel (transposing LDS reads).  u is the forward's operand: gathered from the bf16 tables by the forward's
        // own concat_rows_kernel when that applies (one id tensor, no learned scalars, 16-byte pieces), else gathered in fp32 from
        // the widened tables and narrowed.
        const Du16Layout U = du16_layout(d);
        __bf16 *dy16 = (__bf16 *)(ws16 + U.dy16), *u16 = (__bf16 *)(ws16 + U.uT);
        const __bf16 *dyr = dy16p;
        if (!dyr) {
            if ((rc = launch_narrow(dyp, (int64_t)N * Dm, dy16, stream))) return rc;
            dyr = dy16;
        }
        if (d16 && !d.ids_b && !d.scale_tok && !d.scale_byte && (Dt & 7) == 0 && (d.byte_dim & 7) == 0) {
            if (d.norm_byte && (rc = launch_rows_rnorm(d16->byte_table, d.byte_rows, d.byte_dim, eps, rn, MOT_BF16, stream))) return rc;
            if ((rc = launch_concat_rows(d.tokens, d.ids_a, N, d16->tok_table, d.tok_rows, Dt, d16->byte_table, d.byte_rows, d.byte_dim, d.bpt, d.norm_tok,
                                         d.norm_byte ? rn : nullptr, eps, u16, K, tok_lo, byte_lo, d.status, MOT_BF16, stream))) return rc;
        } else {
            if ((rc = launch_gather_rows_placed(d.tokens, nullptr, 4, N, d.tok_table, d.tok_rows, Dt, d.norm_tok, eps, d.scale_tok, utok + tok_lo, 1, K,
                                                d.status, kStatusTokenOor, MOT_F32, stream))) return rc;
            if ((rc = launch_gather_rows_placed(d.ids_a, d.ids_b, 8, N * d.bpt, d.byte_table, d.byte_rows, d.byte_dim, d.norm_byte, eps, d.scale_byte,
                                                utok + byte_lo, d.bpt, K, d.status, kStatusByteOor, MOT_F32, stream))) return rc;
            if ((rc = launch_narrow(utok, (int64_t)N * K, u16, stream))) return rc;
        }
        if ((rc = launch_gemm_tn_bf16(dyr, Dm, Dm, u16, K, K, N, dW, K, stream))) return rc;
    }
    hipLaunchKernelGGL(iota_kernel, dim3(256), dim3(kThreads), 0, stream, iota, N);
    if (w16) {
        // 3'. du on the bf16 MFMA: bf16(dy) rows x W^T on the dense bf16 kernel
        const Du16Layout U = du16_layout(d);
        __bf16 *dy16 = (__bf16 *)(ws16 + U.dy16), *wt16 = (__bf16 *)(ws16 + U.wt16);
        if (dy16p) dy16 = const_cast<__bf16 *>(dy16p);   // (else narrowed for dW above)
        if ((rc = launch_transpose_bf16(w16, Dm, K, wt16, stream))) return rc;
        // du[n][k] = sum_m dy16[n][m] * wt16[k][m], accumulated and written in fp32 (no bf16 round trip before the scatter)
        if ((rc = launch_gemm_rows_bf16(dy16, Dm, N, wt16, Dm, Dm, K, du, K, false, nullptr, stream))) return rc;
    } else {
    // 3. du = dy . W   (N x Dm) @ (Dm x K): both row-major as they are (nn.Linear keeps W as [Dm][K])
    //    (W transposed once and the product on the LDS-DMA kernel, as the cross-attention backward does with its k-major products:
    //     measured, 2.625 against 2.63 ms for forward + backward -- not kept here)
    if ((rc = launch_gemm_rows(dyp, Dm, N, (const float *)d.weight, K, Dm, K, du, K, false, stream))) return rc;
    }
    // 4. table gradients from du (its row layout is the concat layout)
    BwdArgs A;
    fill_bwd_args(A, d, gr);
    A.grad_out = du; A.D = K; A.norm_out = 0;
    A.Dt = Dt; A.tok_lo = tok_lo; A.byte_lo = byte_lo; A.nbk = nbk;
    // The two halves of a du row are two embedding backwards: the token part a plain one (NOOP) over Dt columns, the byte part a SUM
    // over byte slots with no token table -- both on the lane-contiguous kernel, reading their columns of du in place (row stride K),
    // sharing one grouping of the positions.  (The strided kernel of round 1 took 242 us of the 870 us the bf16 concat forward +
    // backward takes at 65 536 tokens.)  One id tensor only: norm_byte over two id tensors normalises the SUM of two rows.
    if (!d.ids_b) {
        BwdArgs At = A, Ab = A;
        At.D = At.Dt = Dt; At.tok_lo = At.byte_lo = 0; At.nbk = 0; At.grad_out = du + tok_lo; At.g_ld = K; At.d_byte = nullptr;
        Ab.D = Ab.Dt = nbk; Ab.tok_lo = Ab.byte_lo = 0; Ab.nbk = nbk; Ab.grad_out = du + byte_lo; Ab.g_ld = K; Ab.no_tok = 1; Ab.d_tok = nullptr;
        Ab.norm_tok = 0; Ab.tok_table = nullptr;
        // the byte part in blocks of whole slots, <= 1024 columns each (16 x 128-wide slots are two blocks of 8)
        int per = d.bpt;
        while (per > 1 && per * d.byte_dim > 1024) per = (per + 1) / 2;
        Ab.D = Ab.Dt = Ab.nbk = per * d.byte_dim;
        // (the token part: the lane-contiguous kernel, or -- 896 columns -- the general one, which knows the row stride too)
        bool split = d.bpt % per == 0 && lc_layout(MOT_MIX_SUM, Ab) && (lc_layout(MOT_MIX_NOOP, At) || K > 2048);
#ifdef MOT_DEV_ABLATION
        if (getenv("MOT_CONCAT_SCATTER_OLD")) split = false;
#endif
        if (split) {
            if ((rc = run_scatter(MOT_MIX_NOOP, At, d, sort_ints, rn, stream))) return rc;
            for (int s0 = 0; s0 < d.bpt; s0 += per) {
                BwdArgs Ac = Ab;
                Ac.pos_sorted = At.pos_sorted; Ac.tok_sorted = At.tok_sorted;
                Ac.slot0 = s0; Ac.grad_out = du + byte_lo + s0 * d.byte_dim;
                if ((rc = run_scatter(MOT_MIX_SUM, Ac, d, sort_ints, rn, stream))) return rc;
            }
            return MOT_OK;
        }
        // Wide byte slots (a slot is a whole embedding row: the digit mixin): every slot is a plain embedding backward of its own, the
        // slot's ids as the "tokens", the byte table as the table, its columns of du as the gradient rows
        if (lc_layout(MOT_MIX_NOOP, At) && (d.byte_dim & 255) == 0 && d.byte_dim <= 1024 && !d.scale_tok && !d.scale_byte) {
            if ((rc = run_scatter(MOT_MIX_NOOP, At, d, sort_ints, rn, stream))) return rc;
            for (int k = 0; k < d.bpt; ++k) {
                hipLaunchKernelGGL(ids_column_i32_kernel, dim3(256), dim3(kThreads), 0, stream, d.ids_a, N, d.bpt, k, d.byte_rows, iota, d.status);
                if ((rc = check_launch("ids_column_i32_kernel"))) return rc;
                BwdArgs As = A;
                As.tokens = iota; As.tok_table = A.byte_table; As.tok_rows = d.byte_rows; As.norm_tok = d.norm_byte;
                As.D = As.Dt = d.byte_dim; As.tok_lo = As.byte_lo = 0; As.nbk = 0; As.grad_out = du + byte_lo + k * d.byte_dim; As.g_ld = K;
                As.d_tok = A.d_byte; As.d_byte = nullptr; As.pos_sorted = As.tok_sorted = nullptr;
                if (!lc_layout(MOT_MIX_NOOP, As)) return set_error(MOT_EUNSUPPORTED, "embed_mix_bwd concat_linear: byte slots of %d columns", d.byte_dim);
                MotEmbedMixDesc ds = d;   // (run_scatter reads the table height from the descriptor)
                ds.tok_rows = d.byte_rows;
                if ((rc = run_scatter(MOT_MIX_NOOP, As, ds, sort_ints, rn, stream))) return rc;
            }
            return MOT_OK;
        }
    }
    if (K > 2048)
        return set_error(MOT_EUNSUPPORTED, "embed_mix_bwd concat_linear: K %d > 2048 needs the part-wise scatter (one id tensor, no learned scalars, "
                         "byte slots that tile blocks of <= 1024 columns)", K);
    return run_scatter(MOT_MIX_CONCAT_LINEAR, A, d, sort_ints, rn, stream);
}

}  // namespace mot
