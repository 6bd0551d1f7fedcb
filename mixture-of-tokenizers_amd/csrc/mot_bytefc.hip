// mot_bytefc.hip -- the linear-on-bytes mixin of modded-nanogpt/runs/71051_mot-in_toks-valemb.py:225-229 (call site 312-314):
//     u_n = cat_k E_byte[ids[n, k]],   x_n = rms_norm?(E_tok[tok_n] + byte_fc u_n),   byte_fc [model_dim, K = bpt * byte_dim]
// forward and backward, fp32 and bf16 (include/mot.h, MotByteFcMixDesc).  Composed from the shared pieces -- the index kernels
// (mot_index.hip), the placed gather (mot_embed.hip), the three products (launch_product_nt / _nn / _tn, mot_internal.hpp), the
// linear front-ends' row passes and pad count (mot_lincore.hip: the finishing pass in its token-row form, the norm's backward for
// fp32 tensors) and the table-gradient scatter (run_scatter, mot_backward.hip) -- plus one kernel of its own, the norm's backward
// for bf16 tensors from the pre-norm row.  The operand u and the gradient rows live in the caller's workspace, slab by slab.
#include "mot_bwd.hpp"
#include "mot_lincore.hpp"

namespace mot {

constexpr int64_t kFcFwdSlab = 16384;   // rows of u per forward slab: 64 MiB of fp32 at K 1024; 64 x 4 product tiles of 256 x 256 fill the chip once
constexpr int64_t kFcBwdSlab = 65536;   // rows of [ds | du] per backward slab (run 71051's whole shard: the caller's token order applies)
constexpr int kFcMaxDim = kRowMaxDim;   // the row passes keep a row of model_dim columns in registers (mot_lincore.hip)

// ------------------------------------------------------------------------------------------ kernel
// The norm's backward for bf16 tensors, from the pre-norm row instead of the saved output (which launch_rows_norm_bwd, the fp32
// tensors' way, reads): the forward's x is a bf16 tensor, three roundings (2^-9 each) away from the exact row, and
// r (g - x mean(g x)) built on it misses the exact ds by 2e-4 .. 8e-4 of its largest element -- the token-table gradient, a plain sum of ds rows, would carry that (measured on the host at model_dim 64 .. 1024).
// So the backward forms p = byte_fc u once more, keeps its fp32 sums (they sit in columns [0, Dm) of the gradient rows when this
// kernel starts), and takes s = tok + p, r and x = r s in fp32 from there: ds then agrees with the float64 gradient at the
// bf16-valued operands like the fp32 path does, for one more product of the forward's size.  Written in place, and as bf16.
__global__ __launch_bounds__(kThreads) void bytefc_ds16_kernel(const __bf16 *__restrict__ g, const int32_t *__restrict__ tokens, int64_t n,
                                                               const __bf16 *__restrict__ tok_table, int64_t tok_rows, int Dm, float eps,
                                                               float *__restrict__ rows, int ld, __bf16 *__restrict__ ds16) {
    constexpr int NCH = kFcMaxDim / 8 / 64;
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (r >= n) return;
    int tok = __builtin_amdgcn_readfirstlane(tokens[r]);
    if ((uint64_t)(uint32_t)tok >= (uint64_t)tok_rows) tok = 0;   // (flagged where the positions are grouped)
    const __bf16 *trow = tok_table + (int64_t)tok * Dm, *gr = g + r * Dm;
    float *pr = rows + r * (int64_t)ld;
    const int nv = Dm / 8;
    float8v sv[NCH], gv[NCH];
    float ss = 0.f, m = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int j = lane + 64 * i;
        sv[i] = (float8v)(0.f); gv[i] = (float8v)(0.f);
        if (j < nv) {
            const float4v p0 = *(const float4v *)(pr + 8 * j), p1 = *(const float4v *)(pr + 8 * j + 4);
            sv[i] = Elem<__bf16>::loadv(trow + 8 * j) + float8v{p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
            gv[i] = Elem<__bf16>::loadv(gr + 8 * j);
#pragma unroll
            for (int e = 0; e < 8; ++e) { ss += sv[i][e] * sv[i][e]; m += gv[i][e] * sv[i][e]; }
        }
    }
    const float rs = rms_scale(wave_sum(ss), Dm, eps);
    const float c = wave_sum(m) / (float)Dm * rs * rs;   // x mean(g x) = s (r^2 mean(g s))
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int j = lane + 64 * i;
        if (j < nv) {
            const float8v d = (gv[i] - sv[i] * c) * rs;
            *(float4v *)(pr + 8 * j) = float4v{d[0], d[1], d[2], d[3]};
            *(float4v *)(pr + 8 * j + 4) = float4v{d[4], d[5], d[6], d[7]};
            Elem<__bf16>::storev_nt(ds16 + r * Dm + 8 * j, d);
        }
    }
}

// ------------------------------------------------------------------------------------------ validation (no HIP call)

// rows of the lane-contiguous scatter: the byte part of [ds | du] in blocks of `per` whole slots (0: the general kernel takes the row)
static int scatter_split_per(int Dm, int Db, int bpt) {
    BwdArgs At{}, Ab{};
    At.D = At.Dt = Dm;
    int per = bpt;
    while (per > 1 && per * Db > 1024) per = (per + 1) / 2;
    Ab.D = Ab.Dt = Ab.nbk = per * Db; Ab.Db = Db;
    return (bpt % per == 0 && lc_layout(MOT_MIX_SUM, Ab) && lc_layout(MOT_MIX_NOOP, At)) ? per : 0;
}

// everything that does not need the pointers: also what the two size queries run
static int byte_fc_check_shape(const MotByteFcMixDesc *d, bool backward) {
    if (!d) return set_error(MOT_EINVAL, "byte_fc_mix: null descriptor");
    if (d->struct_size != sizeof(MotByteFcMixDesc))
        return set_error(MOT_EINVAL, "byte_fc_mix: struct_size %u != %zu (ABI mismatch)", d->struct_size, sizeof(MotByteFcMixDesc));
    if (d->dtype != MOT_F32 && d->dtype != MOT_BF16) return set_error(MOT_EINVAL, "byte_fc_mix: bad dtype %d", d->dtype);
    if (d->flags & ~MOT_BYTE_FC_COMPOSED) return set_error(MOT_EINVAL, "byte_fc_mix: unknown flags 0x%x", d->flags);
    if (d->n_rows < 0 || d->tokens_per_row < 0) return set_error(MOT_ESHAPE, "byte_fc_mix: negative shape");
    if (int rc = check_id_source_shape("byte_fc_mix", id_source_of(*d), backward)) return rc;
    if (d->tok_rows <= 0 || d->byte_rows <= 0 || d->tok_dim <= 0 || d->byte_dim <= 0 || d->model_dim <= 0)
        return set_error(MOT_ESHAPE, "byte_fc_mix: empty table (tok %lld x %d, byte %lld x %d, model_dim %d)", (long long)d->tok_rows, d->tok_dim,
                         (long long)d->byte_rows, d->byte_dim, d->model_dim);
    if (d->tok_dim != d->model_dim) return set_error(MOT_ESHAPE, "byte_fc_mix: tok_dim %d != model_dim %d", d->tok_dim, d->model_dim);
    const int vec = d->dtype == MOT_BF16 ? 8 : 4;
    if ((d->model_dim % vec) || (d->byte_dim % vec))
        return set_error(MOT_EUNSUPPORTED, "byte_fc_mix: model_dim %d / byte_dim %d must be multiples of %d elements (16 bytes)", d->model_dim, d->byte_dim,
                         vec);
    const int64_t K = (int64_t)d->bpt * d->byte_dim;
    if (d->model_dim > kFcMaxDim || K > kFcMaxDim)
        return set_error(MOT_EUNSUPPORTED, "byte_fc_mix: model_dim %d / bpt*byte_dim %lld above %d is not built", d->model_dim, (long long)K, kFcMaxDim);
    if (int rc = check_id_source_limits("byte_fc_mix", id_source_of(*d))) return rc;
    if (backward) {
        if (d->tok_rows >= (1 << 21) - 1)
            return set_error(MOT_EUNSUPPORTED, "byte_fc_mix_bwd: token tables of %lld rows (>= 2^21 - 1) are not built", (long long)d->tok_rows);
        if (d->model_dim + K > kFcMaxDim && !scatter_split_per(d->model_dim, d->byte_dim, d->bpt))
            return set_error(MOT_EUNSUPPORTED, "byte_fc_mix_bwd: gradient rows of model_dim %d + bpt*byte_dim %lld > %d columns need the part-wise scatter "
                             "(model_dim and whole-slot blocks of the byte part multiples of 256, <= 1024)", d->model_dim, (long long)K, kFcMaxDim);
    }
    return MOT_OK;
}

// forward workspace: [u: slab rows x K][ids padded | pulled: N * bpt int64 each (FROM_TTB)]
struct FcFwdLayout { size_t u, ids, total; };
static FcFwdLayout fc_fwd_layout(const MotByteFcMixDesc &d) {
    const size_t N = (size_t)(d.n_rows * d.tokens_per_row), K = (size_t)d.bpt * d.byte_dim, esz = d.dtype == MOT_BF16 ? 2 : 4;
    const size_t ns = N < (size_t)kFcFwdSlab ? N : (size_t)kFcFwdSlab;
    FcFwdLayout L;
    Arena ar;
    L.u = ar.take(ns * K * esz);
    L.ids = ar.take(d.id_source == MOT_IDS_FROM_TTB ? 2 * N * d.bpt * sizeof(int64_t) : 0);
    L.total = ar.o;
    return L;
}

// backward workspace: [rows [ds | du]: slab x (Dm + K) fp32][sort ints][u: slab x K][bf16: ds16, byte_fc^T, fp32 copies of the tables]
struct FcBwdLayout { size_t rows, sort, u, ds16, wt16, tok32, byte32, total; int64_t slab; };
static FcBwdLayout fc_bwd_layout(const MotByteFcMixDesc &d) {
    const size_t N = (size_t)(d.n_rows * d.tokens_per_row), K = (size_t)d.bpt * d.byte_dim, Dm = (size_t)d.model_dim;
    const bool bf = d.dtype == MOT_BF16;
    FcBwdLayout L;
    L.slab = (int64_t)(N < (size_t)kFcBwdSlab ? N : (size_t)kFcBwdSlab);
    const size_t ns = (size_t)L.slab;
    Arena ar;
    L.rows = ar.take(ns * (Dm + K) * 4);
    L.sort = ar.take((2 * (size_t)d.tok_rows + 3 * ns) * 4);
    L.u = ar.take(ns * K * (bf ? 2 : 4));
    L.ds16 = ar.take(bf ? ns * Dm * 2 : 0);
    L.wt16 = ar.take(bf ? K * Dm * 2 : 0);
    L.tok32 = ar.take(bf ? (size_t)d.tok_rows * Dm * 4 : 0);
    L.byte32 = ar.take(bf ? (size_t)d.byte_rows * d.byte_dim * 4 : 0);
    L.total = ar.o;
    return L;
}

size_t byte_fc_mix_workspace_bytes(const MotByteFcMixDesc *d) { return byte_fc_check_shape(d, false) ? 0 : fc_fwd_layout(*d).total; }
size_t byte_fc_mix_bwd_workspace_bytes(const MotByteFcMixDesc *d) { return byte_fc_check_shape(d, true) ? 0 : fc_bwd_layout(*d).total; }

int byte_fc_check(const MotByteFcMixDesc *d, const MotByteFcMixGrads *g, bool backward) {
    if (int rc = byte_fc_check_shape(d, backward)) return rc;
    if (!d->byte_fc) return set_error(MOT_EINVAL, "byte_fc_mix: byte_fc [%d, %d] missing", d->model_dim, d->bpt * d->byte_dim);
    if (!d->tokens || !d->tok_table || !d->byte_table) return set_error(MOT_EINVAL, "byte_fc_mix: tokens/tok_table/byte_table must be non-null");
    if (int rc = check_id_source_ptrs("byte_fc_mix", id_source_of(*d))) return rc;
    if (backward) {
        if (!g || g->struct_size != sizeof(MotByteFcMixGrads)) return set_error(MOT_EINVAL, "byte_fc_mix_bwd: grads struct missing or struct_size mismatch");
        if (!g->grad_out || !g->d_tok || !g->d_byte || !g->d_byte_fc) return set_error(MOT_EINVAL, "byte_fc_mix_bwd: grad_out/d_tok/d_byte/d_byte_fc must be non-null");
        if (d->norm_out && d->dtype == MOT_F32 && (!d->out || !d->out_row_rnorm))
            return set_error(MOT_EINVAL, "byte_fc_mix_bwd: needs the forward's out and out_row_rnorm");
    } else if (!d->out) {
        return set_error(MOT_EINVAL, "byte_fc_mix: out must be non-null");
    }
    if (d->n_rows == 0 || d->tokens_per_row == 0) return MOT_OK;
    return check_workspace("byte_fc_mix", backward, d->workspace, d->workspace_bytes, backward ? fc_bwd_layout(*d).total : fc_fwd_layout(*d).total);
}

// ------------------------------------------------------------------------------------------ forward
int launch_byte_fc_mix_fwd(const MotByteFcMixDesc &d, hipStream_t stream) {
    const int64_t N = d.n_rows * d.tokens_per_row, slots = N * d.bpt;
    const int Dm = d.model_dim, Db = d.byte_dim, bpt = d.bpt, K = bpt * Db;
    const bool bf = d.dtype == MOT_BF16;
    const size_t esz = bf ? 2 : 4;
    const float eps = d.eps > 0.f ? d.eps : FLT_EPSILON;
    const FcFwdLayout L = fc_fwd_layout(d);
    char *ws = (char *)d.workspace;
    int rc;
    // bf16 at the shapes of mot_concat16.hip: one wave-local index pass (16-bit ids, id outputs and statistics included) when the ids
    // come from the token->byte table, then ONE gather-GEMM in its residual form -- u is never built, the K loop is half the
    // [I | byte_fc] emulation's, the token row joins in the epilogue's row pass
    if (bf && !(d.flags & MOT_BYTE_FC_COMPOSED)) {
        MotEmbedMixDesc e{};
        e.struct_size = sizeof(MotEmbedMixDesc); e.dtype = MOT_BF16; e.mode = MOT_MIX_CONCAT_LINEAR;
        e.n_rows = d.n_rows; e.tokens_per_row = d.tokens_per_row; e.bpt = bpt; e.tokens = d.tokens;
        e.id_source = d.id_source; e.pull_dir = d.pull_dir; e.ttb = d.ttb; e.ttb_rows = d.ttb_rows; e.ttb_elem_bytes = d.ttb_elem_bytes;
        e.pad_byte = d.pad_byte; e.eot_byte = d.eot_byte; e.ids_a = d.ids;
        e.tok_table = d.tok_table; e.tok_rows = d.tok_rows; e.tok_dim = Dm; e.byte_dim = Db; e.byte_table = d.byte_table; e.byte_rows = d.byte_rows;
        e.model_dim = Dm; e.weight = d.byte_fc; e.norm_out = d.norm_out; e.eps = eps;
        e.out = d.out; e.out_ids_padded = d.out_ids_padded; e.out_ids_pulled = d.out_ids_pulled; e.counters = d.counters; e.status = d.status;
        if (concat16_residual_usable(e)) {
            if (d.id_source == MOT_IDS_FROM_TTB) {
                uint16_t *ids16 = (uint16_t *)(ws + L.ids);
                if ((rc = launch_wave_ids16(e, ids16, stream))) return rc;
                return launch_concat16(e, d.tokens, nullptr, ids16, N, nullptr, d.out, d.out_row_rnorm, stream, true);
            }
            if (d.counters && (rc = launch_count_pads(nullptr, d.ids, slots, d.pad_byte, N, d.counters, stream))) return rc;
            return launch_concat16(e, d.tokens, d.ids, nullptr, N, nullptr, d.out, d.out_row_rnorm, stream, true);
        }
    }
    // 1. the byte ids: given, or the loader's two index kernels (tokens_to_bytes, pull) into the caller's id outputs or the workspace
    const int64_t *ids = d.ids, *padded_c = nullptr;
    if (d.id_source == MOT_IDS_FROM_TTB) {
        int64_t *ws_ids = (int64_t *)(ws + L.ids);
        int64_t *padded = d.out_ids_padded ? d.out_ids_padded : ws_ids;
        int64_t *pulled = d.out_ids_pulled ? d.out_ids_pulled : ws_ids + slots;
        if ((rc = launch_ids_from_ttb(id_source_of(d), padded, pulled, &ids, stream))) return rc;
        padded_c = padded;
        if (d.pull_dir == MOT_PULL_NONE && d.out_ids_pulled)   // nothing is pulled: that output is the padded tensor again
            if ((rc = launch_tokens_to_bytes(d.tokens, N, d.ttb, d.ttb_elem_bytes, d.ttb_rows, bpt, d.out_ids_pulled, nullptr, stream))) return rc;
    }
    if (d.counters && (rc = launch_count_pads(padded_c, ids, slots, d.pad_byte, N, d.counters, stream))) return rc;
    // 2. slab by slab: u = the token's byte rows side by side, p = u byte_fc^T into `out`, then the row pass in place
    char *u = ws + L.u;
    for (int64_t r0 = 0; r0 < N; r0 += kFcFwdSlab) {
        const int64_t n = N - r0 < kFcFwdSlab ? N - r0 : kFcFwdSlab;
        if ((rc = launch_gather_rows_placed(ids + r0 * bpt, nullptr, 8, n * bpt, d.byte_table, d.byte_rows, Db, 0, eps, nullptr, u, bpt, K, d.status,
                                            kStatusByteOor, d.dtype, stream))) return rc;
        char *out = (char *)d.out + (size_t)r0 * Dm * esz;
        float *rr = d.out_row_rnorm ? d.out_row_rnorm + r0 : nullptr;
        if ((rc = launch_product_nt(d.dtype, u, K, n, d.byte_fc, K, K, Dm, out, Dm, bf, nullptr, false, stream))) return rc;
        // s = tok + p, x = r s: 16 * model_dim bytes of traffic per fp32 token (row in, token row in, row out)
        if ((rc = launch_rows_finish_tok(out, d.tokens + r0, d.tok_table, d.tok_rows, n, Dm, d.norm_out, eps, rr, d.status, d.dtype, stream))) return rc;
    }
    return MOT_OK;
}

// ------------------------------------------------------------------------------------------ backward
// The gradient row [ds | du] of a token is the split row [token part | byte part] of the CONCAT_LINEAR scatter: d_tok and d_byte
// come from run_scatter (mot_backward.hip), which wants fp32 rows and fp32 tables (it reads the rows of both tables although
// nothing is normalised here), so bf16 tables are widened into the workspace first.
int launch_byte_fc_mix_bwd(const MotByteFcMixDesc &d, const MotByteFcMixGrads &gr, hipStream_t stream) {
    const int64_t N = d.n_rows * d.tokens_per_row;
    const int Dm = d.model_dim, Db = d.byte_dim, bpt = d.bpt, K = bpt * Db, ld = Dm + K;
    const bool bf = d.dtype == MOT_BF16;
    const size_t esz = bf ? 2 : 4;
    const float eps = d.eps > 0.f ? d.eps : FLT_EPSILON;
    const FcBwdLayout L = fc_bwd_layout(d);
    char *ws = (char *)d.workspace;
    float *rows = (float *)(ws + L.rows), *dW = (float *)gr.d_byte_fc;
    int32_t *sort_ints = (int32_t *)(ws + L.sort);
    char *u = ws + L.u;
    __bf16 *ds16 = (__bf16 *)(ws + L.ds16), *wt16 = (__bf16 *)(ws + L.wt16);
    const float *tok32 = (const float *)d.tok_table, *byte32 = (const float *)d.byte_table;
    int rc;
    if (bf) {
        if ((rc = launch_widen(d.tok_table, (size_t)d.tok_rows * Dm, (float *)(ws + L.tok32), stream))) return rc;
        if ((rc = launch_widen(d.byte_table, (size_t)d.byte_rows * Db, (float *)(ws + L.byte32), stream))) return rc;
        if ((rc = launch_transpose_bf16(d.byte_fc, Dm, K, wt16, stream))) return rc;   // du[n][k] = sum_m ds[n][m] byte_fc[m][k]: byte_fc^T is the [K, Dm] "weight"
        tok32 = (const float *)(ws + L.tok32); byte32 = (const float *)(ws + L.byte32);
    }
    const int per = scatter_split_per(Dm, Db, bpt);
    for (int64_t r0 = 0; r0 < N; r0 += L.slab) {
        const int64_t n = N - r0 < L.slab ? N - r0 : L.slab;
        const char *g = (const char *)gr.grad_out + (size_t)r0 * Dm * esz;
        const bool saved = d.norm_out && !bf;   // the fp32 backward reads the forward's x and r
        const char *x = saved ? (const char *)d.out + (size_t)r0 * Dm * esz : nullptr;
        const float *rn = saved ? d.out_row_rnorm + r0 : nullptr;
        const int64_t *ids = d.ids + r0 * bpt;
        // 1. u again; 2. ds into columns [0, Dm) of the gradient rows; 3. du = ds byte_fc into columns [Dm, Dm + K); 4. d_byte_fc += ds^T u
        if ((rc = launch_gather_rows_placed(ids, nullptr, 8, n * bpt, d.byte_table, d.byte_rows, Db, 0, eps, nullptr, u, bpt, K, d.status, kStatusByteOor,
                                            d.dtype, stream))) return rc;
        if (bf && d.norm_out) {   // from the pre-norm row: p = u byte_fc^T again, fp32 sums kept (see bytefc_ds16_kernel)
            if ((rc = launch_gemm_rows_bf16(u, K, n, d.byte_fc, K, K, Dm, rows, ld, false, nullptr, stream))) return rc;
            hipLaunchKernelGGL(bytefc_ds16_kernel, dim3((unsigned)((n + kWaves - 1) / kWaves)), dim3(kThreads), 0, stream, (const __bf16 *)g, d.tokens + r0, n,
                               (const __bf16 *)d.tok_table, d.tok_rows, Dm, eps, rows, ld, ds16);
            if ((rc = check_launch("bytefc_ds16_kernel"))) return rc;
        } else if ((rc = launch_rows_norm_bwd(g, x, rn, n, Dm, saved, bf ? ds16 : nullptr, Dm, rows, ld, d.dtype, stream))) {   // fp32, or ds = g
            return rc;
        }
        const void *ds = bf ? (const void *)ds16 : rows;   // the products' operand: the bf16 copy, or columns [0, Dm) of the rows
        const int ld_ds = bf ? Dm : ld;
        if ((rc = launch_product_nn(d.dtype, ds, ld_ds, n, bf ? (const void *)wt16 : d.byte_fc, bf ? Dm : K, Dm, K, rows + Dm, ld, stream))) return rc;
        if ((rc = launch_product_tn(d.dtype, ds, ld_ds, Dm, u, K, K, n, dW, K, stream))) return rc;
        // 5. the table gradients from [ds | du]
        MotEmbedMixDesc e{};
        e.struct_size = sizeof(MotEmbedMixDesc); e.dtype = MOT_F32; e.mode = MOT_MIX_CONCAT_LINEAR;
        e.n_rows = 1; e.tokens_per_row = n; e.bpt = bpt;
        e.tokens = d.tokens + r0; e.id_source = MOT_IDS_GIVEN; e.ids_a = ids;
        e.tok_table = tok32; e.tok_rows = d.tok_rows; e.tok_dim = Dm; e.byte_dim = Db; e.byte_table = byte32; e.byte_rows = d.byte_rows;
        e.model_dim = Dm; e.eps = eps; e.status = d.status;
        MotEmbedMixGrads eg{};
        eg.struct_size = sizeof(MotEmbedMixGrads);
        eg.grad_out = rows; eg.d_tok_table = gr.d_tok; eg.d_byte_table = gr.d_byte;
        eg.token_order = N <= L.slab ? gr.token_order : nullptr;   // the caller's order covers the whole batch: one slab only
        BwdArgs A;
        fill_bwd_args(A, e, eg);
        A.grad_out = rows; A.D = ld; A.norm_out = 0;
        A.Dt = Dm; A.tok_lo = 0; A.byte_lo = Dm; A.nbk = K;
        if (per) {   // the two halves as two embedding backwards on the lane-contiguous kernel, as the CONCAT_LINEAR backward runs them
            BwdArgs At = A, Ab = A;
            At.D = At.Dt = Dm; At.tok_lo = At.byte_lo = 0; At.nbk = 0; At.grad_out = rows; At.g_ld = ld; At.d_byte = nullptr;
            Ab.D = Ab.Dt = Ab.nbk = per * Db; Ab.tok_lo = Ab.byte_lo = 0; Ab.g_ld = ld; Ab.no_tok = 1; Ab.d_tok = nullptr; Ab.tok_table = nullptr;
            if ((rc = run_scatter(MOT_MIX_NOOP, At, e, sort_ints, nullptr, stream))) return rc;
            for (int s0 = 0; s0 < bpt; s0 += per) {
                BwdArgs Ac = Ab;
                Ac.pos_sorted = At.pos_sorted; Ac.tok_sorted = At.tok_sorted;
                Ac.slot0 = s0; Ac.grad_out = rows + Dm + s0 * Db;
                if ((rc = run_scatter(MOT_MIX_SUM, Ac, e, sort_ints, nullptr, stream))) return rc;
            }
        } else if ((rc = run_scatter(MOT_MIX_CONCAT_LINEAR, A, e, sort_ints, nullptr, stream))) {
            return rc;
        }
    }
    return MOT_OK;
}

}  // namespace mot
