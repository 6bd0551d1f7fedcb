// mot_valuemix.hip -- mixture-of-tokenizers value embeddings of modded-nanogpt/runs/9_mot-in_mot-valemb.py:310-313 (mixin_bytes
// 225-235; runs 3 and 6 alike): for one to four slots j over ONE token stream and ONE byte-id stream,
//     u_j[n] = cat(Vt_j[tok_n], Vb_j[ids[n, 0]], ..., Vb_j[ids[n, bpt-1]]),   ve_j[n] = rms_norm?(W_j u_j[n]),   W_j [out_dim, K]
// forward and backward, fp32 and bf16 (include/mot.h, MotValueMixDesc).  Composed from the shared pieces:
//   ids        given, or made once for all slots by the index kernels (mot_index.hip);
//   forward    bf16 at the gather-GEMM's shapes: ONE launch of the concat + linear gather-GEMM over a (token tile, slot) grid
//              (mot_concat16.hip: u is never built, W is read in place, the norm is its epilogue); everything else per slot and
//              slab: the concat operand (mot_embed.hip), the product (launch_product_nt), and the row pass of mot_lincore.hip;
//   backward   per slot over one workspace: dy from the saved output and row factors (mot_lincore.hip), du = dy W and dW += dy^T u
//              (launch_product_nn / _tn) with u gathered again slab by slab, the byte part of du through the LDS fixed-point sums of the byte
//              value embeddings (mot_bytecat.hip), the token part through the order, canon, slices and rows kernels of the token
//              value embeddings (mot_values.hip) from fp32 rows: every token-table gradient is written once in the tables' dtype.
#include <float.h>

#include "mot_lincore.hpp"
#include "mot_mix.hpp"

namespace mot {

constexpr int64_t kVmSlab = 16384;   // rows of u (and of dy, du's byte part) per slab: 64 MiB of bf16 at K 2048
constexpr int kVmMaxDim = kRowMaxDim;   // the row passes keep a row of out_dim columns in registers (mot_lincore.hip)
constexpr int kVmSlots = MOT_VALUE_MIX_MAX_SLOTS;

// ------------------------------------------------------------------------------------------ validation (no HIP call)

// everything that does not need the pointers: also what the size query runs
static int value_mix_check_shape(const MotValueMixDesc *d, bool backward) {
    if (!d) return set_error(MOT_EINVAL, "value_mix: null descriptor");
    if (d->struct_size != sizeof(MotValueMixDesc))
        return set_error(MOT_EINVAL, "value_mix: struct_size %u != %zu (ABI mismatch)", d->struct_size, sizeof(MotValueMixDesc));
    if (d->dtype != MOT_F32 && d->dtype != MOT_BF16) return set_error(MOT_EINVAL, "value_mix: bad dtype %d", d->dtype);
    if (d->n_slots < 1 || d->n_slots > kVmSlots) return set_error(MOT_EUNSUPPORTED, "value_mix: n_slots %d outside [1, %d]", d->n_slots, kVmSlots);
    if (d->n_rows < 0 || d->tokens_per_row < 0) return set_error(MOT_ESHAPE, "value_mix: negative shape");
    if (int rc = check_id_source_shape("value_mix", id_source_of(*d), backward)) return rc;
    if (d->tok_rows <= 0 || d->byte_rows <= 0 || d->token_dim <= 0 || d->byte_dim <= 0 || d->out_dim <= 0)
        return set_error(MOT_ESHAPE, "value_mix: empty table (tok %lld x %d, byte %lld x %d, out_dim %d)", (long long)d->tok_rows, d->token_dim,
                         (long long)d->byte_rows, d->byte_dim, d->out_dim);
    const int vec = d->dtype == MOT_BF16 ? 8 : 4;
    if (d->token_dim % vec) return set_error(MOT_EUNSUPPORTED, "value_mix: token_dim %d must be a multiple of %d elements (16 bytes)", d->token_dim, vec);
    if (d->byte_dim % vec) return set_error(MOT_EUNSUPPORTED, "value_mix: byte_dim %d must be a multiple of %d elements (16 bytes)", d->byte_dim, vec);
    if (d->out_dim % vec) return set_error(MOT_EUNSUPPORTED, "value_mix: out_dim %d must be a multiple of %d elements (16 bytes)", d->out_dim, vec);
    const int64_t K = d->token_dim + (int64_t)d->bpt * d->byte_dim;
    if (K > kVmMaxDim) return set_error(MOT_EUNSUPPORTED, "value_mix: K = token_dim + bpt*byte_dim = %lld above %d is not built", (long long)K, kVmMaxDim);
    if (d->out_dim > kVmMaxDim) return set_error(MOT_EUNSUPPORTED, "value_mix: out_dim %d above %d is not built", d->out_dim, kVmMaxDim);
    if (int rc = check_id_source_limits("value_mix", id_source_of(*d))) return rc;
    if (d->byte_rows > 0x7fffffffLL / d->byte_dim) return set_error(MOT_ESHAPE, "value_mix: byte tables of %lld rows", (long long)d->byte_rows);
    if (backward && d->tok_rows >= (1 << 21) - 1)
        return set_error(MOT_EUNSUPPORTED, "value_mix_bwd: token tables of %lld rows (>= 2^21 - 1, the token order's limit) are not built", (long long)d->tok_rows);
    return MOT_OK;
}

// what concat16_usable looks at, for slot j (j < 0: the shapes only)
static MotEmbedMixDesc vm_mix_desc(const MotValueMixDesc &d, int j, float eps) {
    MotEmbedMixDesc e{};
    e.struct_size = sizeof(MotEmbedMixDesc); e.dtype = d.dtype; e.mode = MOT_MIX_CONCAT_LINEAR;
    e.n_rows = d.n_rows; e.tokens_per_row = d.tokens_per_row; e.bpt = d.bpt; e.tokens = d.tokens; e.id_source = MOT_IDS_GIVEN;
    e.tok_rows = d.tok_rows; e.tok_dim = d.token_dim; e.byte_dim = d.byte_dim; e.byte_rows = d.byte_rows;
    e.model_dim = d.out_dim; e.norm_out = d.norm_out; e.eps = eps; e.status = d.status;
    if (j >= 0) { e.tok_table = d.slot[j].tok_table; e.byte_table = d.slot[j].byte_table; e.weight = d.slot[j].weight; e.out = d.slot[j].out; }
    return e;
}
// the one-launch gather-GEMM takes the forward (by shape: every pointer of a valid call is 16-byte aligned)
static bool vm_one_launch(const MotValueMixDesc &d) { return d.dtype == MOT_BF16 && concat16_usable(vm_mix_desc(d, -1, 0.f)); }

// forward workspace: [u: slab rows x K, unless the gather-GEMM runs][ids padded | pulled: N * bpt int64 each (FROM_TTB)]
struct VmFwdLayout { size_t u, ids, total; };
static VmFwdLayout vm_fwd_layout(const MotValueMixDesc &d) {
    const size_t N = (size_t)(d.n_rows * d.tokens_per_row), K = (size_t)d.token_dim + (size_t)d.bpt * d.byte_dim, esz = d.dtype == MOT_BF16 ? 2 : 4;
    const size_t ns = N < (size_t)kVmSlab ? N : (size_t)kVmSlab;
    VmFwdLayout L;
    Arena ar;
    L.u = ar.take(vm_one_launch(d) ? 0 : ns * K * esz);
    L.ids = ar.take(d.id_source == MOT_IDS_FROM_TTB ? 2 * N * d.bpt * sizeof(int64_t) : 0);
    L.total = ar.o;
    return L;
}

// backward workspace, ONE slot's rows whatever n_slots is:
// [token sums: order, canon, pieces][du token part: N x token_dim fp32][du byte part: slab x bpt*byte_dim fp32][u: slab x K][dy: slab x out_dim][bf16: W^T]
struct VmBwdLayout { size_t sums, dut, dub, u, dy, wt16, total; int64_t slab; };
static VmBwdLayout vm_bwd_layout(const MotValueMixDesc &d) {
    const size_t N = (size_t)(d.n_rows * d.tokens_per_row), Dt = (size_t)d.token_dim, Kb = (size_t)d.bpt * d.byte_dim, K = Dt + Kb, Do = (size_t)d.out_dim;
    const bool bf = d.dtype == MOT_BF16;
    const size_t esz = bf ? 2 : 4;
    VmBwdLayout L;
    L.slab = (int64_t)(N < (size_t)kVmSlab ? N : (size_t)kVmSlab);
    const size_t ns = (size_t)L.slab;
    Arena ar;
    L.sums = ar.take(token_sums_ws_bytes((int64_t)N, d.tok_rows, d.token_dim, d.dtype));
    L.dut = ar.take(N * Dt * 4);
    L.dub = ar.take(ns * Kb * 4);
    L.u = ar.take(ns * K * esz);
    L.dy = ar.take(d.norm_out ? ns * Do * esz : 0);
    L.wt16 = ar.take(bf ? K * Do * 2 : 0);
    L.total = ar.o;
    return L;
}

size_t value_mix_workspace_bytes(const MotValueMixDesc *d, bool backward) {
    if (value_mix_check_shape(d, backward)) return 0;
    if (d->n_rows == 0 || d->tokens_per_row == 0) return 0;
    return backward ? vm_bwd_layout(*d).total : vm_fwd_layout(*d).total;
}

int value_mix_check(const MotValueMixDesc *d, const MotValueMixGrads *g, bool backward) {
    if (int rc = value_mix_check_shape(d, backward)) return rc;
    if (backward && (!g || g->struct_size != sizeof(MotValueMixGrads)))
        return set_error(MOT_EINVAL, "value_mix_bwd: grads struct missing or struct_size mismatch");
    if (!d->tokens) return set_error(MOT_EINVAL, "value_mix: tokens must be non-null");
    uintptr_t align = 0;
    for (int j = 0; j < d->n_slots; ++j) {
        const MotValueMixSlot &s = d->slot[j];
        if (!s.tok_table || !s.byte_table || !s.weight) return set_error(MOT_EINVAL, "value_mix: slot %d has a null tok_table, byte_table or weight", j);
        align |= (uintptr_t)s.tok_table | (uintptr_t)s.byte_table | (uintptr_t)s.weight | (uintptr_t)s.out;
        if (!backward) {
            if (!s.out) return set_error(MOT_EINVAL, "value_mix: slot %d has a null out", j);
            continue;
        }
        const MotValueMixGradSlot &q = g->slot[j];
        if (!q.grad_out) continue;
        if (!q.d_tok || !q.d_byte || !q.d_weight) return set_error(MOT_EINVAL, "value_mix_bwd: slot %d has a grad_out but a null d_tok, d_byte or d_weight", j);
        if (d->norm_out && (!s.out || !s.out_row_rnorm)) return set_error(MOT_EINVAL, "value_mix_bwd: slot %d needs the forward's out and out_row_rnorm", j);
        align |= (uintptr_t)q.grad_out | (uintptr_t)q.d_tok | (uintptr_t)q.d_byte | (uintptr_t)q.d_weight;
    }
    if (align & 15) return set_error(MOT_EINVAL, "value_mix: tables, weights, outputs and gradients must be 16-byte aligned");
    if (int rc = check_id_source_ptrs("value_mix", id_source_of(*d), "out_ids needs")) return rc;
    if (d->n_rows == 0 || d->tokens_per_row == 0) return MOT_OK;
    return check_workspace("value_mix", backward, d->workspace, d->workspace_bytes, backward ? vm_bwd_layout(*d).total : vm_fwd_layout(*d).total);
}

// ------------------------------------------------------------------------------------------ forward
int launch_value_mix_fwd(const MotValueMixDesc &d, hipStream_t stream) {
    const int64_t N = d.n_rows * d.tokens_per_row, slots = N * d.bpt;
    const int Dt = d.token_dim, Db = d.byte_dim, bpt = d.bpt, K = Dt + bpt * Db, Do = d.out_dim;
    const bool bf = d.dtype == MOT_BF16;
    const size_t esz = bf ? 2 : 4;
    const float eps = d.eps > 0.f ? d.eps : FLT_EPSILON;
    const VmFwdLayout L = vm_fwd_layout(d);
    char *ws = (char *)d.workspace;
    int rc;
    // 1. the byte ids, ONCE for all slots: given, or the loader's two index kernels (tokens_to_bytes, pull)
    const int64_t *ids = d.ids;
    if (d.id_source == MOT_IDS_FROM_TTB) {
        int64_t *ws_ids = (int64_t *)(ws + L.ids);
        const bool pull = d.pull_dir != MOT_PULL_NONE;
        int64_t *padded = (!pull && d.out_ids) ? d.out_ids : ws_ids;   // the one id output takes the ids the tables are read with
        int64_t *pulled = d.out_ids ? d.out_ids : ws_ids + slots;
        if ((rc = launch_ids_from_ttb(id_source_of(d), padded, pulled, &ids, stream))) return rc;
    }
    // 2a. bf16 at the gather-GEMM's shapes: one launch over (token tile, slot)
    if (vm_one_launch(d)) {
        Concat16Slots S{};
        S.n = d.n_slots;
        for (int j = 0; j < d.n_slots; ++j) {
            S.tok_table[j] = d.slot[j].tok_table; S.byte_table[j] = d.slot[j].byte_table; S.weight[j] = d.slot[j].weight;
            S.out[j] = d.slot[j].out; S.row_rnorm[j] = d.slot[j].out_row_rnorm;
        }
        return launch_concat16_slots(vm_mix_desc(d, 0, eps), S, d.tokens, ids, N, stream);
    }
    // 2b. per slot, slab by slab: u, y = u W^T into `out`, then the row pass in place
    char *u = ws + L.u;
    for (int j = 0; j < d.n_slots; ++j) {
        const MotValueMixSlot &s = d.slot[j];
        for (int64_t r0 = 0; r0 < N; r0 += kVmSlab) {
            const int64_t n = N - r0 < kVmSlab ? N - r0 : kVmSlab;
            if ((rc = launch_concat_rows(d.tokens + r0, ids + r0 * bpt, n, s.tok_table, d.tok_rows, Dt, s.byte_table, d.byte_rows, Db, bpt, 0, nullptr, eps, u,
                                         K, 0, Dt, d.status, d.dtype, stream))) return rc;
            char *out = (char *)s.out + (size_t)r0 * Do * esz;
            if ((rc = launch_product_nt(d.dtype, u, K, n, s.weight, K, K, Do, out, Do, bf, nullptr, false, stream))) return rc;
            // bf16: y arrives rounded by the product and r y is rounded on store -- the roundings of the reference's bf16 run
            if (d.norm_out && (rc = launch_rows_finish(out, n, Do, 1, eps, s.out_row_rnorm ? s.out_row_rnorm + r0 : nullptr, d.dtype, stream))) return rc;
        }
    }
    return MOT_OK;
}

// ------------------------------------------------------------------------------------------ backward
int launch_value_mix_bwd(const MotValueMixDesc &d, const MotValueMixGrads &gr, hipStream_t stream) {
    const int64_t N = d.n_rows * d.tokens_per_row;
    const int Dt = d.token_dim, Db = d.byte_dim, bpt = d.bpt, Kb = bpt * Db, K = Dt + Kb, Do = d.out_dim;
    const bool bf = d.dtype == MOT_BF16;
    const size_t esz = bf ? 2 : 4;
    const float eps = d.eps > 0.f ? d.eps : FLT_EPSILON;
    const VmBwdLayout L = vm_bwd_layout(d);
    char *ws = (char *)d.workspace;
    float *dut = (float *)(ws + L.dut), *dub = (float *)(ws + L.dub);
    char *u = ws + L.u, *dyws = ws + L.dy;
    __bf16 *wt16 = (__bf16 *)(ws + L.wt16);
    int rc;
    bool first = true;   // the token order and the canonical positions are made by the first slot that has a gradient
    for (int j = 0; j < d.n_slots; ++j) {
        const MotValueMixSlot &s = d.slot[j];
        const MotValueMixGradSlot &q = gr.slot[j];
        if (!q.grad_out) continue;
        // du[n][k] = sum_m dy[n][m] W[m][k]: fp32 reads W [out_dim, K] itself, the bf16 launcher its k-major copy W^T [K, out_dim];
        // Wb is the byte part of either, columns [Dt, K) of W or rows [Dt, K) of W^T
        if (bf && (rc = launch_transpose_bf16(s.weight, Do, K, wt16, stream))) return rc;
        const void *Wd = bf ? (const void *)wt16 : s.weight, *Wb = bf ? (const void *)(wt16 + (size_t)Dt * Do) : (const float *)s.weight + Dt;
        const int ldw = bf ? Do : K;
        for (int64_t r0 = 0; r0 < N; r0 += L.slab) {
            const int64_t n = N - r0 < L.slab ? N - r0 : L.slab;
            const char *g = (const char *)q.grad_out + (size_t)r0 * Do * esz;
            const int64_t *ids = d.ids + r0 * bpt;
            // 1. u again; 2. dy; 3. du = dy W, token part for the whole batch, byte part for the slab; 4. d_weight += dy^T u
            if ((rc = launch_concat_rows(d.tokens + r0, ids, n, s.tok_table, d.tok_rows, Dt, s.byte_table, d.byte_rows, Db, bpt, 0, nullptr, eps, u, K, 0, Dt,
                                         d.status, d.dtype, stream))) return rc;
            const char *dy = g;   // without the norm dy is g
            if (d.norm_out) {   // bf16 tensors: dy in bf16, the operand of the two bf16 products
                const char *x = (const char *)s.out + (size_t)r0 * Do * esz;
                if ((rc = launch_rows_norm_bwd(g, x, s.out_row_rnorm + r0, n, Do, 1, dyws, Do, nullptr, 0, d.dtype, stream))) return rc;
                dy = dyws;
            }
            if ((rc = launch_product_nn(d.dtype, dy, Do, n, Wd, ldw, Do, Dt, dut + r0 * Dt, Dt, stream))) return rc;
            if ((rc = launch_product_nn(d.dtype, dy, Do, n, Wb, ldw, Do, Kb, dub, Kb, stream))) return rc;
            if ((rc = launch_product_tn(d.dtype, dy, Do, Do, u, K, K, n, (float *)q.d_weight, K, stream))) return rc;
            // 5. d_byte += the byte part, as the gradient of an un-normed fp32 byte_cat over this slab
            MotByteCatDesc c{};
            c.struct_size = sizeof(MotByteCatDesc); c.dtype = MOT_F32; c.n_rows = 1; c.tokens_per_row = n; c.bpt = bpt; c.byte_dim = Db; c.n_out = 1;
            c.id_source = MOT_IDS_GIVEN; c.ids = ids; c.eps = eps; c.status = d.status;
            c.slot[0].table = s.byte_table; c.slot[0].rows = d.byte_rows; c.slot[0].norm = 0; c.slot[0].dtype = MOT_F32;
            MotByteCatGrads cg{};
            cg.struct_size = sizeof(MotByteCatGrads);
            cg.slot[0].grad_out = dub; cg.slot[0].d_table = q.d_byte;
            if ((rc = launch_byte_cat_bwd(c, cg, stream))) return rc;
        }
        // 6. d_tok, written once in the tables' dtype, from the token part of the whole batch over the shared order
        if ((rc = launch_token_sums_f32(d.tokens, N, d.tok_rows, Dt, d.dtype, dut, Dt, q.d_tok, gr.token_order, first, ws + L.sums, d.status, stream))) return rc;
        first = false;
    }
    return MOT_OK;
}

}  // namespace mot
