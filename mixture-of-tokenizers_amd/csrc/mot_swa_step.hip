// mot_swa_step.hip -- one decode step of the Llama character mixer (mot_char_swa_step, gfx950): row t of what mot_char_swa_fwd
// (mot_swa.hip) computes for a sequence, from the newest token and a device-side state, for up to 16 sequences at once.
//
// Rotary cancels (mot_swa.hip), so row t depends on the token at t, the character ids of the tokens t-window+1 .. t and on how
// many of those lie in front of the row's start.  The state keeps exactly that:
//   ring [n_rows, window, c_v] int32   the characters of source position s sit in slot s % window
//   pos  [n_rows] int64                tokens of the row seen so far
// Three launches, nothing read on the host, no atomics on a value (only the status word), every sum in a fixed order:
//   swa_step_query   the LAST workgroup is the state kernel: t = pos[b], the new token's characters (row tokens[b] of the
//                    token -> character table, or the caller's ids) into slot t % window, pos[b] = t + 1.  No other workgroup
//                    of this launch reads the state; the two later launches see pos[b] - 1: one t for the whole call.
//                    Every other workgroup stages the R <= 16 gathered, normalised token rows in LDS (R * dim elements) and
//                    computes its slice of q = wq xn: a wave owns four rows of wq at a time, every lane a 16-byte slice of the
//                    reduction (wq is read once), the wave's DPP sum closes each product.
//   swa_step_attn    one wave per (row, head); lane = key (window slot, character slot).  The key / value rows of the at most
//                    64 ids come straight from the fp32 tables mot_char_swa_fwd left in kv_tables (L2): nothing is staged.
//                    Softmax by two wave reductions; y with lane = (key group, four elements of the head).
//   swa_step_out     out = wo y + residuals, the same skinny product with y in LDS; the residual terms are added per output
//                    element by the lane that stores it.
// MOT_BF16: the tables, wq and wo are bf16 and read in place; xn, q, k, v, y and the output of wo are rounded to bf16 where
// launch_char_swa (matmul_dtype = io_dtype = MOT_BF16) rounds them, softmax and sums stay fp32, the residuals are added to the
// widened bf16 output of wo in fp32 with one rounding (swa_residual_bf16_kernel).
#include "mot_step.hpp"

namespace mot {
namespace {

struct StepArgs {
    int n_rows, c_v, window, n_heads, dim, hdim, version, char_rows;
    int64_t tok_rows;
    const int64_t *tokens, *char_ids_new;
    const int32_t *tok_chars;
    const void *tok_table, *char_table, *wq, *wo;
    const float *attn_norm_w, *lambda_tok, *lambda_char, *ktab, *vtab;
    int32_t *ring;
    int64_t *pos;
    float *q, *y;    // workspace: [n_rows, hdim] each (bf16 mode: the bf16 values, held as floats)
    void *out;
    uint32_t *status;
    float eps;
};

__device__ __forceinline__ int64_t step_token(const StepArgs &A, int r) {   // clamped; the state workgroup raises the flag
    const int64_t id = A.tokens[r];
    return (uint64_t)id < (uint64_t)A.tok_rows ? id : 0;
}

template <typename T, int R>
__global__ __launch_bounds__(kStepThreads) void swa_step_query(StepArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char step_smem[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (blockIdx.x == gridDim.x - 1) {
        // ---- the state: one wave per row, lane = character slot
        for (int b = wave; b < A.n_rows; b += kStepWaves) {
            const int64_t t = A.pos[b];
            int64_t tok = A.tokens[b];
            if ((uint64_t)tok >= (uint64_t)A.tok_rows) {
                if (A.status && lane == 0) atomicOr(A.status, kStatusTokenOor);
                tok = 0;
            }
            if (lane < A.c_v) {
                const int64_t c = A.tok_chars ? (int64_t)A.tok_chars[tok * A.c_v + lane] : A.char_ids_new[(int64_t)b * A.c_v + lane];
                int id = (int)c;
                if ((uint64_t)c >= (uint64_t)A.char_rows) {
                    if (A.status) atomicOr(A.status, kStatusByteOor);
                    id = 0;
                }
                const int slot = (int)(((t % A.window) + A.window) % A.window);
                A.ring[((int64_t)b * A.window + slot) * A.c_v + lane] = id;
            }
            if (lane == 0) A.pos[b] = t + 1;
        }
        return;
    }
    // ---- xn = RMSNorm_a(E_tok[token]) of every row into LDS, as a tensor of type T (rows_rmsnorm_w_kernel's arithmetic)
    T *xs = (T *)step_smem;   // [R][dim]
    const int nv = A.dim >> 2;
    for (int r = wave; r < R; r += kStepWaves) {
        T *o = xs + r * A.dim;
        if (r >= A.n_rows) {
            for (int j = lane; j < A.dim; j += 64) o[j] = (T)0.f;
            continue;
        }
        const T *p = (const T *)A.tok_table + step_token(A, r) * A.dim;
        float ss = 0.f;
        for (int j = lane; j < nv; j += 64) {
            const float4v v = Elem<T>::load4(p + 4 * j);
            ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
        }
        ss = wave_sum(ss);
        const float rs = 1.0f / sqrtf(ss / (float)A.dim + A.eps);
        for (int j = lane; j < nv; j += 64) {
            const float4v v = Elem<T>::load4(p + 4 * j), w = *(const float4v *)(A.attn_norm_w + 4 * j);
            const float4v x = (v * rs) * w;
            if constexpr (sizeof(T) == 2) *(bf16x4v *)(o + 4 * j) = __builtin_convertvector(x, bf16x4v);
            else *(float4v *)(o + 4 * j) = x;
        }
    }
    __syncthreads();
    // ---- q = wq xn: groups of four rows of wq, one group per wave at a time
    const int groups = A.hdim / kStepCls, nblk = gridDim.x - 1;
    for (int g = blockIdx.x * kStepWaves + wave; g < groups; g += nblk * kStepWaves)
        step_products<T, R>(xs, (const T *)A.wq, A.dim, g * kStepCls, A.n_rows,
                            [&](int r, int c, float v) { A.q[(int64_t)r * A.hdim + c] = step_round<T>(v); });
}

// One wave per (row b, head h).  Slot w of the ring holds the newest source position s <= t with s % window == w; s < 0: a padding key.
template <typename T, int HDL>
__global__ __launch_bounds__(kThreads) void swa_step_attn(StepArgs A) {
    constexpr int HD = 64 * HDL, QUADS = HD / 4, GROUPS = 64 / QUADS;
    const int lane = threadIdx.x & 63;
    const int item = blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (item >= A.n_rows * A.n_heads) return;
    const int b = item / A.n_heads, h = item - b * A.n_heads;
    const int64_t t = A.pos[b] - 1;              // the state workgroup of the first launch has advanced pos
    const int nkeys = A.window * A.c_v;
    const int w = lane / A.c_v;
    const bool is_key = lane < nkeys;
    int id = 0;
    bool real = false;
    if (is_key) {
        const int back = (int)((((t - w) % A.window) + A.window) % A.window);   // t - s
        real = t - back >= 0;
        if (real) {
            const int raw = A.ring[((int64_t)b * A.window) * A.c_v + lane];      // slot w, character lane - w * c_v
            id = raw;
            if ((unsigned)raw >= (unsigned)A.char_rows) {
                if (A.status) atomicOr(A.status, kStatusByteOor);
                id = 0;
            }
        }
    }
    // ---- score of the lane's key: four chains over the head's elements, in element order
    const float *qrow = A.q + (int64_t)b * A.hdim + h * HD;
    const float *krow = A.ktab + (int64_t)id * A.hdim + h * HD;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
    for (int d4 = 0; d4 < QUADS; ++d4) {
        const float4v k = *(const float4v *)(krow + 4 * d4), q = *(const float4v *)(qrow + 4 * d4);
        s0 = __builtin_fmaf(q.x, step_round<T>(k.x), s0);
        s1 = __builtin_fmaf(q.y, step_round<T>(k.y), s1);
        s2 = __builtin_fmaf(q.z, step_round<T>(k.z), s2);
        s3 = __builtin_fmaf(q.w, step_round<T>(k.w), s3);
    }
    const float s = real ? ((s0 + s1) + (s2 + s3)) * (1.0f / sqrtf((float)HD)) : 0.f;   // a padding key: the zero vector
    const float m = wave_max(is_key ? s : -INFINITY);
    const float e = is_key ? expf(s - m) : 0.f;
    const float z = wave_sum(e);                   // (every lane takes part: outside any lane-dependent condition)
    const float p = real ? e / z : 0.f;            // a padding key keeps its place in the sum and has the zero value
    // ---- y = sum_j p_j v_j: lane = (key group g, element quad dq); group g takes the keys g, g + GROUPS, ..
    const int g = lane / QUADS, dq = lane - g * QUADS;
    float4v acc = {0.f, 0.f, 0.f, 0.f};
    for (int j = g; j < 64; j += GROUPS) {
        const float pj = __shfl(p, j, 64);
        const int idj = __shfl(id, j, 64);
        const float4v v = *(const float4v *)(A.vtab + (int64_t)idj * A.hdim + h * HD + 4 * dq);
        acc.x = __builtin_fmaf(pj, step_round<T>(v.x), acc.x);
        acc.y = __builtin_fmaf(pj, step_round<T>(v.y), acc.y);
        acc.z = __builtin_fmaf(pj, step_round<T>(v.z), acc.z);
        acc.w = __builtin_fmaf(pj, step_round<T>(v.w), acc.w);
    }
#pragma unroll
    for (int o = QUADS; o < 64; o <<= 1) {
        acc.x += __shfl_xor(acc.x, o, 64); acc.y += __shfl_xor(acc.y, o, 64);
        acc.z += __shfl_xor(acc.z, o, 64); acc.w += __shfl_xor(acc.w, o, 64);
    }
    if (lane < QUADS) {
        float *yo = A.y + (int64_t)b * A.hdim + h * HD + 4 * dq;
        *(float4v *)yo = float4v{step_round<T>(acc.x), step_round<T>(acc.y), step_round<T>(acc.z), step_round<T>(acc.w)};
    }
}

template <typename T, int R>
__global__ __launch_bounds__(kStepThreads) void swa_step_out(StepArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char step_smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    T *ys = (T *)step_smem;   // [R][hdim]
    for (int i = threadIdx.x; i < R * A.hdim; i += kStepThreads) ys[i] = i < A.n_rows * A.hdim ? (T)A.y[i] : (T)0.f;   // (bf16: exact, y holds bf16 values)
    __syncthreads();
    const float lt = A.lambda_tok ? *A.lambda_tok : 1.f, lc = (A.lambda_char ? *A.lambda_char : 1.f) / (float)A.c_v;
    const int groups = A.dim / kStepCls;
    for (int g = blockIdx.x * kStepWaves + wave; g < groups; g += gridDim.x * kStepWaves)
        step_products<T, R>(ys, (const T *)A.wo, A.hdim, g * kStepCls, A.n_rows, [&](int r, int c, float v) {
            float x = step_round<T>(v);           // the output of wo: a bf16 tensor in bf16 mode
            if (A.version != MOT_SWA_NO_RESIDUAL) {
                const float tok = Elem<T>::load1((const T *)A.tok_table + step_token(A, r) * A.dim + c);
                if (A.version == MOT_SWA_ONE_RESIDUAL) {
                    x += tok;
                } else {
                    x += lt * tok;
                    const int64_t t = A.pos[r] - 1;
                    const int32_t *ids = A.ring + ((int64_t)r * A.window + (int)(((t % A.window) + A.window) % A.window)) * A.c_v;
                    float msum = 0.f;
                    for (int k = 0; k < A.c_v; ++k) {
                        const int id = ids[k];
                        msum += Elem<T>::load1((const T *)A.char_table + (int64_t)((unsigned)id < (unsigned)A.char_rows ? id : 0) * A.dim + c);
                    }
                    x += lc * msum;
                }
            }
            Elem<T>::store1((T *)A.out + (int64_t)r * A.dim + c, x);
        });
}

struct StepGeom {
    int R, hdim;
    bool bf16;
    size_t q, y, total;   // workspace offsets in bytes
};

// every refusal of the call but the workspace's, before any HIP call (the size query makes the same checks)
int step_check(const MotCharSwaStepDesc *d, StepGeom *out, const char *fn) {
    if (!d) return set_error(MOT_EINVAL, "%s: null descriptor", fn);
    if (d->struct_size != sizeof(MotCharSwaStepDesc))
        return set_error(MOT_EINVAL, "%s: struct_size %u != %zu (ABI mismatch)", fn, d->struct_size, sizeof(MotCharSwaStepDesc));
    if (d->dtype != MOT_F32 && d->dtype != MOT_BF16) return set_error(MOT_EINVAL, "%s: bad dtype %d", fn, d->dtype);
    if (d->reserved0 || d->reserved1) return set_error(MOT_EINVAL, "%s: reserved fields must be 0", fn);
    if (d->n_rows < 0) return set_error(MOT_ESHAPE, "%s: negative n_rows", fn);
    if (d->n_rows > kStepMaxRows)
        return set_error(MOT_EUNSUPPORTED, "%s: n_rows %d above %d: the step is built for a few rows, use mot_char_swa_fwd", fn, d->n_rows, kStepMaxRows);
    if (d->c_v < 1 || d->window < 1 || d->c_v * (int64_t)d->window > 64)
        return set_error(MOT_EUNSUPPORTED, "%s: window %d x %d characters must give 1..64 keys per query", fn, d->window, d->c_v);
    if (d->head_dim != 64 && d->head_dim != 128) return set_error(MOT_EUNSUPPORTED, "%s: head_dim %d (64 and 128 are built)", fn, d->head_dim);
    if (d->n_heads < 1 || d->n_heads > (1 << 16) || d->dim < 4 || (d->dim & 3))
        return set_error(MOT_ESHAPE, "%s: n_heads %d / dim %d (dim must be a multiple of 4)", fn, d->n_heads, d->dim);
    if (d->dtype == MOT_BF16 && (d->dim & 7)) return set_error(MOT_EUNSUPPORTED, "%s: bf16 needs dim %d to be a multiple of 8", fn, d->dim);
    if (d->version < MOT_SWA_NO_RESIDUAL || d->version > MOT_SWA_TWO_RESIDUAL) return set_error(MOT_EINVAL, "%s: bad version %d", fn, d->version);
    if (d->tok_rows <= 0 || d->char_rows <= 0) return set_error(MOT_ESHAPE, "%s: empty table", fn);
    StepGeom &g = *out;
    g.bf16 = d->dtype == MOT_BF16;
    g.hdim = d->n_heads * d->head_dim;
    g.R = d->n_rows <= 1 ? 1 : d->n_rows <= 2 ? 2 : d->n_rows <= 4 ? 4 : d->n_rows <= 8 ? 8 : 16;
    const size_t e = g.bf16 ? 2 : 4, widest = (size_t)(d->dim > g.hdim ? d->dim : g.hdim);
    if ((size_t)g.R * widest * e > kStepMaxLds)
        return set_error(MOT_EUNSUPPORTED, "%s: %d rows x %zu elements need more than %zu B of LDS, use mot_char_swa_fwd", fn, g.R, widest, kStepMaxLds);
    {
        if (!d->tokens || !d->tok_table || !d->char_table || !d->attn_norm_w || !d->wq || !d->wo || !d->ring || !d->pos || !d->out)
            return set_error(MOT_EINVAL, "%s: tokens/tables/attn_norm_w/wq/wo/ring/pos/out must be non-null", fn);
        if (!d->kv_tables)
            return set_error(MOT_EINVAL, "%s: null kv_tables: the step needs the key / value tables a mot_char_swa_fwd call filled", fn);
        if (!d->tok_chars == !d->char_ids_new) return set_error(MOT_EINVAL, "%s: exactly one of tok_chars and char_ids_new must be given", fn);
        if (((uintptr_t)d->tok_table & 15) || ((uintptr_t)d->char_table & 15) || ((uintptr_t)d->wq & 15) || ((uintptr_t)d->wo & 15) ||
            ((uintptr_t)d->attn_norm_w & 15) || ((uintptr_t)d->kv_tables & 15))
            return set_error(MOT_EUNSUPPORTED, "%s: tables, weights and kv_tables must be 16-byte aligned", fn);
    }
    Arena a;
    g.q = a.take((size_t)d->n_rows * g.hdim * sizeof(float));
    g.y = a.take((size_t)d->n_rows * g.hdim * sizeof(float));
    g.total = a.o;
    return MOT_OK;
}

template <typename T, int R>
int step_run(const StepArgs &A, int head_dim, hipStream_t stream) {
    static std::atomic<uint64_t> lds_q{0}, lds_o{0};
    const size_t lq = (size_t)R * A.dim * sizeof(T), lo = (size_t)R * A.hdim * sizeof(T);
    if (lq > (48u << 10))
        if (int rc = ensure_max_dyn_lds((const void *)swa_step_query<T, R>, lds_q, "swa_step_query")) return rc;
    if (lo > (48u << 10))
        if (int rc = ensure_max_dyn_lds((const void *)swa_step_out<T, R>, lds_o, "swa_step_out")) return rc;
    const int qblocks = (A.hdim / kStepCls + kStepWaves - 1) / kStepWaves, oblocks = (A.dim / kStepCls + kStepWaves - 1) / kStepWaves;
    hipLaunchKernelGGL((swa_step_query<T, R>), dim3((unsigned)qblocks + 1), dim3(kStepThreads), lq, stream, A);
    if (int rc = check_launch("swa_step_query")) return rc;
    const dim3 agrid((unsigned)((A.n_rows * A.n_heads + kWaves - 1) / kWaves));
    if (head_dim == 64) hipLaunchKernelGGL((swa_step_attn<T, 1>), agrid, dim3(kThreads), 0, stream, A);
    else hipLaunchKernelGGL((swa_step_attn<T, 2>), agrid, dim3(kThreads), 0, stream, A);
    if (int rc = check_launch("swa_step_attn")) return rc;
    hipLaunchKernelGGL((swa_step_out<T, R>), dim3((unsigned)oblocks), dim3(kStepThreads), lo, stream, A);
    return check_launch("swa_step_out");
}

template <typename T>
int step_rows(const StepArgs &A, int R, int head_dim, hipStream_t stream) {
    return R == 1 ? step_run<T, 1>(A, head_dim, stream)
         : R == 2 ? step_run<T, 2>(A, head_dim, stream)
         : R == 4 ? step_run<T, 4>(A, head_dim, stream)
         : R == 8 ? step_run<T, 8>(A, head_dim, stream)
                  : step_run<T, 16>(A, head_dim, stream);
}

}  // namespace

size_t char_swa_step_workspace_bytes(const MotCharSwaStepDesc *d) {
    StepGeom g;
    if (step_check(d, &g, "mot_char_swa_step_workspace_bytes") || d->n_rows == 0) return 0;
    return g.total;
}

int launch_char_swa_step(const MotCharSwaStepDesc *d, hipStream_t stream) {
    static const char fn[] = "mot_char_swa_step";
    StepGeom g;
    if (int rc = step_check(d, &g, fn)) return rc;
    if (d->n_rows == 0) return MOT_OK;
    if (int rc = check_workspace(fn, false, d->workspace, d->workspace_bytes, g.total)) return rc;
    StepArgs A{};
    A.n_rows = d->n_rows; A.c_v = d->c_v; A.window = d->window; A.n_heads = d->n_heads; A.dim = d->dim; A.hdim = g.hdim;
    A.version = d->version; A.char_rows = d->char_rows; A.tok_rows = d->tok_rows;
    A.tokens = d->tokens; A.char_ids_new = d->char_ids_new; A.tok_chars = d->tok_chars;
    A.tok_table = d->tok_table; A.char_table = d->char_table; A.wq = d->wq; A.wo = d->wo;
    A.attn_norm_w = d->attn_norm_w;
    const bool two = d->version == MOT_SWA_TWO_RESIDUAL;
    A.lambda_tok = two ? d->lambda_tok : nullptr; A.lambda_char = two ? d->lambda_char : nullptr;
    A.ktab = d->kv_tables; A.vtab = d->kv_tables + (size_t)d->char_rows * g.hdim;
    A.ring = d->ring; A.pos = d->pos;
    A.q = (float *)((unsigned char *)d->workspace + g.q); A.y = (float *)((unsigned char *)d->workspace + g.y);
    A.out = d->out; A.status = d->status;
    A.eps = d->norm_eps > 0.f ? d->norm_eps : 1e-5f;
    return g.bf16 ? step_rows<__bf16>(A, g.R, d->head_dim, stream) : step_rows<float>(A, g.R, d->head_dim, stream);
}

}  // namespace mot
