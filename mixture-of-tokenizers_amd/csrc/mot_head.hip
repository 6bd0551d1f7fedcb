// mot_head.hip -- the byte output head of a mixout run (scaled-pre-train/train_gpt.py:618-623 with identity ByteSelfAttn layers):
//   h = repeat(x) | rearrange(x);  h = h + norm(h) (n_layer_out times);  l = norm(h) W^T;  z = 30 sigmoid(l / 7.5);  loss = CE(z, y)
//
// With identity layers every step scales a row by one number, so norm(h_L) = c(m0) x_row with m0 = mean(x_row^2) (row_scale).
// A *row* is what the contraction sees: a token row of x (K = model_dim) in copy mode, whose bpt byte rows carry identical logits,
// or a byte row of the contiguous view x as (n_tokens * bpt, model_dim / bpt) in split mode.  Row r has `tpr` targets (bpt in copy
// mode, 1 in split mode), and with p = softmax(z_r), hist_r = the row's target counts per class, M = n_tokens * bpt:
//   loss    = (1 / M) sum_r (tpr lse(z_r) - sum_k z_r[y_rk]),   lse = 30 + log sum exp(z - 30)  (z in (0, 30): no max pass)
//   dL/dl_r = (grad_loss / M) 4 s (1 - s) (tpr p_r - hist_r),  s = sigmoid(l / 7.5)
// A target outside [0, 512) addresses nothing: its term (lse - z[y]) leaves the sum, M stays, MOT_STATUS_TARGET_OOR is raised.
// The rows run in chunks (kChunkBytes of scratch at most): the logits of a chunk, s_r = x_r W^T, are one product on the shared GEMM
// launchers; a wave-per-row epilogue applies c, the softcap and the loss.  The backward recomputes the chunk's logits, writes
// G_r = c_r dL/dl_r (overwriting the logits in fp32, a bf16 copy in bf16), then u = G W (= c dL/dnorm(h)), the row chain
// dx_r = u_r + (dc/dm0) (2 / K) (x_r . u_r / c_r) x_r, and dW += G^T x.  Every buffer of the chunk is bounded by kChunkBytes,
// so no tensor of M x 512 exists in split mode.  The loss is a fixed-order double sum of per-row terms (per-workgroup partials over
// fixed row ranges, then one ordered sum of the partials): the same bits every run.
#include "mot_internal.hpp"
#include "mot_rowloss.hpp"
#include "mot_tile.hpp"

namespace mot {
namespace {

constexpr int kV = 512;                           // rows of W: next_multiple_of_n(458, n=128), the only head the reference builds
constexpr int kMaxK = 2048;
constexpr int64_t kChunkBytes = 48ll << 20;       // per-chunk scratch: logits, bf16 G, u
constexpr float kCap = 30.f, kInvDiv = 1.f / 7.5f;

__device__ __forceinline__ float sigm(float l) { return 1.f / (1.f + __expf(-l * kInvDiv)); }

template <typename T>
__device__ __forceinline__ float row_sumsq(const T *x, int K, int lane) {
    float ss = 0.f;
    for (int k = lane; k < K; k += 64) {
        const float v = (float)x[k];
        ss += v * v;
    }
    return wave_sum(ss);
}

// one wave per row: c, z, lse and the row's loss term; lane j holds classes lane + 64 i
template <typename T>
__global__ __launch_bounds__(kThreads) void head_fwd_rows(const float *__restrict__ S, const T *__restrict__ x, int K, const int64_t *__restrict__ tgt,
                                                          int tpr, int64_t rows, int L, float eps, float *__restrict__ lse, float *__restrict__ cst,
                                                          float *__restrict__ term, uint32_t *status) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (r >= rows) return;
    float c, dc;
    row_scale(row_sumsq(x + r * K, K, lane) / (float)K, L, eps, c, dc);
    const float *s = S + r * kV;
    float z[8], se = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        z[i] = kCap * sigm(c * s[lane + 64 * i]);
        se += __expf(z[i] - kCap);
    }
    const float l = kCap + __logf(wave_sum(se));
    float tz = 0.f;
    int nv = 0;   // targets in range: an out-of-range one never addresses anything, its term is dropped, the status word says so
    for (int k = 0; k < tpr; ++k) {
        const int64_t y = tgt[r * tpr + k];
        if (y < 0 || y >= kV) continue;
        ++nv;
#pragma unroll
        for (int i = 0; i < 8; ++i) tz += (lane + 64 * i == (int)y) ? z[i] : 0.f;
    }
    tz = wave_sum(tz);
    if (lane == 0) {
        lse[r] = l;
        cst[r] = c;
        term[r] = (float)nv * l - tz;
        if (nv < tpr && status) atomicOr(status, (uint32_t)MOT_STATUS_TARGET_OOR);
    }
}

// G_r = c_r dL/dl_r from the row's logits s_r (read before G is written: G may alias S in fp32).  In bf16, G is rounded once to
// bf16 for the two bf16 products that take it, as the reference's logits gradient is a bf16 tensor in that cast.
template <typename TG>
__global__ __launch_bounds__(kThreads) void head_grad_rows(const float *S, const int64_t *__restrict__ tgt, int tpr, int64_t rows, const float *__restrict__ lse,
                                                           const float *__restrict__ cst, const float *__restrict__ grad_loss, float inv_m, TG *G) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float c = cst[r], l = lse[r], go = *grad_loss * inv_m;
    float v[8], cnt[8], nv = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        v[i] = S[r * kV + lane + 64 * i];
        cnt[i] = 0.f;
    }
    for (int k = 0; k < tpr; ++k) {
        const int64_t y = tgt[r * tpr + k];
        if (y < 0 || y >= kV) continue;   // dropped, as in the forward
        nv += 1.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) cnt[i] += (lane + 64 * i == y) ? 1.f : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float sg = sigm(c * v[i]), z = kCap * sg, p = __expf(z - l);
        const float g = go * 4.f * sg * (1.f - sg) * (nv * p - cnt[i]);
        G[r * kV + lane + 64 * i] = (TG)(c * g);
    }
}

// dx_r = u_r + (dc/dm0) (2 / K) (x_r . u_r / c_r) x_r
template <typename T>
__global__ __launch_bounds__(kThreads) void head_chain_rows(const T *__restrict__ x, const float *__restrict__ u, int K, int64_t rows, int L, float eps,
                                                            T *__restrict__ dx) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (r >= rows) return;
    const T *xr = x + r * K;
    const float *ur = u + r * K;
    float ss = 0.f, xu = 0.f;
    for (int k = lane; k < K; k += 64) {
        const float a = (float)xr[k];
        ss += a * a;
        xu += a * ur[k];
    }
    ss = wave_sum(ss);
    xu = wave_sum(xu);
    float c, dc;
    row_scale(ss / (float)K, L, eps, c, dc);
    const float coef = dc * (2.f / (float)K) * xu / c;
    for (int k = lane; k < K; k += 64) dx[r * K + k] = (T)(ur[k] + coef * (float)xr[k]);
}

// WT[k][v] = W[v][k] (bf16), the transposed operand of u = G W on the bf16 launcher
__global__ __launch_bounds__(kThreads) void head_transpose_bf16(const __bf16 *__restrict__ W, int K, __bf16 *__restrict__ WT) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (int64_t)kV * K) return;
    const int v = (int)(i / K), k = (int)(i % K);
    WT[(int64_t)k * kV + v] = W[i];
}

struct HeadGeom {
    int64_t rows;   // R: tokens (copy) or byte rows (split)
    int K;          // row width
    int tpr;        // targets per row
    int64_t M;      // targets in all: n_tokens * bpt
    int64_t chunk;  // rows per chunk
    bool bf16;
    float eps;
};

struct HeadWs {   // carve of the workspace, offsets in bytes
    size_t term, part, S, G16, u, WT, total;
};

HeadWs head_ws(const HeadGeom &g) {
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    HeadWs w{};
    size_t o = 0;
    w.term = o, o += up((size_t)g.rows * 4);
    w.part = o, o += up((size_t)kLossParts * 8);
    w.S = o, o += up((size_t)g.chunk * kV * 4);
    w.G16 = o, o += g.bf16 ? up((size_t)g.chunk * kV * 2) : 0;
    w.u = o, o += up((size_t)g.chunk * g.K * 4);
    w.WT = o, o += g.bf16 ? up((size_t)kV * g.K * 2) : 0;
    w.total = o;
    return w;
}

}  // namespace

static int byte_head_geom(const MotByteHeadDesc *d, HeadGeom *geom_out) {
    if (!d) return set_error(MOT_EINVAL, "byte_head: null descriptor");
    if (d->struct_size != sizeof(MotByteHeadDesc))
        return set_error(MOT_EINVAL, "byte_head: struct_size %u != %zu (ABI mismatch)", d->struct_size, sizeof(MotByteHeadDesc));
    if (d->method != MOT_HEAD_COPY && d->method != MOT_HEAD_SPLIT)
        return set_error(MOT_EUNSUPPORTED, "byte_head: method %d is not built (copy and split are)", d->method);
    if (d->dtype != MOT_F32 && d->dtype != MOT_BF16) return set_error(MOT_EUNSUPPORTED, "byte_head: dtype %d is not built", d->dtype);
    if (d->n_tokens < 0 || d->model_dim <= 0 || d->n_layer_out < 0 || d->n_layer_out > 64)
        return set_error(MOT_ESHAPE, "byte_head: n_tokens %lld, model_dim %d, n_layer_out %d", (long long)d->n_tokens, d->model_dim, d->n_layer_out);
    if (d->bpt < 1 || d->bpt > MOT_MAX_BPT) return set_error(MOT_ESHAPE, "byte_head: bpt %d outside [1, %d]", d->bpt, MOT_MAX_BPT);
    if (d->vocab != kV) return set_error(MOT_EUNSUPPORTED, "byte_head: vocab %d: only the %d-row head is built", d->vocab, kV);
    const bool split = d->method == MOT_HEAD_SPLIT;
    if (split && d->model_dim % d->bpt)
        return set_error(MOT_ESHAPE, "byte_head: split needs model_dim %% bpt == 0 (train_gpt.py:503), got %d %% %d", d->model_dim, d->bpt);
    const int K = split ? d->model_dim / d->bpt : d->model_dim;
    if (K % 16 || K > kMaxK) return set_error(MOT_EUNSUPPORTED, "byte_head: row width %d must be a multiple of 16 and at most %d", K, kMaxK);
    const int64_t M = d->n_tokens * (int64_t)d->bpt;
    if (M > 0x7fffffffLL) return set_error(MOT_EUNSUPPORTED, "byte_head: n_tokens * bpt exceeds 2^31");
    HeadGeom &g = *geom_out;
    g.rows = split ? M : d->n_tokens;
    g.K = K;
    g.tpr = split ? 1 : d->bpt;
    g.M = M;
    g.bf16 = d->dtype == MOT_BF16;
    g.eps = d->eps > 0.f ? d->eps : 1.1920928955078125e-07f;   // F.rms_norm(eps=None): the fp32 opmath epsilon, bf16 inputs included
    const int64_t per_row = (int64_t)kV * 4 + (g.bf16 ? kV * 2 : 0) + (int64_t)K * 4;
    int64_t ch = kChunkBytes / per_row / 256 * 256;
    if (ch < 256) ch = 256;
    g.chunk = g.rows < ch ? g.rows : ch;
    return MOT_OK;
}

int byte_head_check(const MotByteHeadDesc *d) {
    HeadGeom g;
    return byte_head_geom(d, &g);
}

size_t byte_head_workspace_bytes(const MotByteHeadDesc &d) {
    HeadGeom g;
    if (byte_head_geom(&d, &g) || g.rows == 0) return 0;
    return head_ws(g).total;
}

static int head_check_ptrs(const MotByteHeadDesc &d, const HeadGeom &g, size_t need) {
    if (!d.x || !d.weight || !d.targets || !d.row_stats) return set_error(MOT_EINVAL, "byte_head: null x / weight / targets / row_stats");
    if (!d.workspace || d.workspace_bytes < need)
        return set_error(MOT_EWORKSPACE, "byte_head: workspace %zu bytes < %zu", d.workspace ? d.workspace_bytes : (size_t)0, need);
    if (((uintptr_t)d.x & 15) || ((uintptr_t)d.weight & 15)) return set_error(MOT_EUNSUPPORTED, "byte_head: x and weight must be 16-byte aligned");
    return MOT_OK;
}

// s = x W^T for rows [r0, r0 + n) of the chunk into S (fp32 [n][512])
static int head_logits(const MotByteHeadDesc &d, const HeadGeom &g, int64_t r0, int64_t n, float *S, hipStream_t stream) {
    if (g.bf16)
        return launch_gemm_rows_bf16((const __bf16 *)d.x + r0 * g.K, g.K, n, d.weight, g.K, g.K, kV, S, kV, false, nullptr, stream);
    return launch_gemm_rows((const float *)d.x + r0 * g.K, g.K, n, (const float *)d.weight, g.K, g.K, kV, S, kV, true, stream);
}

int launch_byte_head_fwd(const MotByteHeadDesc &d, hipStream_t stream) {
    HeadGeom g;
    int rc = byte_head_geom(&d, &g);
    if (rc) return rc;
    if (!d.loss) return set_error(MOT_EINVAL, "byte_head: null loss");
    if (g.rows == 0) return set_error(MOT_ESHAPE, "byte_head: no targets (the mean over zero targets is undefined)");
    const HeadWs w = head_ws(g);
    if ((rc = head_check_ptrs(d, g, w.total))) return rc;
    unsigned char *ws = (unsigned char *)d.workspace;
    float *term = (float *)(ws + w.term), *S = (float *)(ws + w.S);
    float *lse = d.row_stats, *cst = d.row_stats + g.rows;
    for (int64_t r0 = 0; r0 < g.rows; r0 += g.chunk) {
        const int64_t n = g.rows - r0 < g.chunk ? g.rows - r0 : g.chunk;
        if ((rc = head_logits(d, g, r0, n, S, stream))) return rc;
        const unsigned blocks = (unsigned)((n + kWaves - 1) / kWaves);
        const int64_t *tg = d.targets + r0 * g.tpr;
        if (g.bf16)
            hipLaunchKernelGGL(head_fwd_rows<__bf16>, dim3(blocks), dim3(kThreads), 0, stream, S, (const __bf16 *)d.x + r0 * g.K, g.K, tg, g.tpr, n,
                               d.n_layer_out, g.eps, lse + r0, cst + r0, term + r0, d.status);
        else
            hipLaunchKernelGGL(head_fwd_rows<float>, dim3(blocks), dim3(kThreads), 0, stream, S, (const float *)d.x + r0 * g.K, g.K, tg, g.tpr, n,
                               d.n_layer_out, g.eps, lse + r0, cst + r0, term + r0, d.status);
        if ((rc = check_launch("head_fwd_rows"))) return rc;
    }
    double *part = (double *)(ws + w.part);
    const int parts = loss_parts(g.rows);
    hipLaunchKernelGGL(head_loss_parts, dim3(parts), dim3(kThreads), 0, stream, term, g.rows, part);
    if ((rc = check_launch("head_loss_parts"))) return rc;
    hipLaunchKernelGGL(head_loss_final, dim3(1), dim3(kThreads), 0, stream, part, parts, 1.0 / (double)g.M, d.loss);
    return check_launch("head_loss_final");
}

int launch_byte_head_bwd(const MotByteHeadDesc &d, const float *grad_loss, void *dx, float *dW, hipStream_t stream) {
    HeadGeom g;
    int rc = byte_head_geom(&d, &g);
    if (rc) return rc;
    if (!grad_loss || !dx || !dW) return set_error(MOT_EINVAL, "byte_head: null grad_loss / dx / dW");
    if (g.rows == 0) return set_error(MOT_ESHAPE, "byte_head: no targets");
    const HeadWs w = head_ws(g);
    if ((rc = head_check_ptrs(d, g, w.total))) return rc;
    if ((uintptr_t)dx & 15) return set_error(MOT_EUNSUPPORTED, "byte_head: dx must be 16-byte aligned");
    unsigned char *ws = (unsigned char *)d.workspace;
    float *S = (float *)(ws + w.S), *u = (float *)(ws + w.u);
    __bf16 *G16 = (__bf16 *)(ws + w.G16), *WT = (__bf16 *)(ws + w.WT);
    const float *lse = d.row_stats, *cst = d.row_stats + g.rows;
    const float inv_m = (float)(1.0 / (double)g.M);
    if ((rc = launch_zero_words(dW, (int64_t)kV * g.K, stream))) return rc;
    if (g.bf16) {
        hipLaunchKernelGGL(head_transpose_bf16, dim3((unsigned)((kV * g.K + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, (const __bf16 *)d.weight,
                           g.K, WT);
        if ((rc = check_launch("head_transpose_bf16"))) return rc;
    }
    for (int64_t r0 = 0; r0 < g.rows; r0 += g.chunk) {
        const int64_t n = g.rows - r0 < g.chunk ? g.rows - r0 : g.chunk;
        const unsigned blocks = (unsigned)((n + kWaves - 1) / kWaves);
        const int64_t *tg = d.targets + r0 * g.tpr;
        if ((rc = head_logits(d, g, r0, n, S, stream))) return rc;
        if (g.bf16) {
            const __bf16 *x = (const __bf16 *)d.x + r0 * g.K;
            hipLaunchKernelGGL(head_grad_rows<__bf16>, dim3(blocks), dim3(kThreads), 0, stream, S, tg, g.tpr, n, lse + r0, cst + r0, grad_loss, inv_m, G16);
            if ((rc = check_launch("head_grad_rows"))) return rc;
            if ((rc = launch_gemm_rows_bf16(G16, kV, n, WT, kV, kV, g.K, u, g.K, false, nullptr, stream))) return rc;
            if ((rc = launch_gemm_tn_bf16(G16, kV, kV, x, g.K, g.K, n, dW, g.K, stream))) return rc;
            hipLaunchKernelGGL(head_chain_rows<__bf16>, dim3(blocks), dim3(kThreads), 0, stream, x, u, g.K, n, d.n_layer_out, g.eps, (__bf16 *)dx + r0 * g.K);
        } else {
            const float *x = (const float *)d.x + r0 * g.K;
            hipLaunchKernelGGL(head_grad_rows<float>, dim3(blocks), dim3(kThreads), 0, stream, S, tg, g.tpr, n, lse + r0, cst + r0, grad_loss, inv_m, S);
            if ((rc = check_launch("head_grad_rows"))) return rc;
            if ((rc = launch_gemm_rows(S, kV, n, (const float *)d.weight, g.K, kV, g.K, u, g.K, false, stream))) return rc;
            if ((rc = launch_gemm_tn(S, kV, kV, x, g.K, g.K, n, dW, g.K, stream))) return rc;
            hipLaunchKernelGGL(head_chain_rows<float>, dim3(blocks), dim3(kThreads), 0, stream, x, u, g.K, n, d.n_layer_out, g.eps, (float *)dx + r0 * g.K);
        }
        if ((rc = check_launch("head_chain_rows"))) return rc;
    }
    return MOT_OK;
}

}  // namespace mot
