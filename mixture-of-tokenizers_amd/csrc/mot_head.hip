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
// so no tensor of M x 512 exists in split mode.  The loss is a fixed-order double sum of per-row terms: the same bits every run.
// mot_byte_head_eval is the forward whose row pass (head_fwd_rows<T, true>) also writes, per byte position, the loss term, the class
// of the largest stored logit and the number of stored logits above the target's (include/mot.h).
// This unit holds the two 512-wide row passes, head_fwd_rows and head_grad_rows, the checks and the carve; row_scale, the products,
// the chunk rule, the row chain and the loss's sum are the heads' shared ones (mot_headcore.hpp).
#include "mot_headcore.hpp"

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

// one wave per row: c, z, lse and the row's loss term; lane j holds classes lane + 64 i.
// EVAL is the evaluation variant (lse and cst optional): it also writes, for each of the row's tpr targets (lane k keeps those of
// target k: tpr <= MOT_MAX_BPT = 64), lse - z[y], the class of the row's largest stored logit and the number of stored logits
// above the target's into `ev` at byte position r * tpr + k.
template <typename T, bool EVAL>
__global__ __launch_bounds__(kThreads) void head_fwd_rows(const float *__restrict__ S, const T *__restrict__ x, int K, const int64_t *__restrict__ tgt,
                                                          int tpr, int64_t rows, int L, float eps, float *__restrict__ lse, float *__restrict__ cst,
                                                          float *__restrict__ term, uint32_t *status, HeadEvalRows ev) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (r >= rows) return;
    float c, dc;
    row_scale(row_sumsq(x + r * K, K, lane) / (float)K, L, eps, c, dc);
    const float *s = S + r * kV;
    float z[8], sv[EVAL ? 8 : 1], se = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float si = s[lane + 64 * i];
        if (EVAL) sv[i] = si;
        z[i] = kCap * sigm(c * si);
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
        if (!EVAL || lse) lse[r] = l;
        if (!EVAL || cst) cst[r] = c;
        term[r] = (float)nv * l - tz;
        if (nv < tpr && status) atomicOr(status, (uint32_t)MOT_STATUS_TARGET_OOR);
    }
    if (!EVAL) return;
    float best = -INFINITY;
    int best_cls = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < 8; ++i)   // ascending classes: `>` keeps the lowest of equal logits
        if (sv[i] > best) {
            best = sv[i];
            best_cls = lane + 64 * i;
        }
    wave_argmax(best, best_cls);
    float my_loss = 0.f;
    int my_rank = -1;
    for (int k = 0; k < tpr; ++k) {
        const int64_t y = tgt[r * tpr + k];
        if (y < 0 || y >= kV) continue;   // wave-uniform
        const float sy = s[y];
        int above = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) above += sv[i] > sy ? 1 : 0;
        const float n_above = wave_sum((float)above);   // at most 512: exact in fp32
        if (lane == k) {
            my_loss = l - kCap * sigm(c * sy);
            my_rank = (int)n_above;
        }
    }
    if (lane < tpr) {
        const int64_t at = r * tpr + lane;
        if (ev.row_loss) ev.row_loss[at] = my_loss;
        if (ev.pred) ev.pred[at] = best_cls;
        if (ev.rank) ev.rank[at] = my_rank;
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
    Arena a;
    HeadWs w{};
    w.term = a.take((size_t)g.rows * 4);
    w.part = a.take((size_t)kLossParts * 8);
    w.S = a.take((size_t)g.chunk * kV * 4);
    w.G16 = a.take(g.bf16 ? (size_t)g.chunk * kV * 2 : 0);
    w.u = a.take((size_t)g.chunk * g.K * 4);
    w.WT = a.take(g.bf16 ? (size_t)kV * g.K * 2 : 0);
    w.total = a.o;
    return w;
}

}  // namespace

static int byte_head_geom(const MotByteHeadDesc *d, HeadGeom *geom_out, const char *fn = "byte_head") {
    if (!d) return set_error(MOT_EINVAL, "%s: null descriptor", fn);
    if (d->struct_size != sizeof(MotByteHeadDesc))
        return set_error(MOT_EINVAL, "%s: struct_size %u != %zu (ABI mismatch)", fn, d->struct_size, sizeof(MotByteHeadDesc));
    if (d->method != MOT_HEAD_COPY && d->method != MOT_HEAD_SPLIT)
        return set_error(MOT_EUNSUPPORTED, "%s: method %d is not built (copy and split are)", fn, d->method);
    if (d->dtype != MOT_F32 && d->dtype != MOT_BF16) return set_error(MOT_EUNSUPPORTED, "%s: dtype %d is not built", fn, d->dtype);
    if (d->n_tokens < 0 || d->model_dim <= 0 || d->n_layer_out < 0 || d->n_layer_out > 64)
        return set_error(MOT_ESHAPE, "%s: n_tokens %lld, model_dim %d, n_layer_out %d", fn, (long long)d->n_tokens, d->model_dim, d->n_layer_out);
    if (d->bpt < 1 || d->bpt > MOT_MAX_BPT) return set_error(MOT_ESHAPE, "%s: bpt %d outside [1, %d]", fn, d->bpt, MOT_MAX_BPT);
    if (d->vocab != kV) return set_error(MOT_EUNSUPPORTED, "%s: vocab %d: only the %d-row head is built", fn, d->vocab, kV);
    const bool split = d->method == MOT_HEAD_SPLIT;
    if (split && d->model_dim % d->bpt)
        return set_error(MOT_ESHAPE, "%s: split needs model_dim %% bpt == 0 (train_gpt.py:503), got %d %% %d", fn, d->model_dim, d->bpt);
    const int K = split ? d->model_dim / d->bpt : d->model_dim;
    if (K % 16 || K > kMaxK) return set_error(MOT_EUNSUPPORTED, "%s: row width %d must be a multiple of 16 and at most %d", fn, K, kMaxK);
    const int64_t M = d->n_tokens * (int64_t)d->bpt;
    if (M > 0x7fffffffLL) return set_error(MOT_EUNSUPPORTED, "%s: n_tokens * bpt exceeds 2^31", fn);
    HeadGeom &g = *geom_out;
    g.rows = split ? M : d->n_tokens;
    g.K = K;
    g.tpr = split ? 1 : d->bpt;
    g.M = M;
    g.bf16 = d->dtype == MOT_BF16;
    g.eps = d->eps > 0.f ? d->eps : kHeadEps;
    g.chunk = head_chunk_rows(kChunkBytes, (int64_t)kV * 4 + (g.bf16 ? kV * 2 : 0) + (int64_t)K * 4, g.rows);
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

static int head_check_ptrs(const MotByteHeadDesc &d, const HeadGeom &g, size_t need, const char *fn = "byte_head", bool need_stats = true) {
    if (!d.x || !d.weight || !d.targets || (need_stats && !d.row_stats))
        return set_error(MOT_EINVAL, "%s: null x / weight / targets%s", fn, need_stats ? " / row_stats" : "");
    if (!d.workspace || d.workspace_bytes < need)
        return set_error(MOT_EWORKSPACE, "%s: workspace %zu bytes < %zu", fn, d.workspace ? d.workspace_bytes : (size_t)0, need);
    if (((uintptr_t)d.x & 15) || ((uintptr_t)d.weight & 15)) return set_error(MOT_EUNSUPPORTED, "%s: x and weight must be 16-byte aligned", fn);
    return MOT_OK;
}

// `ev` set: the evaluation call: the row pass also writes ev's rows per byte position, and the counts are closed behind the loss
template <typename T>
static int byte_head_fwd_run(const MotByteHeadDesc &d, const HeadGeom &g, const HeadWs &w, const MotHeadEvalOut *ev, hipStream_t stream) {
    unsigned char *ws = (unsigned char *)d.workspace;
    float *term = (float *)(ws + w.term), *S = (float *)(ws + w.S);
    float *lse = d.row_stats, *cst = d.row_stats ? d.row_stats + g.rows : nullptr;
    const HeadEvalRows ev_rows = ev ? HeadEvalRows{ev->row_loss, ev->pred, ev->rank} : HeadEvalRows{};
    int rc;
    for (int64_t r0 = 0; r0 < g.rows; r0 += g.chunk) {
        const int64_t n = g.rows - r0 < g.chunk ? g.rows - r0 : g.chunk;
        const T *x = (const T *)d.x + r0 * g.K;
        if ((rc = launch_product_nt(head_dtype<T>, x, g.K, n, d.weight, g.K, g.K, kV, S, kV, false, nullptr, false, stream))) return rc;
        const dim3 grid((unsigned)((n + kWaves - 1) / kWaves));
        if (ev)
            hipLaunchKernelGGL((head_fwd_rows<T, true>), grid, dim3(kThreads), 0, stream, S, x, g.K, d.targets + r0 * g.tpr, g.tpr, n, d.n_layer_out, g.eps,
                               lse ? lse + r0 : nullptr, cst ? cst + r0 : nullptr, term + r0, d.status, ev_rows.at(r0 * g.tpr));
        else
            hipLaunchKernelGGL((head_fwd_rows<T, false>), grid, dim3(kThreads), 0, stream, S, x, g.K, d.targets + r0 * g.tpr, g.tpr, n, d.n_layer_out, g.eps,
                               lse + r0, cst + r0, term + r0, d.status, HeadEvalRows{});
        if ((rc = check_launch("head_fwd_rows"))) return rc;
    }
    if ((rc = launch_head_loss(term, g.rows, (double *)(ws + w.part), 1.0 / (double)g.M, d.loss, stream))) return rc;
    if (ev && ev->counts) return launch_head_eval_counts(ev->pred, d.targets, g.M / d.bpt, d.bpt, kV, ws + w.part, ev->counts, 3, stream);
    return MOT_OK;
}

int launch_byte_head_fwd(const MotByteHeadDesc &d, hipStream_t stream) {
    HeadGeom g;
    int rc = byte_head_geom(&d, &g);
    if (rc) return rc;
    if (!d.loss) return set_error(MOT_EINVAL, "byte_head: null loss");
    if (g.rows == 0) return set_error(MOT_ESHAPE, "byte_head: no targets (the mean over zero targets is undefined)");
    const HeadWs w = head_ws(g);
    if ((rc = head_check_ptrs(d, g, w.total))) return rc;
    return g.bf16 ? byte_head_fwd_run<__bf16>(d, g, w, nullptr, stream) : byte_head_fwd_run<float>(d, g, w, nullptr, stream);
}

int launch_byte_head_eval(const MotByteHeadDesc *d, const MotHeadEvalOut *out, hipStream_t stream) {
    static const char fn[] = "mot_byte_head_eval";
    HeadGeom g;
    int rc = byte_head_geom(d, &g, fn);
    if (rc || (rc = head_eval_check(fn, out))) return rc;
    if (!d->loss) return set_error(MOT_EINVAL, "%s: null loss", fn);
    if (g.rows == 0) return set_error(MOT_ESHAPE, "%s: no targets (the mean over zero targets is undefined)", fn);
    const HeadWs w = head_ws(g);
    if ((rc = head_check_ptrs(*d, g, w.total, fn, false))) return rc;
    return g.bf16 ? byte_head_fwd_run<__bf16>(*d, g, w, out, stream) : byte_head_fwd_run<float>(*d, g, w, out, stream);
}

// In fp32 G overwrites the chunk's logits S; in bf16 it is the bf16 copy G16, and u = G W reads the k-major copy WT of W.
template <typename T>
static int byte_head_bwd_run(const MotByteHeadDesc &d, const HeadGeom &g, const HeadWs &w, const float *grad_loss, T *dx, float *dW, hipStream_t stream) {
    constexpr bool BF = sizeof(T) == 2;
    unsigned char *ws = (unsigned char *)d.workspace;
    float *S = (float *)(ws + w.S), *u = (float *)(ws + w.u);
    T *G = (T *)(ws + (BF ? w.G16 : w.S)), *WT = (T *)(ws + w.WT);
    const T *W = (const T *)d.weight;
    const float *lse = d.row_stats, *cst = d.row_stats + g.rows;
    const float inv_m = (float)(1.0 / (double)g.M);
    int rc;
    if ((rc = launch_zero_words(dW, (int64_t)kV * g.K, stream))) return rc;
    if (BF && (rc = launch_transpose_bf16(W, kV, g.K, WT, stream))) return rc;
    for (int64_t r0 = 0; r0 < g.rows; r0 += g.chunk) {
        const int64_t n = g.rows - r0 < g.chunk ? g.rows - r0 : g.chunk;
        const T *x = (const T *)d.x + r0 * g.K;
        if ((rc = launch_product_nt(head_dtype<T>, x, g.K, n, W, g.K, g.K, kV, S, kV, false, nullptr, false, stream))) return rc;
        hipLaunchKernelGGL(head_grad_rows<T>, dim3((unsigned)((n + kWaves - 1) / kWaves)), dim3(kThreads), 0, stream, S, d.targets + r0 * g.tpr, g.tpr, n,
                           lse + r0, cst + r0, grad_loss, inv_m, G);
        if ((rc = check_launch("head_grad_rows"))) return rc;
        if ((rc = launch_product_nn(head_dtype<T>, G, kV, n, BF ? WT : W, BF ? kV : g.K, kV, g.K, u, g.K, stream))) return rc;
        if ((rc = launch_product_tn(head_dtype<T>, G, kV, kV, x, g.K, g.K, n, dW, g.K, stream))) return rc;
        if ((rc = launch_head_chain<T>(x, u, g.K, n, d.n_layer_out, 1, g.eps, dx + r0 * g.K, stream))) return rc;
    }
    return MOT_OK;
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
    return g.bf16 ? byte_head_bwd_run<__bf16>(d, g, w, grad_loss, (__bf16 *)dx, dW, stream) : byte_head_bwd_run<float>(d, g, w, grad_loss, (float *)dx, dW, stream);
}

}  // namespace mot
