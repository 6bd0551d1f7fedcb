// mot_tokhead.hip -- the token-level output head, the last five lines of every training script of the reference:
//   scaled-pre-train/train_gpt.py:619-623 (byte_mixout_method "noop"):  x = norm(x); l = lm_head(x); z = 30 sigmoid(l.float() / 7.5); CE(z, y)
//   modded-nanogpt/runs/71_*.py:331-334 (all 50 runs):                 x = norm(x); l = x W^T;       z = 15 l rsqrt(l^2 + 225);   CE(z, y)
// over a vocabulary of 50 304 rows, forward and backward in ONE call and without any N x V tensor.
//
// Per row r of x [N, D], W [V, D], y [N]:  c_r = (mean(x_r^2) + eps)^-1/2 (1 without norm_in),  l = c_r (x_r W^T),  z = cap(l).
// z is bounded (0 < z < 30, |z| < 15), so lse = zmax + log sum exp(z - zmax) with the constant zmax: no max pass.
//   loss    = (1 / N) sum_r (lse_r - z_r[y_r])                       fixed-order double sum (mot_headcore.hip)
//   dL/dl_r = (1 / N) (softmax(z_r) - onehot(y_r)) dz/dl,   G_r = c_r dL/dl_r,   u = G W,   dW = G^T x,
//   dx_r    = u_r - c_r^2 (x_r . u_r / D) x_r  (norm_in),  u_r (else)
// A target outside [0, V) addresses nothing: its term leaves the sum (the mean still divides by N), its row of G is zero, so its row
// of dx is exactly zero and it adds nothing to dW; MOT_STATUS_TARGET_OOR is raised.
//
// The rows run in chunks.  A chunk's logits s = x W^T are one product on the shared launchers into the chunk scratch S (fp32, or bf16
// in bf16 mode: the reference's own rounding point, CastedLinear returns bf16).  tokhead_rows, the V-wide row pass and the new kernel
// of this file, takes one row per workgroup: it loads the row's logits ONCE with 16-byte accesses into registers, forms c, sum exp,
// z[y] and the row's loss term, and, when gradients are asked for, writes G in place over the logits from the same registers.  Then
// u = G W and dW += G^T x are two more products on the shared launchers, and the heads' wave-per-row chain closes dx.  So a chunk's
// logits are formed once and a training step costs three products.  The gradients are those of grad_loss = 1; the caller scales them.
// mot_token_head_eval is the loss call without gradients whose row pass (the EVAL instantiations of tokhead_rows) also writes every
// row's loss term, the class of its largest stored logit and the number of stored logits above the target's (include/mot.h).
// This unit holds tokhead_rows, the checks and the carve; row_scale, the products, the chunk rule, the chain and the loss's sum are
// the heads' shared ones (mot_headcore.hpp); the vector of logits, the workgroup's sums and the evaluation's share of a vector are
// shared with the plain head's row pass (mot_headrows.hpp).
#include "mot_headrows.hpp"

namespace mot {
namespace {

// z = cap(l) and dz/dl
template <int CAP>
__device__ __forceinline__ float softcap(float l, float &dz) {
    if (CAP == MOT_SOFTCAP_SIGMOID30) {
        const float s = 1.f / (1.f + __expf(-l * (1.f / 7.5f)));
        dz = 4.f * s * (1.f - s);
        return 30.f * s;
    } else {
        const float r = rsqrtf(l * l + 225.f);
        dz = 3375.f * r * r * r;
        return 15.f * l * r;
    }
}
template <int CAP>
__device__ __forceinline__ float softcap_max() { return CAP == MOT_SOFTCAP_SIGMOID30 ? 30.f : 15.f; }

// sum exp(z - zmax) over one vector, and z[y] when the vector holds class y (ey: its element there, else -1)
template <typename T, int CAP>
__device__ __forceinline__ float vec_stats(const LogitVec<T> &a, float c, int ey, float &zy) {
    float se = 0.f;
#pragma unroll
    for (int e = 0; e < LogitVec<T>::N; ++e) {
        float dz;
        const float z = softcap<CAP>(c * a.get(e), dz);
        se += __expf(z - softcap_max<CAP>());
        if (e == ey) zy = z;
    }
    return se;
}

// G = c (1 / N) dz/dl (exp(z - lse) - onehot) over one vector; `scale` = c / N, or 0 for a dropped row
template <typename T, int CAP>
__device__ __forceinline__ void vec_grad(LogitVec<T> &a, float c, float lse, float scale, int ey) {
    float g[LogitVec<T>::N];
#pragma unroll
    for (int e = 0; e < LogitVec<T>::N; ++e) {
        float dz;
        const float z = softcap<CAP>(c * a.get(e), dz);
        const float p = __expf(z - lse);
        g[e] = scale * dz * (p - (e == ey ? 1.f : 0.f));
    }
    a.put(g);
}

// One workgroup per row of the chunk.  NV > 0: the row's vectors (nvec = V / N <= NV * blockDim.x) stay in registers between the
// two uses, vector i of thread t is number t + i * blockDim.x, so a wave's 64 lanes touch 1 KiB at a time and the ragged last
// round is a predicate.  NV == 0: rows too wide for the register file (V above kRegV) are read a second time.
// EVAL (never with GRAD) is the evaluation variant: the same sweep also carries the row's largest stored logit with its class and
// counts the stored logits above the target's, which every thread fetches for itself (one cached address); `ev` takes the results.
template <typename T, int CAP, int NV, bool GRAD, bool EVAL>
__global__ __launch_bounds__(kRowThreads) void tokhead_rows(T *S, int V, const T *__restrict__ x, int K, int norm_in, float eps,
                                                            const int64_t *__restrict__ tgt, int64_t rows, float inv_n, float *__restrict__ term,
                                                            float *__restrict__ row_stats, int64_t stats_stride, uint32_t *status, HeadEvalRows ev) {
    typedef LogitVec<T> Vec;
    __shared__ float sh_ss[kRowWavesMax], sh_se[kRowWavesMax], sh_zy[kRowWavesMax];
    __shared__ float sh_top[EVAL ? kRowWavesMax : 1], sh_above[EVAL ? kRowWavesMax : 1];
    __shared__ int sh_cls[EVAL ? kRowWavesMax : 1];
    const int64_t r = blockIdx.x;
    if (r >= rows) return;
    const int tid = threadIdx.x, nt = blockDim.x, nvec = V / Vec::N;
    Vec *row = (Vec *)(S + r * (int64_t)V);
    Vec a[NV > 0 ? NV : 1];
    if (NV > 0) {   // every load of the row is in flight before anything waits
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = tid + i * nt;
            if (idx < nvec) a[i] = row[idx];
        }
    }
    float c = 1.f;
    if (norm_in) {
        float ss = 0.f;
        for (int k = tid; k < K; k += nt) {
            const float v = (float)x[r * K + k];
            ss += v * v;
        }
        float dc;
        row_scale(rows_block_sum(ss, sh_ss) / (float)K, 0, eps, c, dc);
    }
    const int64_t y = tgt[r];
    const bool in_range = y >= 0 && y < V;
    const int yvec = in_range ? (int)(y / Vec::N) : -1, yel = in_range ? (int)(y % Vec::N) : -1;
    float se = 0.f, zy = 0.f;
    float sy = 0.f, best = -INFINITY;   // EVAL: the target's stored logit, the largest of this thread's
    int best_cls = 0x7fffffff, above = 0;
    if (EVAL && in_range) sy = (float)S[r * (int64_t)V + y];
    if (NV > 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = tid + i * nt;
            if (idx < nvec) {
                se += vec_stats<T, CAP>(a[i], c, idx == yvec ? yel : -1, zy);
                if (EVAL) vec_top<T>(a[i], idx * Vec::N, sy, best, best_cls, above);
            }
        }
    } else {
        for (int idx = tid; idx < nvec; idx += nt) {
            const Vec v = row[idx];
            se += vec_stats<T, CAP>(v, c, idx == yvec ? yel : -1, zy);
            if (EVAL) vec_top<T>(v, idx * Vec::N, sy, best, best_cls, above);
        }
    }
    if (EVAL) {   // the waves' pairs, met in wave order behind the next sum's barrier
        wave_argmax(best, best_cls);
        if ((tid & 63) == 0) {
            sh_top[tid >> 6] = best;
            sh_cls[tid >> 6] = best_cls;
        }
    }
    se = rows_block_sum(se, sh_se);
    zy = rows_block_sum(zy, sh_zy);   // one thread holds z[y], the others 0
    const float lse = softcap_max<CAP>() + __logf(se);
    if (tid == 0) {
        term[r] = in_range ? lse - zy : 0.f;
        if (row_stats) {
            row_stats[r] = lse;
            row_stats[stats_stride + r] = c;
        }
        if (!in_range && status) atomicOr(status, (uint32_t)MOT_STATUS_TARGET_OOR);
    }
    if (EVAL) {
        const float n_above = rows_block_sum((float)above, sh_above);   // at most kMaxV = 2^18: exact in fp32
        if (tid == 0) {
            for (int w = 1; w < (nt >> 6); ++w) argmax_take(best, best_cls, sh_top[w], sh_cls[w]);   // thread 0 holds wave 0's pair
            if (ev.row_loss) ev.row_loss[r] = in_range ? lse - zy : 0.f;
            if (ev.pred) ev.pred[r] = best_cls;
            if (ev.rank) ev.rank[r] = in_range ? (int)n_above : -1;
        }
    }
    if (!GRAD) return;
    const float scale = in_range ? c * inv_n : 0.f;
    if (NV > 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = tid + i * nt;
            if (idx < nvec) {
                vec_grad<T, CAP>(a[i], c, lse, scale, idx == yvec ? yel : -1);
                row[idx] = a[i];
            }
        }
    } else {
        for (int idx = tid; idx < nvec; idx += nt) {
            Vec v = row[idx];
            vec_grad<T, CAP>(v, c, lse, scale, idx == yvec ? yel : -1);
            row[idx] = v;
        }
    }
}

struct TokGeom {
    int64_t rows, chunk;
    int K, V, norm_in;
    bool bf16, grad_x;
    float eps;
};

struct TokWs {   // carve of the workspace, offsets in bytes
    size_t term, part, S, u, WT, total;
};

TokWs tok_ws(const TokGeom &g) {
    Arena a;
    TokWs w{};
    w.term = a.take((size_t)g.rows * 4);
    w.part = a.take((size_t)kLossParts * 8);
    w.S = a.take((size_t)g.chunk * g.V * (g.bf16 ? 2 : 4));
    w.u = a.take(g.grad_x ? (size_t)g.chunk * g.K * 4 : 0);
    w.WT = a.take(g.grad_x && g.bf16 ? (size_t)g.V * g.K * 2 : 0);
    w.total = a.o;
    return w;
}

// the row pass of one chunk: the workgroup size and the registers per thread follow the row's number of 16-byte vectors
template <typename T, int CAP, bool GRAD, bool EVAL = false>
int launch_rows(T *S, const TokGeom &g, const T *x, const int64_t *tgt, int64_t n, float inv_n, float *term, float *row_stats, uint32_t *status,
                hipStream_t stream, HeadEvalRows ev = {}) {
    int nt, nv;
    rows_geometry<T>(g.V, nt, nv);
#define MOT_TOKHEAD_ROWS(NV)                                                                                                                              \
    hipLaunchKernelGGL((tokhead_rows<T, CAP, NV, GRAD, EVAL>), dim3((unsigned)n), dim3(nt), 0, stream, S, g.V, x, g.K, g.norm_in, g.eps, tgt, n, inv_n, \
                       term, row_stats, g.rows, status, ev)
    // registers hold a row of up to kRegV classes (16 vectors a thread in fp32, 8 in bf16); a wider row is read twice
    if (nv <= 4) MOT_TOKHEAD_ROWS(4);
    else if (nv <= 8) MOT_TOKHEAD_ROWS(8);
    else if (g.V <= kRegV) MOT_TOKHEAD_ROWS(kRegV / (kRowThreads * LogitVec<T>::N));   // 16 in fp32 (bf16 rows this wide took 8 above)
    else MOT_TOKHEAD_ROWS(0);
#undef MOT_TOKHEAD_ROWS
    return check_launch("tokhead_rows");
}

}  // namespace

static int token_head_geom(const MotTokenHeadDesc *d, TokGeom *out, const char *fn = "token_head") {
    if (!d) return set_error(MOT_EINVAL, "%s: null descriptor", fn);
    if (d->struct_size != sizeof(MotTokenHeadDesc))
        return set_error(MOT_EINVAL, "%s: struct_size %u != %zu (ABI mismatch)", fn, d->struct_size, sizeof(MotTokenHeadDesc));
    if (d->dtype != MOT_F32 && d->dtype != MOT_BF16) return set_error(MOT_EUNSUPPORTED, "%s: dtype %d is not built", fn, d->dtype);
    if (d->softcap != MOT_SOFTCAP_SIGMOID30 && d->softcap != MOT_SOFTCAP_RSQRT15)
        return set_error(MOT_EUNSUPPORTED, "%s: softcap %d is not built (sigmoid30 and rsqrt15 are)", fn, d->softcap);
    if (d->n_rows < 0 || d->n_rows > 0x7fffffffLL || d->model_dim <= 0 || d->vocab <= 0)
        return set_error(MOT_ESHAPE, "%s: n_rows %lld, model_dim %d, vocab %d", fn, (long long)d->n_rows, d->model_dim, d->vocab);
    if (d->vocab % kMinV || d->vocab > kMaxV)
        return set_error(MOT_EUNSUPPORTED, "%s: vocab %d must be a multiple of %d and at most %d", fn, d->vocab, kMinV, kMaxV);
    if (d->model_dim % 16 || d->model_dim > kMaxD)
        return set_error(MOT_EUNSUPPORTED, "%s: model_dim %d must be a multiple of 16 and at most %d", fn, d->model_dim, kMaxD);
    if (d->chunk_rows < 0 || d->chunk_rows % 32)
        return set_error(MOT_ESHAPE, "%s: chunk_rows %d must be 0 (the library's choice) or a multiple of 32", fn, d->chunk_rows);
    if ((int64_t)d->chunk_rows * d->vocab > 0x7fffffffLL)
        return set_error(MOT_EUNSUPPORTED, "%s: chunk_rows %d x vocab %d exceeds 2^31 logits a chunk", fn, d->chunk_rows, d->vocab);
    TokGeom &g = *out;
    g.rows = d->n_rows;
    g.K = d->model_dim;
    g.V = d->vocab;
    g.norm_in = d->norm_in ? 1 : 0;
    g.bf16 = d->dtype == MOT_BF16;
    g.grad_x = d->dx != nullptr;
    g.eps = d->eps > 0.f ? d->eps : kHeadEps;
    if (d->chunk_rows)
        g.chunk = g.rows < d->chunk_rows ? g.rows : d->chunk_rows;
    else   // the library's choice: a chunk's logits and u stay below kChunkBytes
        g.chunk = head_chunk_rows(kChunkBytes, (int64_t)g.V * (g.bf16 ? 2 : 4) + (int64_t)g.K * 4, g.rows);
    return MOT_OK;
}

int token_head_check(const MotTokenHeadDesc *d) {
    TokGeom g;
    return token_head_geom(d, &g);
}

size_t token_head_workspace_bytes(const MotTokenHeadDesc &d) {
    TokGeom g;
    if (token_head_geom(&d, &g) || g.rows == 0) return 0;
    return tok_ws(g).total;
}

// `ev` set: the evaluation call (no gradients): its row pass also writes ev's rows, and the counts are closed behind the loss
template <typename T, int CAP>
static int token_head_run(const MotTokenHeadDesc &d, const TokGeom &g, const TokWs &w, const MotHeadEvalOut *ev, hipStream_t stream) {
    constexpr bool BF = sizeof(T) == 2;
    unsigned char *ws = (unsigned char *)d.workspace;
    float *term = (float *)(ws + w.term), *u = (float *)(ws + w.u);
    T *S = (T *)(ws + w.S), *WT = (T *)(ws + w.WT);
    const T *X = (const T *)d.x, *W = (const T *)d.weight;
    const bool grad = d.dx || d.dW;
    const float inv_n = (float)(1.0 / (double)g.rows);
    const HeadEvalRows ev_rows = ev ? HeadEvalRows{ev->row_loss, ev->pred, ev->rank} : HeadEvalRows{};
    int rc;
    if (d.dW && (rc = launch_zero_words(d.dW, (int64_t)g.V * g.K, stream))) return rc;
    if (BF && d.dx && (rc = launch_transpose_bf16(W, g.V, g.K, WT, stream))) return rc;   // WT[k][v]: the operand of u = G W on the bf16 launcher
    for (int64_t r0 = 0; r0 < g.rows; r0 += g.chunk) {
        const int64_t n = g.rows - r0 < g.chunk ? g.rows - r0 : g.chunk;
        const T *x = X + r0 * g.K;
        if ((rc = launch_product_nt(head_dtype<T>, x, g.K, n, W, g.K, g.K, g.V, S, g.V, BF, nullptr, false, stream))) return rc;   // s = x W^T for the chunk's rows, in T
        float *stats = d.row_stats ? d.row_stats + r0 : nullptr;
        if (ev)
            rc = launch_rows<T, CAP, false, true>(S, g, x, d.targets + r0, n, inv_n, term + r0, stats, d.status, stream, ev_rows.at(r0));
        else if (grad)
            rc = launch_rows<T, CAP, true>(S, g, x, d.targets + r0, n, inv_n, term + r0, stats, d.status, stream);
        else
            rc = launch_rows<T, CAP, false>(S, g, x, d.targets + r0, n, inv_n, term + r0, stats, d.status, stream);
        if (rc) return rc;
        if (d.dx) {   // u = G W, then the row chain of the plain norm (L = 0)
            if ((rc = launch_product_nn(head_dtype<T>, S, g.V, n, BF ? WT : W, BF ? g.V : g.K, g.V, g.K, u, g.K, stream))) return rc;
            if ((rc = launch_head_chain<T>(x, u, g.K, n, 0, g.norm_in, g.eps, (T *)d.dx + r0 * g.K, stream))) return rc;
        }
        if (d.dW && (rc = launch_product_tn(head_dtype<T>, S, g.V, g.V, x, g.K, g.K, n, d.dW, g.K, stream))) return rc;   // dW += G^T x
    }
    if ((rc = launch_head_loss(term, g.rows, (double *)(ws + w.part), 1.0 / (double)g.rows, d.loss, stream))) return rc;
    if (ev && ev->counts) return launch_head_eval_counts(ev->pred, d.targets, g.rows, 1, g.V, ws + w.part, ev->counts, 2, stream);
    return MOT_OK;
}

// the checks behind the descriptor's own, then the launches; `fn` starts the messages
static int token_head_launch(const MotTokenHeadDesc &d, const TokGeom &g, const MotHeadEvalOut *ev, const char *fn, hipStream_t stream) {
    if (!d.x || !d.weight || !d.targets || !d.loss) return set_error(MOT_EINVAL, "%s: null x / weight / targets / loss", fn);
    if (g.rows == 0) return set_error(MOT_ESHAPE, "%s: no rows (the mean over zero targets is undefined)", fn);
    const TokWs w = tok_ws(g);
    if (!d.workspace || d.workspace_bytes < w.total)
        return set_error(MOT_EWORKSPACE, "%s: workspace %zu bytes < %zu", fn, d.workspace ? d.workspace_bytes : (size_t)0, w.total);
    if (((uintptr_t)d.x & 15) || ((uintptr_t)d.weight & 15) || ((uintptr_t)d.workspace & 15) || ((uintptr_t)d.dx & 15) || ((uintptr_t)d.dW & 15))
        return set_error(MOT_EUNSUPPORTED, "%s: x, weight, workspace, dx and dW must be 16-byte aligned", fn);
    const bool sig = d.softcap == MOT_SOFTCAP_SIGMOID30;
    if (g.bf16)
        return sig ? token_head_run<__bf16, MOT_SOFTCAP_SIGMOID30>(d, g, w, ev, stream) : token_head_run<__bf16, MOT_SOFTCAP_RSQRT15>(d, g, w, ev, stream);
    return sig ? token_head_run<float, MOT_SOFTCAP_SIGMOID30>(d, g, w, ev, stream) : token_head_run<float, MOT_SOFTCAP_RSQRT15>(d, g, w, ev, stream);
}

int launch_token_head_fwd(const MotTokenHeadDesc &d, hipStream_t stream) {
    TokGeom g;
    int rc = token_head_geom(&d, &g);
    if (rc) return rc;
    return token_head_launch(d, g, nullptr, "token_head", stream);
}

int launch_token_head_eval(const MotTokenHeadDesc *d, const MotHeadEvalOut *out, hipStream_t stream) {
    static const char fn[] = "mot_token_head_eval";
    TokGeom g;
    int rc = token_head_geom(d, &g, fn);
    if (rc || (rc = head_eval_check(fn, out))) return rc;
    if (d->dx || d->dW) return set_error(MOT_EINVAL, "%s: dx / dW set: the evaluation forms no gradients (mot_token_head_fwd does)", fn);
    return token_head_launch(*d, g, out, fn, stream);
}

}  // namespace mot
