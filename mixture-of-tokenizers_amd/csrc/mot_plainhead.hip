// mot_plainhead.hip -- the plain cross-entropy head: lm_head and F.cross_entropy on the logits as they are, with no softcap, with
// ignore_index, and with the mean taken over the kept targets.  The loss of the reference's two remaining loops:
//   mathblations/model.py:337-338 with main.py:294-303 (evaluation :164-187): F.rms_norm(x); lm_head(x).float();
//                                  slice_logits_and_targets; F.cross_entropy                       (50 304 classes, fp32)
//   inference/inference.py:349-359: lm_head(hidden_states); shift; CrossEntropyLoss()              (128 256 classes, no norm)
// forward and backward in ONE call and without any N x V tensor.
//
// Per row r of x [N, D], W [V, D], y [N]:  c_r = (mean(x_r^2) + eps)^-1/2 (1 without norm_in),  l = c_r (x_r W^T),
//   m_r = max_v l,  lse_r = m_r + log sum_v exp(l - m_r).
// A row is kept when 0 <= y_r < V and y_r != ignore_index; `kept` is their number, counted on the device in front of the first chunk
// (head_kept_parts / _final, mot_headcore.hip) and never read on the host.
//   loss    = (sum over kept rows of (lse_r - l_r[y_r])) / kept        fixed-order double sum; NaN at kept == 0, as torch
//   G_r     = (c_r / kept) (softmax(l_r) - onehot(y_r)) for a kept row, else a row of zeros,   u = G W,   dW = G^T x,
//   dx_r    = u_r - c_r^2 (x_r . u_r / D) x_r  (norm_in),  u_r (else)
// A target equal to ignore_index drops its row silently; any other target outside [0, V) drops it and raises MOT_STATUS_TARGET_OOR.
//
// The chunks, the three products, the row chain and the loss's sum are the token-level head's (mot_tokhead.hip, mot_headcore.hpp).
// New is plainhead_rows, the V-wide row pass for logits without a bound.  It has tokhead_rows' shape, one workgroup per row, the
// row's 16-byte vectors in registers, every load issued before anything waits, G written over the logits from the same registers,
// but it cannot take lse from a constant maximum: the row's maximum is a workgroup max (rows_block_max), then sum exp(l - m) comes
// from the registers.  Rows above 65 536 classes do not fit the registers: their first sweep carries an online (m, sum) pair per
// thread, which the workgroup's max and one rescale per thread merge in a fixed order, so such a row is read twice (statistics, then
// gradient), not three times.  The divisor 1 / kept is read from device memory.
#include "mot_headrows.hpp"

namespace mot {
namespace {

// One workgroup per row of the chunk; NV as in tokhead_rows (NV > 0: the row stays in registers, NV == 0: it is read twice).
// EVAL (never with GRAD): the sweep also carries the row's largest stored logit with its class and the count of stored logits
// above the target's.  `kept` is read only with GRAD.
template <typename T, int NV, bool GRAD, bool EVAL>
__global__ __launch_bounds__(kRowThreads) void plainhead_rows(T *S, int V, const T *__restrict__ x, int K, int norm_in, float eps,
                                                              const int64_t *__restrict__ tgt, int64_t ignore, int64_t rows,
                                                              const long long *__restrict__ kept, float *__restrict__ term, uint32_t *status,
                                                              HeadEvalRows ev) {
    typedef LogitVec<T> Vec;
    __shared__ float sh_ss[kRowWavesMax], sh_m[kRowWavesMax], sh_se[kRowWavesMax], sh_ly[kRowWavesMax];
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
    const bool in_range = y >= 0 && y < V, keep = in_range && y != ignore;
    const int yvec = in_range ? (int)(y / Vec::N) : -1, yel = in_range ? (int)(y % Vec::N) : -1;
    float sy = 0.f, best = -INFINITY;   // EVAL: the target's stored logit, the largest of this thread's
    int best_cls = 0x7fffffff, above = 0;
    if (EVAL && in_range) sy = (float)S[r * (int64_t)V + y];
    float m = -INFINITY, se = 0.f, ly = 0.f;   // the thread's largest l, its sum exp(l - m), l[y] in the one thread that meets it
    if (NV > 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = tid + i * nt;
            if (idx < nvec) {
#pragma unroll
                for (int e = 0; e < Vec::N; ++e) {
                    const float l = c * a[i].get(e);
                    m = fmaxf(m, l);
                    if (idx == yvec && e == yel) ly = l;
                }
                if (EVAL) vec_top<T>(a[i], idx * Vec::N, sy, best, best_cls, above);
            }
        }
        m = rows_block_max(m, sh_m);   // the row's maximum, then the sum from the registers
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = tid + i * nt;
            if (idx < nvec) {
#pragma unroll
                for (int e = 0; e < Vec::N; ++e) se += __expf(c * a[i].get(e) - m);
            }
        }
    } else {   // one sweep: the thread's online pair (every thread meets at least one vector: nvec > kRegV / 8 >= blockDim.x)
        for (int idx = tid; idx < nvec; idx += nt) {
            const Vec v = row[idx];
            float l[Vec::N], vm = -INFINITY;
#pragma unroll
            for (int e = 0; e < Vec::N; ++e) {
                l[e] = c * v.get(e);
                vm = fmaxf(vm, l[e]);
                if (idx == yvec && e == yel) ly = l[e];
            }
            if (vm > m) {   // exp(-inf) = 0 at the first vector, where se = 0
                se *= __expf(m - vm);
                m = vm;
            }
#pragma unroll
            for (int e = 0; e < Vec::N; ++e) se += __expf(l[e] - m);
            if (EVAL) vec_top<T>(v, idx * Vec::N, sy, best, best_cls, above);
        }
        const float mt = m;   // the pairs merge in a fixed order: the workgroup's max, one rescale per thread, the fixed-order sum
        m = rows_block_max(mt, sh_m);
        se *= __expf(mt - m);
    }
    if (EVAL) {   // the waves' pairs, met in wave order behind the next sum's barrier
        wave_argmax(best, best_cls);
        if ((tid & 63) == 0) {
            sh_top[tid >> 6] = best;
            sh_cls[tid >> 6] = best_cls;
        }
    }
    se = rows_block_sum(se, sh_se);
    ly = rows_block_sum(ly, sh_ly);   // one thread holds l[y], the others 0
    // lse = m + log(se) is never formed: at logits of a few hundred its rounding (2^-16 at 300) would sit in every exp(l - lse) of the
    // row and in the loss term, so both subtract m first, as log_softmax does
    const float lg = __logf(se), row_term = (m - ly) + lg;
    if (tid == 0) {
        term[r] = keep ? row_term : 0.f;
        if (!in_range && y != ignore && status) atomicOr(status, (uint32_t)MOT_STATUS_TARGET_OOR);
    }
    if (EVAL) {
        const float n_above = rows_block_sum((float)above, sh_above);   // at most kMaxV = 2^18: exact in fp32
        if (tid == 0) {
            for (int w = 1; w < (nt >> 6); ++w) argmax_take(best, best_cls, sh_top[w], sh_cls[w]);   // thread 0 holds wave 0's pair
            if (ev.row_loss) ev.row_loss[r] = keep ? row_term : 0.f;
            if (ev.pred) ev.pred[r] = best_cls;
            if (ev.rank) ev.rank[r] = keep ? (int)n_above : -1;
        }
    }
    if (!GRAD) return;
    // G = (c / kept) (exp((l - m) - log(se)) - onehot); a dropped row is a row of zeros whatever its logits hold
    const float scale = keep ? c / (float)*kept : 0.f;
    float mg = m;   // the same value behind an opaque copy: sharing l - m with the sum's sweep would hold a second row in registers
    asm volatile("" : "+v"(mg));
    if (NV > 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = tid + i * nt;
            if (idx < nvec) {
                float g[Vec::N];
#pragma unroll
                for (int e = 0; e < Vec::N; ++e) {
                    const float p = __expf((c * a[i].get(e) - mg) - lg);
                    g[e] = keep ? scale * (p - (idx == yvec && e == yel ? 1.f : 0.f)) : 0.f;
                }
                a[i].put(g);
                row[idx] = a[i];
            }
        }
    } else {
        for (int idx = tid; idx < nvec; idx += nt) {
            Vec v = row[idx];
            float g[Vec::N];
#pragma unroll
            for (int e = 0; e < Vec::N; ++e) {
                const float p = __expf((c * v.get(e) - mg) - lg);
                g[e] = keep ? scale * (p - (idx == yvec && e == yel ? 1.f : 0.f)) : 0.f;
            }
            v.put(g);
            row[idx] = v;
        }
    }
}

struct PlainGeom {
    int64_t rows, chunk, ignore;
    int K, V, norm_in, group;
    bool bf16, grad_x;
    float eps;
};

struct PlainWs {   // carve of the workspace, offsets in bytes
    size_t term, part, kept, S, u, WT, total;
};

PlainWs plain_ws(const PlainGeom &g) {
    Arena a;
    PlainWs w{};
    w.term = a.take((size_t)g.rows * 4);
    w.part = a.take((size_t)kLossParts * 8);
    w.kept = a.take(8);
    w.S = a.take((size_t)g.chunk * g.V * (g.bf16 ? 2 : 4));
    w.u = a.take(g.grad_x ? (size_t)g.chunk * g.K * 4 : 0);
    w.WT = a.take(g.grad_x && g.bf16 ? (size_t)g.V * g.K * 2 : 0);
    w.total = a.o;
    return w;
}

// the row pass of one chunk: workgroup size and registers per thread as in the token-level head's launch_rows
template <typename T, bool GRAD, bool EVAL = false>
int launch_plain_rows(T *S, const PlainGeom &g, const T *x, const int64_t *tgt, int64_t n, const long long *kept, float *term, uint32_t *status,
                      hipStream_t stream, HeadEvalRows ev = {}) {
    int nt, nv;
    rows_geometry<T>(g.V, nt, nv);
#define MOT_PLAINHEAD_ROWS(NV)                                                                                                                    \
    hipLaunchKernelGGL((plainhead_rows<T, NV, GRAD, EVAL>), dim3((unsigned)n), dim3(nt), 0, stream, S, g.V, x, g.K, g.norm_in, g.eps, tgt, g.ignore, n, \
                       kept, term, status, ev)
    if (nv <= 4) MOT_PLAINHEAD_ROWS(4);
    else if (nv <= 8) MOT_PLAINHEAD_ROWS(8);
    else if (g.V <= kRegV) MOT_PLAINHEAD_ROWS(kRegV / (kRowThreads * LogitVec<T>::N));   // 16 in fp32 (bf16 rows this wide took 8 above)
    else MOT_PLAINHEAD_ROWS(0);
#undef MOT_PLAINHEAD_ROWS
    return check_launch("plainhead_rows");
}

int plain_head_geom(const MotPlainHeadDesc *d, PlainGeom *out, const char *fn) {
    if (!d) return set_error(MOT_EINVAL, "%s: null descriptor", fn);
    if (d->struct_size != sizeof(MotPlainHeadDesc))
        return set_error(MOT_EINVAL, "%s: struct_size %u != %zu (ABI mismatch)", fn, d->struct_size, sizeof(MotPlainHeadDesc));
    if (d->dtype != MOT_F32 && d->dtype != MOT_BF16) return set_error(MOT_EUNSUPPORTED, "%s: dtype %d is not built", fn, d->dtype);
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
    if (d->group_rows < 0 || (d->group_rows > 0 && d->n_rows % d->group_rows))
        return set_error(MOT_ESHAPE, "%s: group_rows %d must be 0 (no groups) or divide n_rows %lld", fn, d->group_rows, (long long)d->n_rows);
    PlainGeom &g = *out;
    g.rows = d->n_rows;
    g.K = d->model_dim;
    g.V = d->vocab;
    g.norm_in = d->norm_in ? 1 : 0;
    g.group = d->group_rows;
    g.ignore = d->ignore_index;
    g.bf16 = d->dtype == MOT_BF16;
    g.grad_x = d->dx != nullptr;
    g.eps = d->eps > 0.f ? d->eps : kHeadEps;
    if (d->chunk_rows)
        g.chunk = g.rows < d->chunk_rows ? g.rows : d->chunk_rows;
    else   // the library's choice: a chunk's logits and u stay below kChunkBytes
        g.chunk = head_chunk_rows(kChunkBytes, (int64_t)g.V * (g.bf16 ? 2 : 4) + (int64_t)g.K * 4, g.rows);
    return MOT_OK;
}

// `ev` set: the evaluation call (no gradients): its row pass also writes ev's rows, and the counts are closed behind the loss
template <typename T>
int plain_head_run(const MotPlainHeadDesc &d, const PlainGeom &g, const PlainWs &w, const MotHeadEvalOut *ev, hipStream_t stream) {
    constexpr bool BF = sizeof(T) == 2;
    unsigned char *ws = (unsigned char *)d.workspace;
    float *term = (float *)(ws + w.term), *u = (float *)(ws + w.u);
    long long *kept = (long long *)(ws + w.kept);
    T *S = (T *)(ws + w.S), *WT = (T *)(ws + w.WT);
    const T *X = (const T *)d.x, *W = (const T *)d.weight;
    const bool grad = d.dx || d.dW;
    const HeadEvalRows ev_rows = ev ? HeadEvalRows{ev->row_loss, ev->pred, ev->rank} : HeadEvalRows{};
    int rc;
    if ((rc = launch_head_kept(d.targets, g.rows, g.V, g.ignore, ws + w.part, kept, stream))) return rc;   // the row pass divides by it
    if (d.dW && (rc = launch_zero_words(d.dW, (int64_t)g.V * g.K, stream))) return rc;
    if (BF && d.dx && (rc = launch_transpose_bf16(W, g.V, g.K, WT, stream))) return rc;   // WT[k][v]: the operand of u = G W on the bf16 launcher
    for (int64_t r0 = 0; r0 < g.rows; r0 += g.chunk) {
        const int64_t n = g.rows - r0 < g.chunk ? g.rows - r0 : g.chunk;
        const T *x = X + r0 * g.K;
        if ((rc = launch_product_nt(head_dtype<T>, x, g.K, n, W, g.K, g.K, g.V, S, g.V, BF, nullptr, false, stream))) return rc;   // s = x W^T for the chunk's rows, in T
        if (ev)
            rc = launch_plain_rows<T, false, true>(S, g, x, d.targets + r0, n, kept, term + r0, d.status, stream, ev_rows.at(r0));
        else if (grad)
            rc = launch_plain_rows<T, true>(S, g, x, d.targets + r0, n, kept, term + r0, d.status, stream);
        else
            rc = launch_plain_rows<T, false>(S, g, x, d.targets + r0, n, kept, term + r0, d.status, stream);
        if (rc) return rc;
        if (d.dx) {   // u = G W, then the row chain of the plain norm (L = 0)
            if ((rc = launch_product_nn(head_dtype<T>, S, g.V, n, BF ? WT : W, BF ? g.V : g.K, g.V, g.K, u, g.K, stream))) return rc;
            if ((rc = launch_head_chain<T>(x, u, g.K, n, 0, g.norm_in, g.eps, (T *)d.dx + r0 * g.K, stream))) return rc;
        }
        if (d.dW && (rc = launch_product_tn(head_dtype<T>, S, g.V, g.V, x, g.K, g.K, n, d.dW, g.K, stream))) return rc;   // dW += G^T x
    }
    if ((rc = launch_head_loss_kept(term, g.rows, (double *)(ws + w.part), kept, d.loss, stream))) return rc;
    if (ev && ev->counts) {   // per row, or per group of group_rows rows with the dropped rows left out of their groups
        const int per = g.group > 0 ? g.group : 1;
        return launch_head_eval_counts(ev->pred, d.targets, g.rows / per, per, g.V, ws + w.part, ev->counts, g.group > 0 ? 3 : 2, stream, 1, g.ignore);
    }
    return MOT_OK;
}

// the checks behind the descriptor's own, then the launches; `fn` starts the messages
int plain_head_launch(const MotPlainHeadDesc &d, const PlainGeom &g, const MotHeadEvalOut *ev, const char *fn, hipStream_t stream) {
    if (!d.x || !d.weight || !d.targets || !d.loss) return set_error(MOT_EINVAL, "%s: null x / weight / targets / loss", fn);
    if (g.rows == 0) return set_error(MOT_ESHAPE, "%s: no rows (the mean over zero targets is undefined)", fn);
    const PlainWs w = plain_ws(g);
    if (!d.workspace || d.workspace_bytes < w.total)
        return set_error(MOT_EWORKSPACE, "%s: workspace %zu bytes < %zu", fn, d.workspace ? d.workspace_bytes : (size_t)0, w.total);
    if (((uintptr_t)d.x & 15) || ((uintptr_t)d.weight & 15) || ((uintptr_t)d.workspace & 15) || ((uintptr_t)d.dx & 15) || ((uintptr_t)d.dW & 15))
        return set_error(MOT_EUNSUPPORTED, "%s: x, weight, workspace, dx and dW must be 16-byte aligned", fn);
    return g.bf16 ? plain_head_run<__bf16>(d, g, w, ev, stream) : plain_head_run<float>(d, g, w, ev, stream);
}

}  // namespace

size_t plain_head_workspace_bytes(const MotPlainHeadDesc *d) {
    PlainGeom g;
    if (plain_head_geom(d, &g, "mot_plain_head_workspace_bytes") || g.rows == 0) return 0;
    return plain_ws(g).total;
}

int launch_plain_head_fwd(const MotPlainHeadDesc *d, hipStream_t stream) {
    static const char fn[] = "mot_plain_head_fwd";
    PlainGeom g;
    if (int rc = plain_head_geom(d, &g, fn)) return rc;
    return plain_head_launch(*d, g, nullptr, fn, stream);
}

int launch_plain_head_eval(const MotPlainHeadDesc *d, const MotHeadEvalOut *out, hipStream_t stream) {
    static const char fn[] = "mot_plain_head_eval";
    PlainGeom g;
    int rc = plain_head_geom(d, &g, fn);
    if (rc || (rc = head_eval_check(fn, out))) return rc;
    if (d->dx || d->dW) return set_error(MOT_EINVAL, "%s: dx / dW set: the evaluation forms no gradients (mot_plain_head_fwd does)", fn);
    return plain_head_launch(*d, g, out, fn, stream);
}

}  // namespace mot
