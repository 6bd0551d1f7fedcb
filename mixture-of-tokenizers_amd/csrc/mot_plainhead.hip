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
// The compacted form (mot_plain_head_compact_*, second half of this file) runs the same products and row pass on the kept rows
// alone, gathered behind a bound the caller gives.
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

// ---- The compacted form (mot_plain_head_compact_*): the kept rows are gathered into slots 0 .. kept-1 behind the caller's bound
// cap = min(max_kept, n_rows), normed in the gather, and the products and the row pass above run per slot (the row pass without a
// factor); the row chain writes through the index into dx.  Every grid and the workspace
// depend on (n_rows, cap, chunk) alone; what depends on the targets is read on the device: the count `kept` (published as 0 on
// overflow, so that every slot is padding and no later kernel has a special case) and idx[0, kept), the kept rows in ascending order.
//
// The index pass is a stable compaction in three launches, none of which waits on another workgroup: compact_count (workgroup p
// counts the kept rows of its fixed range of rows), compact_scan (one wave turns the counts into exclusive offsets, publishes kept
// and the overflow bit), compact_write (workgroup p walks its range again in tiles of kThreads rows and writes its rows' numbers
// from its offset on, ranked by ballot and popcount inside the wave and by the waves' totals in LDS across the waves).
inline int compact_parts(int64_t rows) {
    const int64_t p = (rows + 2047) / 2048;
    return (int)(p < 1 ? 1 : p > kLossParts ? kLossParts : p);
}

__global__ __launch_bounds__(kThreads) void compact_count(const int64_t *__restrict__ tgt, int64_t rows, int vocab, int64_t ignore,
                                                          long long *__restrict__ cnt, uint32_t *status) {
    __shared__ int sh_n[kWaves], sh_oor[kWaves];
    const int tid = threadIdx.x;
    const int64_t per = (rows + gridDim.x - 1) / gridDim.x, lo = (int64_t)blockIdx.x * per, hi = lo + per < rows ? lo + per : rows;
    int n = 0, oor = 0;   // wave-uniform: the ballots' popcounts
    for (int64_t b = lo; b < hi; b += kThreads) {
        const int64_t i = b + tid;
        const int64_t y = i < hi ? tgt[i] : ignore;
        const bool in = y >= 0 && y < vocab;
        n += __popcll(__ballot(in && y != ignore));
        oor |= __ballot(!in && y != ignore) != 0;
    }
    if ((tid & 63) == 0) {
        sh_n[tid >> 6] = n;
        sh_oor[tid >> 6] = oor;
    }
    __syncthreads();
    if (tid == 0) {
        long long a = 0;
        int o = 0;
        for (int w = 0; w < kWaves; ++w) {
            a += sh_n[w];
            o |= sh_oor[w];
        }
        cnt[blockIdx.x] = a;
        if (o && status) atomicOr(status, (uint32_t)MOT_STATUS_TARGET_OOR);
    }
}

// cnt[0, parts) -> exclusive offsets in place; *kept = the total, or 0 when it exceeds cap (with the overflow bit)
__global__ __launch_bounds__(64) void compact_scan(long long *__restrict__ cnt, int parts, long long cap, long long *__restrict__ kept,
                                                   uint32_t *status) {
    constexpr int kPer = kLossParts / 64;
    const int lane = threadIdx.x;
    long long v[kPer], s = 0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int p = lane * kPer + j;
        v[j] = p < parts ? cnt[p] : 0;
        s += v[j];
    }
    long long incl = s;
    for (int o = 1; o < 64; o <<= 1) {
        const long long t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    long long run = incl - s;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int p = lane * kPer + j;
        if (p < parts) cnt[p] = run;
        run += v[j];
    }
    if (lane == 63) {
        *kept = incl > cap ? 0 : incl;
        if (incl > cap && status) atomicOr(status, (uint32_t)MOT_STATUS_KEPT_OVERFLOW);
    }
}

__global__ __launch_bounds__(kThreads) void compact_write(const int64_t *__restrict__ tgt, int64_t rows, int vocab, int64_t ignore,
                                                          const long long *__restrict__ off, const long long *__restrict__ kept, long long cap,
                                                          int32_t *__restrict__ idx) {
    __shared__ int sh[kWaves];
    if (*kept == 0) return;   // nothing kept, or overflow: no slot is valid and idx is never read
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t per = (rows + gridDim.x - 1) / gridDim.x, lo = (int64_t)blockIdx.x * per, hi = lo + per < rows ? lo + per : rows;
    long long base = off[blockIdx.x];
    for (int64_t b = lo; b < hi; b += kThreads) {
        const int64_t i = b + tid;
        const int64_t y = i < hi ? tgt[i] : ignore;
        const bool keep = y >= 0 && y < vocab && y != ignore;
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) sh[wave] = __popcll(mask);
        __syncthreads();
        int before = __popcll(mask & ((1ull << lane) - 1ull)), total = 0;
        for (int w = 0; w < kWaves; ++w) {
            before += w < wave ? sh[w] : 0;
            total += sh[w];
        }
        const long long slot = base + before;
        if (keep && slot < cap) idx[slot] = (int32_t)i;   // slot < kept <= cap by the scan; the bound is kept in sight
        base += total;
        __syncthreads();   // sh is rewritten by the next tile
    }
}

int launch_compact_index(const int64_t *tgt, int64_t rows, int vocab, int64_t ignore, int64_t cap, long long *scan, long long *kept, int32_t *idx,
                         uint32_t *status, hipStream_t stream) {
    const int parts = compact_parts(rows);
    hipLaunchKernelGGL(compact_count, dim3(parts), dim3(kThreads), 0, stream, tgt, rows, vocab, ignore, scan, status);
    if (int rc = check_launch("compact_count")) return rc;
    hipLaunchKernelGGL(compact_scan, dim3(1), dim3(64), 0, stream, scan, parts, (long long)cap, kept, status);
    if (int rc = check_launch("compact_scan")) return rc;
    hipLaunchKernelGGL(compact_write, dim3(parts), dim3(kThreads), 0, stream, tgt, rows, vocab, ignore, (const long long *)scan, (const long long *)kept,
                       (long long)cap, idx);
    return check_launch("compact_write");
}

// One wave per slot of the chunk [s0, s0 + n): its row as the products take it, and its target.  With norm_in the row is normed
// HERE, hg = T(c x) with c = (mean(x^2) + eps)^-1/2 in fp32, and rounded to the call's dtype as F.rms_norm's output is in front of
// lm_head: the row pass then runs without a factor on l = hg W^T, so in bf16 the logits carry the reference's own two roundings
// (norm(x), then the product) instead of a product of the un-normed row scaled in fp32.  A slot at or beyond the device count is
// compared first and never reads idx (stale or uninitialised there): it gets a zero row and the ignored target.
template <typename T>
__global__ __launch_bounds__(kThreads) void compact_gather(const T *__restrict__ x, int K, int norm_in, float eps, const int64_t *__restrict__ tgt,
                                                           const int32_t *__restrict__ idx, const long long *__restrict__ kept, int64_t s0, int64_t n,
                                                           int64_t ignore, T *__restrict__ hg, int64_t *__restrict__ tg) {
    const int lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (j >= n) return;
    const bool valid = s0 + j < *kept;   // wave-uniform
    T *out = hg + j * K;
    if (!valid) {
        for (int k = lane; k < K; k += 64) out[k] = (T)0.f;
        if (lane == 0) tg[j] = ignore;
        return;
    }
    const int64_t r = idx[s0 + j];
    const T *xr = x + r * K;
    float c = 1.f;
    if (norm_in) {
        float ss = 0.f, dc;
        for (int k = lane; k < K; k += 64) {
            const float v = (float)xr[k];
            ss += v * v;
        }
        row_scale(wave_sum(ss) / (float)K, 0, eps, c, dc);
    }
    for (int k = lane; k < K; k += 64) out[k] = norm_in ? (T)(c * (float)xr[k]) : xr[k];
    if (lane == 0) tg[j] = tgt[r];
}

// The row chain and the scatter in one pass, one wave per valid slot of the chunk: with u = G W for G = dloss / dl on l = hg W^T
// (no factor inside), dx[idx[s]] = c u - c^3 (x . u / K) x for the norm's c of the row's own x (read in place, not gathered), else
// dx[idx[s]] = u (not u + 0 x: a non-finite x stays out of dx).  fp32 arithmetic, one rounding on store.
template <typename T>
__global__ __launch_bounds__(kThreads) void compact_chain_scatter(const T *__restrict__ x, const float *__restrict__ u, int K, int norm_in, float eps,
                                                                  const int32_t *__restrict__ idx, const long long *__restrict__ kept, int64_t s0,
                                                                  int64_t n, T *__restrict__ dx) {
    const int lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (j >= n || s0 + j >= *kept) return;
    const int64_t r = idx[s0 + j];
    const T *xr = x + r * K;
    const float *ur = u + j * K;
    T *out = dx + r * K;
    if (!norm_in) {
        for (int k = lane; k < K; k += 64) out[k] = (T)ur[k];
        return;
    }
    float ss = 0.f, xu = 0.f;
    for (int k = lane; k < K; k += 64) {
        const float a = (float)xr[k];
        ss += a * a;
        xu += a * ur[k];
    }
    ss = wave_sum(ss);
    xu = wave_sum(xu);
    float c, dc;
    row_scale(ss / (float)K, 0, eps, c, dc);
    const float coef = 2.f * dc * xu / (float)K;   // dc = -c^3 / 2 at L = 0
    for (int k = lane; k < K; k += 64) out[k] = (T)(c * ur[k] + coef * (float)xr[k]);
}

// +0 into every element of the rows of dx the scatter does not write: decided per row from its target (and every row when the
// count is 0: nothing kept, or overflow), so no row is written twice.  One wave per row.
__global__ __launch_bounds__(kThreads) void compact_zero_dropped(const int64_t *__restrict__ tgt, int64_t rows, int vocab, int64_t ignore,
                                                                 const long long *__restrict__ kept, int vecs, uint4 *__restrict__ dx) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int64_t y = tgt[r];
    if (y >= 0 && y < vocab && y != ignore && *kept != 0) return;
    for (int k = lane; k < vecs; k += 64) dx[r * vecs + k] = make_uint4(0u, 0u, 0u, 0u);
}

// The evaluation's per-row outputs: thread i writes (0, -1, -1) for a dropped row i and carries slot i's triple to its row
__global__ __launch_bounds__(kThreads) void compact_eval_rows(const int64_t *__restrict__ tgt, int64_t rows, int vocab, int64_t ignore,
                                                              const int32_t *__restrict__ idx, const long long *__restrict__ kept, HeadEvalRows slot,
                                                              HeadEvalRows out) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const long long n = *kept;
    if (i < rows) {
        const int64_t y = tgt[i];
        if (!(y >= 0 && y < vocab && y != ignore && n != 0)) {
            if (out.row_loss) out.row_loss[i] = 0.f;
            if (out.pred) out.pred[i] = -1;
            if (out.rank) out.rank[i] = -1;
        }
    }
    if (i < n) {
        const int64_t r = idx[i];
        if (out.row_loss) out.row_loss[r] = slot.row_loss[i];
        if (out.pred) out.pred[r] = slot.pred[i];
        if (out.rank) out.rank[r] = slot.rank[i];
    }
}

struct CompactWs {   // carve of the compacted call's workspace, offsets in bytes (Arena: every piece starts on 256 bytes)
    size_t term, part, kept, scan, idx, tg, hg, S, u, WT, ev_loss, ev_pred, ev_rank, total;
};

// g.chunk is the chunk over cap
CompactWs compact_ws(const PlainGeom &g, int64_t cap) {
    const size_t e = g.bf16 ? 2 : 4;
    Arena a;
    CompactWs w{};
    w.term = a.take((size_t)cap * 4);
    w.part = a.take((size_t)kLossParts * 8);
    w.kept = a.take(8);
    w.scan = a.take((size_t)kLossParts * 8);
    w.idx = a.take((size_t)cap * 4);
    w.tg = a.take((size_t)g.chunk * 8);
    w.hg = a.take((size_t)g.chunk * g.K * e);
    w.S = a.take((size_t)g.chunk * g.V * e);
    w.u = a.take(g.grad_x ? (size_t)g.chunk * g.K * 4 : 0);
    w.WT = a.take(g.grad_x && g.bf16 ? (size_t)g.V * g.K * 2 : 0);
    w.ev_loss = a.take((size_t)cap * 4);   // the evaluation's per-slot rows; 12 bytes a slot, carved for both calls so that one query serves them
    w.ev_pred = a.take((size_t)cap * 4);
    w.ev_rank = a.take((size_t)cap * 4);
    w.total = a.o;
    return w;
}

// the descriptor's checks, the compact struct's, then cap and the chunk over cap
int compact_geom(const MotPlainHeadDesc *d, const MotPlainHeadCompact *c, PlainGeom *g, int64_t *cap, const char *fn) {
    if (int rc = plain_head_geom(d, g, fn)) return rc;
    if (!c) return set_error(MOT_EINVAL, "%s: null compact struct", fn);
    if (c->struct_size != sizeof(MotPlainHeadCompact))
        return set_error(MOT_EINVAL, "%s: compact struct_size %u != %zu (ABI mismatch)", fn, c->struct_size, sizeof(MotPlainHeadCompact));
    if (c->reserved) return set_error(MOT_EINVAL, "%s: compact reserved %u must be 0", fn, c->reserved);
    if (c->max_kept <= 0) return set_error(MOT_ESHAPE, "%s: max_kept %lld must be positive", fn, (long long)c->max_kept);
    *cap = c->max_kept < g->rows ? c->max_kept : g->rows;
    if (d->chunk_rows)
        g->chunk = *cap < d->chunk_rows ? *cap : d->chunk_rows;
    else
        g->chunk = head_chunk_rows(kChunkBytes, (int64_t)g->V * (g->bf16 ? 2 : 4) + (int64_t)g->K * 4, *cap);
    return MOT_OK;
}

template <typename T>
int compact_run(const MotPlainHeadDesc &d, const PlainGeom &g, int64_t cap, const CompactWs &w, const MotHeadEvalOut *ev, hipStream_t stream) {
    constexpr bool BF = sizeof(T) == 2;
    unsigned char *ws = (unsigned char *)d.workspace;
    float *term = (float *)(ws + w.term), *u = (float *)(ws + w.u);
    long long *kept = (long long *)(ws + w.kept), *scan = (long long *)(ws + w.scan);
    int32_t *idx = (int32_t *)(ws + w.idx);
    int64_t *tg = (int64_t *)(ws + w.tg);
    T *S = (T *)(ws + w.S), *WT = (T *)(ws + w.WT), *hg = (T *)(ws + w.hg);
    const T *X = (const T *)d.x, *W = (const T *)d.weight;
    const bool grad = d.dx || d.dW;
    PlainGeom gr = g;   // the row pass sees rows that are normed already
    gr.norm_in = 0;
    const int vecs = g.K * (int)sizeof(T) / 16;   // model_dim is a multiple of 16: whole 16-byte vectors in both dtypes
    const HeadEvalRows slot_rows{(float *)(ws + w.ev_loss), (int32_t *)(ws + w.ev_pred), (int32_t *)(ws + w.ev_rank)};
    const auto wave_grid = [](int64_t n) { return dim3((unsigned)((n + kWaves - 1) / kWaves)); };
    int rc;
    if ((rc = launch_compact_index(d.targets, g.rows, g.V, g.ignore, cap, scan, kept, idx, d.status, stream))) return rc;
    if (d.dW && (rc = launch_zero_words(d.dW, (int64_t)g.V * g.K, stream))) return rc;
    if (d.dx) {
        hipLaunchKernelGGL(compact_zero_dropped, wave_grid(g.rows), dim3(kThreads), 0, stream, d.targets, g.rows, g.V, g.ignore, (const long long *)kept, vecs,
                           (uint4 *)d.dx);
        if ((rc = check_launch("compact_zero_dropped"))) return rc;
    }
    if (BF && d.dx && (rc = launch_transpose_bf16(W, g.V, g.K, WT, stream))) return rc;
    for (int64_t s0 = 0; s0 < cap; s0 += g.chunk) {
        const int64_t n = cap - s0 < g.chunk ? cap - s0 : g.chunk;
        hipLaunchKernelGGL(compact_gather<T>, wave_grid(n), dim3(kThreads), 0, stream, X, g.K, g.norm_in, g.eps, d.targets, (const int32_t *)idx,
                           (const long long *)kept, s0, n, g.ignore, hg, tg);
        if ((rc = check_launch("compact_gather"))) return rc;
        if ((rc = launch_product_nt(head_dtype<T>, hg, g.K, n, W, g.K, g.K, g.V, S, g.V, BF, nullptr, false, stream))) return rc;   // l = hg W^T
        if (ev)
            rc = launch_plain_rows<T, false, true>(S, gr, hg, tg, n, kept, term + s0, nullptr, stream, slot_rows.at(s0));
        else if (grad)
            rc = launch_plain_rows<T, true>(S, gr, hg, tg, n, kept, term + s0, nullptr, stream);
        else
            rc = launch_plain_rows<T, false>(S, gr, hg, tg, n, kept, term + s0, nullptr, stream);
        if (rc) return rc;
        if (d.dx) {   // u = G W, then the row chain of each valid slot straight into its row of dx
            if ((rc = launch_product_nn(head_dtype<T>, S, g.V, n, BF ? WT : W, BF ? g.V : g.K, g.V, g.K, u, g.K, stream))) return rc;
            hipLaunchKernelGGL(compact_chain_scatter<T>, wave_grid(n), dim3(kThreads), 0, stream, X, (const float *)u, g.K, g.norm_in, g.eps,
                               (const int32_t *)idx, (const long long *)kept, s0, n, (T *)d.dx);
            if ((rc = check_launch("compact_chain_scatter"))) return rc;
        }
        if (d.dW && (rc = launch_product_tn(head_dtype<T>, S, g.V, g.V, hg, g.K, g.K, n, d.dW, g.K, stream))) return rc;   // dW += G^T hg
    }
    if ((rc = launch_head_loss_kept(term, cap, (double *)(ws + w.part), kept, d.loss, stream))) return rc;
    if (!ev) return MOT_OK;
    if (ev->row_loss || ev->pred || ev->rank) {
        const int64_t span = g.rows > cap ? g.rows : cap;
        hipLaunchKernelGGL(compact_eval_rows, dim3((unsigned)((span + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, d.targets, g.rows, g.V, g.ignore,
                           (const int32_t *)idx, (const long long *)kept, slot_rows, HeadEvalRows{ev->row_loss, ev->pred, ev->rank});
        if ((rc = check_launch("compact_eval_rows"))) return rc;
    }
    if (ev->counts) {   // from the per-row pred: a dropped row's -1 is never compared
        const int per = g.group > 0 ? g.group : 1;
        return launch_head_eval_counts(ev->pred, d.targets, g.rows / per, per, g.V, ws + w.part, ev->counts, g.group > 0 ? 3 : 2, stream, 1, g.ignore);
    }
    return MOT_OK;
}

int compact_launch(const MotPlainHeadDesc &d, const PlainGeom &g, int64_t cap, const MotHeadEvalOut *ev, const char *fn, hipStream_t stream) {
    if (!d.x || !d.weight || !d.targets || !d.loss) return set_error(MOT_EINVAL, "%s: null x / weight / targets / loss", fn);
    if (g.rows == 0) return set_error(MOT_ESHAPE, "%s: no rows (the mean over zero targets is undefined)", fn);
    const CompactWs w = compact_ws(g, cap);
    if (!d.workspace || d.workspace_bytes < w.total)
        return set_error(MOT_EWORKSPACE, "%s: workspace %zu bytes < %zu", fn, d.workspace ? d.workspace_bytes : (size_t)0, w.total);
    if (((uintptr_t)d.x & 15) || ((uintptr_t)d.weight & 15) || ((uintptr_t)d.workspace & 15) || ((uintptr_t)d.dx & 15) || ((uintptr_t)d.dW & 15))
        return set_error(MOT_EUNSUPPORTED, "%s: x, weight, workspace, dx and dW must be 16-byte aligned", fn);
    return g.bf16 ? compact_run<__bf16>(d, g, cap, w, ev, stream) : compact_run<float>(d, g, cap, w, ev, stream);
}

}  // namespace

size_t plain_head_compact_workspace_bytes(const MotPlainHeadDesc *d, const MotPlainHeadCompact *c) {
    PlainGeom g;
    int64_t cap;
    if (compact_geom(d, c, &g, &cap, "mot_plain_head_compact_workspace_bytes") || g.rows == 0) return 0;
    return compact_ws(g, cap).total;
}

int launch_plain_head_compact_fwd(const MotPlainHeadDesc *d, const MotPlainHeadCompact *c, hipStream_t stream) {
    static const char fn[] = "mot_plain_head_compact_fwd";
    PlainGeom g;
    int64_t cap;
    if (int rc = compact_geom(d, c, &g, &cap, fn)) return rc;
    return compact_launch(*d, g, cap, nullptr, fn, stream);
}

int launch_plain_head_compact_eval(const MotPlainHeadDesc *d, const MotPlainHeadCompact *c, const MotHeadEvalOut *out, hipStream_t stream) {
    static const char fn[] = "mot_plain_head_compact_eval";
    PlainGeom g;
    int64_t cap;
    int rc = compact_geom(d, c, &g, &cap, fn);
    if (rc || (rc = head_eval_check(fn, out))) return rc;
    if (d->dx || d->dW) return set_error(MOT_EINVAL, "%s: dx / dW set: the evaluation forms no gradients (mot_plain_head_compact_fwd does)", fn);
    return compact_launch(*d, g, cap, out, fn, stream);
}

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
