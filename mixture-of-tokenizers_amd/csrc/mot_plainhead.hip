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
// The chunks, the three products, the row chain and the loss's sum are the V-wide heads' one chunk loop (wide_run, mot_widehead.hpp).
// This unit holds PlainStat, the arithmetic of the shared row pass wide_rows (mot_headrows.hpp) for logits without a bound.  It
// cannot take lse from a constant maximum: the row's maximum is a workgroup max (rows_block_max), then sum exp(l - m) comes from the
// registers.  Rows above 65 536 classes do not fit the registers: their first sweep carries an online (m, sum) pair per thread, which
// the workgroup's max and one rescale per thread merge in a fixed order, so such a row is read twice (statistics, then gradient),
// not three times.  The divisor 1 / kept is read from device memory.
// The compacted form (mot_plain_head_compact_*, second half of this file) runs the same loop on the kept rows alone, gathered
// behind a bound the caller gives; its index pass, gather and scatter are the loop's compaction context.
#include "mot_widehead.hpp"

namespace mot {
namespace {

// The plain head's share of wide_rows.  A row is kept when its target is in range and not `ignore`; the divisor is the device
// count *kept, read only with GRAD.
struct PlainStat {
    static constexpr bool kCounted = true;
    struct Args {
        int64_t ignore;
        const long long *kept;
    };
    struct alignas(16) Lds {
        float m[kRowWavesMax], se[kRowWavesMax], ly[kRowWavesMax];
    };
    float m, se, ly;   // the thread's largest l, its sum exp(l - m), l[y] in the one thread that meets it
    float lg, scale, mg;
    bool keep;

    static Args args(const MotPlainHeadDesc &, const WideGeom &g, const long long *kept, int64_t) { return {g.ignore, kept}; }
    static __device__ __forceinline__ bool keeps(bool in_range, int64_t y, const Args &a) { return in_range && y != a.ignore; }
    static __device__ __forceinline__ bool oor(bool in_range, int64_t y, const Args &a) { return !in_range && y != a.ignore; }
    template <typename T, int NV, typename E>
    __device__ __forceinline__ void sweep(const RowVecs<T, NV> &rv, float c, int yvec, int yel, Lds &sh, E eval) {
        typedef LogitVec<T> Vec;
        m = -INFINITY;
        se = ly = 0.f;
        if (NV > 0) {
            rv.each([&](int idx, const Vec &v) __attribute__((always_inline)) {
#pragma unroll
                for (int e = 0; e < Vec::N; ++e) {
                    const float l = c * v.get(e);
                    m = fmaxf(m, l);
                    ly = idx == yvec && e == yel ? l : ly;   // a select: a conditional store through `this` would stay a branch
                }
                eval(idx, v);
            });
            m = rows_block_max(m, sh.m);   // the row's maximum, then the sum from the registers
            rv.each([&](int, const Vec &v) __attribute__((always_inline)) {
#pragma unroll
                for (int e = 0; e < Vec::N; ++e) se += __expf(c * v.get(e) - m);
            });
        } else {   // one sweep: the thread's online pair (every thread meets at least one vector: nvec > kRegV / 8 >= blockDim.x)
            rv.each([&](int idx, const Vec &v) __attribute__((always_inline)) {
                float l[Vec::N], vm = -INFINITY;
#pragma unroll
                for (int e = 0; e < Vec::N; ++e) {
                    l[e] = c * v.get(e);
                    vm = fmaxf(vm, l[e]);
                    ly = idx == yvec && e == yel ? l[e] : ly;
                }
                if (vm > m) {   // exp(-inf) = 0 at the first vector, where se = 0
                    se *= __expf(m - vm);
                    m = vm;
                }
#pragma unroll
                for (int e = 0; e < Vec::N; ++e) se += __expf(l[e] - m);
                eval(idx, v);
            });
            const float mt = m;   // the pairs merge in a fixed order: the workgroup's max, one rescale per thread, the fixed-order sum
            m = rows_block_max(mt, sh.m);
            se *= __expf(mt - m);
        }
    }
    // lse = m + log(se) is never formed: at logits of a few hundred its rounding (2^-16 at 300) would sit in every exp(l - lse) of the
    // row and in the loss term, so both subtract m first, as log_softmax does
    __device__ __forceinline__ float close(Lds &sh) {
        se = rows_block_sum(se, sh.se);
        ly = rows_block_sum(ly, sh.ly);   // one thread holds l[y], the others 0
        lg = __logf(se);
        return (m - ly) + lg;
    }
    __device__ __forceinline__ void store_stats(const Args &, int64_t, float) const {}
    // G = (c / kept) (exp((l - m) - log(se)) - onehot); a dropped row is a row of zeros whatever its logits hold
    __device__ __forceinline__ void grad_prep(bool keep_row, float c, const Args &a) {
        keep = keep_row;
        scale = keep ? c / (float)*a.kept : 0.f;
        float opaque = m;   // the same value behind an opaque copy: sharing l - m with the sum's sweep would hold a second row in registers
        asm volatile("" : "+v"(opaque));
        mg = opaque;
    }
    __device__ __forceinline__ float grad(float s, float c, bool hit) const {
        const float p = __expf((c * s - mg) - lg);
        return keep ? scale * (p - (hit ? 1.f : 0.f)) : 0.f;
    }
    // the compaction's launchers of the chunk loop, defined behind their kernels in the second half of this file
    static int compact_index(const int64_t *tgt, const WideGeom &g, const WideCompact &cx, long long *kept, uint32_t *status, hipStream_t stream);
    static int compact_zero_dropped(const int64_t *tgt, const WideGeom &g, const long long *kept, void *dx, hipStream_t stream);
    template <typename T>
    static int compact_gather(const T *x, const int64_t *tgt, const WideGeom &g, const WideCompact &cx, const long long *kept, int64_t s0, int64_t n,
                              hipStream_t stream);
    template <typename T>
    static int compact_chain_scatter(const T *x, const float *u, const WideGeom &g, const WideCompact &cx, const long long *kept, int64_t s0, int64_t n,
                                     T *dx, hipStream_t stream);
    static int compact_eval_rows(const int64_t *tgt, const WideGeom &g, const WideCompact &cx, const long long *kept, HeadEvalRows out, hipStream_t stream);
};

// the descriptor's checks, with `compact` the compact struct's behind them, then the geometry: the chunks run over n_rows, or over
// cap = min(max_kept, n_rows)
int plain_head_geom(const MotPlainHeadDesc *d, WideGeom *g, const char *fn, bool compact = false, const MotPlainHeadCompact *c = nullptr) {
    if (!d) return set_error(MOT_EINVAL, "%s: null descriptor", fn);
    if (d->struct_size != sizeof(MotPlainHeadDesc))
        return set_error(MOT_EINVAL, "%s: struct_size %u != %zu (ABI mismatch)", fn, d->struct_size, sizeof(MotPlainHeadDesc));
    if (int rc = wide_shape_check(fn, d->dtype, d->n_rows, d->model_dim, d->vocab, &d->chunk_rows)) return rc;
    if (d->group_rows < 0 || (d->group_rows > 0 && d->n_rows % d->group_rows))
        return set_error(MOT_ESHAPE, "%s: group_rows %d must be 0 (no groups) or divide n_rows %lld", fn, d->group_rows, (long long)d->n_rows);
    if (compact) {
        if (!c) return set_error(MOT_EINVAL, "%s: null compact struct", fn);
        if (c->struct_size != sizeof(MotPlainHeadCompact))
            return set_error(MOT_EINVAL, "%s: compact struct_size %u != %zu (ABI mismatch)", fn, c->struct_size, sizeof(MotPlainHeadCompact));
        if (c->reserved) return set_error(MOT_EINVAL, "%s: compact reserved %u must be 0", fn, c->reserved);
        if (c->max_kept <= 0) return set_error(MOT_ESHAPE, "%s: max_kept %lld must be positive", fn, (long long)c->max_kept);
    }
    g->group = d->group_rows;
    g->ignore = d->ignore_index;
    g->counted = true;
    g->compact = compact;
    wide_geom_fill(*d, compact && c->max_kept < d->n_rows ? c->max_kept : d->n_rows, *g);
    return MOT_OK;
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

int PlainStat::compact_index(const int64_t *tgt, const WideGeom &g, const WideCompact &cx, long long *kept, uint32_t *status, hipStream_t stream) {
    const int parts = compact_parts(g.rows);
    hipLaunchKernelGGL(compact_count, dim3(parts), dim3(kThreads), 0, stream, tgt, g.rows, g.V, g.ignore, cx.scan, status);
    if (int rc = check_launch("compact_count")) return rc;
    hipLaunchKernelGGL(compact_scan, dim3(1), dim3(64), 0, stream, cx.scan, parts, (long long)g.over, kept, status);
    if (int rc = check_launch("compact_scan")) return rc;
    hipLaunchKernelGGL(compact_write, dim3(parts), dim3(kThreads), 0, stream, tgt, g.rows, g.V, g.ignore, (const long long *)cx.scan, (const long long *)kept,
                       (long long)g.over, cx.idx);
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
    norm_round_row<T>(x + r * K, K, norm_in, eps, out);
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

inline dim3 wave_grid(int64_t n) { return dim3((unsigned)((n + kWaves - 1) / kWaves)); }   // one wave per row or slot

int PlainStat::compact_zero_dropped(const int64_t *tgt, const WideGeom &g, const long long *kept, void *dx, hipStream_t stream) {
    const int vecs = g.K * (g.bf16 ? 2 : 4) / 16;   // model_dim is a multiple of 16: whole 16-byte vectors in both dtypes
    hipLaunchKernelGGL(mot::compact_zero_dropped, wave_grid(g.rows), dim3(kThreads), 0, stream, tgt, g.rows, g.V, g.ignore, kept, vecs, (uint4 *)dx);
    return check_launch("compact_zero_dropped");
}

template <typename T>
int PlainStat::compact_gather(const T *x, const int64_t *tgt, const WideGeom &g, const WideCompact &cx, const long long *kept, int64_t s0, int64_t n,
                              hipStream_t stream) {
    hipLaunchKernelGGL(mot::compact_gather<T>, wave_grid(n), dim3(kThreads), 0, stream, x, g.K, g.norm_in, g.eps, tgt, (const int32_t *)cx.idx, kept, s0, n, g.ignore,
                       (T *)cx.hg, cx.tg);
    return check_launch("compact_gather");
}

template <typename T>
int PlainStat::compact_chain_scatter(const T *x, const float *u, const WideGeom &g, const WideCompact &cx, const long long *kept, int64_t s0, int64_t n,
                                     T *dx, hipStream_t stream) {
    hipLaunchKernelGGL(mot::compact_chain_scatter<T>, wave_grid(n), dim3(kThreads), 0, stream, x, u, g.K, g.norm_in, g.eps, (const int32_t *)cx.idx, kept, s0, n, dx);
    return check_launch("compact_chain_scatter");
}

int PlainStat::compact_eval_rows(const int64_t *tgt, const WideGeom &g, const WideCompact &cx, const long long *kept, HeadEvalRows out, hipStream_t stream) {
    const int64_t span = g.rows > g.over ? g.rows : g.over;
    hipLaunchKernelGGL(mot::compact_eval_rows, dim3((unsigned)((span + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, tgt, g.rows, g.V, g.ignore,
                       (const int32_t *)cx.idx, kept, cx.slot, out);
    return check_launch("compact_eval_rows");
}

}  // namespace

size_t plain_head_compact_workspace_bytes(const MotPlainHeadDesc *d, const MotPlainHeadCompact *c) {
    WideGeom g;
    if (plain_head_geom(d, &g, "mot_plain_head_compact_workspace_bytes", true, c) || g.rows == 0) return 0;
    return wide_ws(g).total;
}

int launch_plain_head_compact_fwd(const MotPlainHeadDesc *d, const MotPlainHeadCompact *c, hipStream_t stream) {
    static const char fn[] = "mot_plain_head_compact_fwd";
    WideGeom g;
    if (int rc = plain_head_geom(d, &g, fn, true, c)) return rc;
    return wide_launch<PlainStat>(*d, g, nullptr, fn, stream);
}

int launch_plain_head_compact_eval(const MotPlainHeadDesc *d, const MotPlainHeadCompact *c, const MotHeadEvalOut *out, hipStream_t stream) {
    static const char fn[] = "mot_plain_head_compact_eval";
    WideGeom g;
    int rc = plain_head_geom(d, &g, fn, true, c);
    if (rc || (rc = head_eval_check(fn, out))) return rc;
    if (d->dx || d->dW) return set_error(MOT_EINVAL, "%s: dx / dW set: the evaluation forms no gradients (mot_plain_head_compact_fwd does)", fn);
    return wide_launch<PlainStat>(*d, g, out, fn, stream);
}

size_t plain_head_workspace_bytes(const MotPlainHeadDesc *d) {
    WideGeom g;
    if (plain_head_geom(d, &g, "mot_plain_head_workspace_bytes") || g.rows == 0) return 0;
    return wide_ws(g).total;
}

int launch_plain_head_fwd(const MotPlainHeadDesc *d, hipStream_t stream) {
    static const char fn[] = "mot_plain_head_fwd";
    WideGeom g;
    if (int rc = plain_head_geom(d, &g, fn)) return rc;
    return wide_launch<PlainStat>(*d, g, nullptr, fn, stream);
}

int launch_plain_head_eval(const MotPlainHeadDesc *d, const MotHeadEvalOut *out, hipStream_t stream) {
    static const char fn[] = "mot_plain_head_eval";
    WideGeom g;
    int rc = plain_head_geom(d, &g, fn);
    if (rc || (rc = head_eval_check(fn, out))) return rc;
    if (d->dx || d->dW) return set_error(MOT_EINVAL, "%s: dx / dW set: the evaluation forms no gradients (mot_plain_head_fwd does)", fn);
    return wide_launch<PlainStat>(*d, g, out, fn, stream);
}

}  // namespace mot
