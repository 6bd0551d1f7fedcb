// mot_headrows.hpp -- the V-wide row pass of the cross-entropy heads: the limits and the geometry of a row pass, 16 bytes of a row of
// logits, the workgroup's fixed-order sums, the evaluation's share of a vector, and wide_rows, the one shell of the row pass, which
// the token-level head (TokStat, mot_tokhead.hip) and the plain head (PlainStat, mot_plainhead.hip) fill with their arithmetic, with
// its launcher.  The generation step (mot_nexttoken.hip) takes the vectors, the geometry and norm_round_row from here.
#pragma once
#include "mot_headcore.hpp"

namespace mot {

constexpr int kMinV = 128, kMaxV = 262144, kMaxD = 2048;
constexpr int64_t kChunkBytes = 512ll << 20;      // the library's chunk: logits and u of a chunk stay below this
constexpr int kRowThreads = 1024;                 // workgroup of the row pass at wide rows; kRowThreadsSmall when a row has <= 1024 vectors
constexpr int kRowThreadsSmall = 256;
constexpr int kRowWavesMax = kRowThreads / 64;
constexpr int kRegV = 65536;                      // widest row the row pass keeps in registers between its two uses

// 16 bytes of a row of logits: 4 fp32 or 8 bf16
template <typename T>
struct LogitVec;
template <>
struct LogitVec<float> {
    static constexpr int N = 4;
    float4 q;
    __device__ __forceinline__ float get(int e) const { return e == 0 ? q.x : e == 1 ? q.y : e == 2 ? q.z : q.w; }
    __device__ __forceinline__ void put(const float *v) { q = make_float4(v[0], v[1], v[2], v[3]); }
};
template <>
struct LogitVec<__bf16> {
    static constexpr int N = 8;
    uint4 q;
    __device__ __forceinline__ float get(int e) const {
        const uint32_t w = e < 2 ? q.x : e < 4 ? q.y : e < 6 ? q.z : q.w;
        return __uint_as_float((e & 1) ? (w & 0xffff0000u) : (w << 16));
    }
    static __device__ __forceinline__ uint32_t pack(float lo, float hi) {   // two roundings to nearest even
        const __bf16 a = (__bf16)lo, b = (__bf16)hi;
        return (uint32_t)__builtin_bit_cast(unsigned short, a) | ((uint32_t)__builtin_bit_cast(unsigned short, b) << 16);
    }
    __device__ __forceinline__ void put(const float *v) { q = make_uint4(pack(v[0], v[1]), pack(v[2], v[3]), pack(v[4], v[5]), pack(v[6], v[7])); }
};

// workgroup size and vectors per thread of a row pass over V classes of T: 256 threads while a row has at most 1024 vectors
template <typename T>
inline void rows_geometry(int V, int &threads, int &vecs_per_thread) {
    const int nvec = V / LogitVec<T>::N;
    threads = nvec <= 4 * kRowThreadsSmall ? kRowThreadsSmall : kRowThreads;
    vecs_per_thread = (nvec + threads - 1) / threads;
}

// sum over the workgroup in a fixed order: the waves' DPP sums, then the waves in index order.  `sh` holds one float per wave and is
// used by one sum only, so a single barrier suffices.
__device__ __forceinline__ float rows_block_sum(float v, float *sh) {
    const int nw = blockDim.x >> 6;
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = 0.f;
    for (int w = 0; w < nw; ++w) s += sh[w];
    return s;
}

// the workgroup's largest value, laid out as rows_block_sum: the waves' DPP maxima, then the waves in index order
__device__ __forceinline__ float rows_block_max(float v, float *sh) {
    const int nw = blockDim.x >> 6;
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    float m = sh[0];
    for (int w = 1; w < nw; ++w) m = fmaxf(m, sh[w]);
    return m;
}

// the evaluation's share of one vector whose first class is cls0, on the logits as stored: the largest so far with its class (a
// thread meets its classes in ascending order, so `>` keeps the lowest class of equal logits) and the count of those above sy
template <typename T>
__device__ __forceinline__ void vec_top(const LogitVec<T> &a, int cls0, float sy, float &best, int &best_cls, int &above) {
    int n = 0;   // this vector's count: one add into the thread's
#pragma unroll
    for (int e = 0; e < LogitVec<T>::N; ++e) {
        const float s = a.get(e);
        if (s > best) {
            best = s;
            best_cls = cls0 + e;
        }
        n += s > sy ? 1 : 0;
    }
    above += n;
}

// One wave: dst[0, K) = the row xr as a product takes it.  With norm_in it is normed HERE, T(c xr) with c = (mean(xr^2) + eps)^-1/2
// in fp32, and rounded to the call's dtype as F.rms_norm's output is in front of lm_head; else it is copied.
template <typename T>
__device__ __forceinline__ void norm_round_row(const T *__restrict__ xr, int K, int norm_in, float eps, T *dst) {
    const int lane = threadIdx.x & 63;
    float c = 1.f;
    if (norm_in) {
        float ss = 0.f, dc;
        for (int k = lane; k < K; k += 64) {
            const float v = (float)xr[k];
            ss += v * v;
        }
        row_scale(wave_sum(ss) / (float)K, 0, eps, c, dc);
    }
    for (int k = lane; k < K; k += 64) dst[k] = norm_in ? (T)(c * (float)xr[k]) : xr[k];
}

// A thread's 16-byte vectors of its row.  NV > 0: the row's vectors (nvec = V / N <= NV * blockDim.x) stay in registers between
// their uses, vector i of thread t is number t + i * blockDim.x, so a wave's 64 lanes touch 1 KiB at a time and the ragged last
// round is a predicate.  NV == 0: rows too wide for the register file (V above kRegV) are read again by every sweep.
template <typename T, int NV>
struct RowVecs {
    typedef LogitVec<T> Vec;
    Vec *row;
    int tid, nt, nvec;
    Vec a[NV > 0 ? NV : 1];
    __device__ __forceinline__ void load() {   // every load of the row is in flight before anything waits
        if (NV > 0) {
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int idx = tid + i * nt;
                if (idx < nvec) a[i] = row[idx];
            }
        }
    }
    template <typename F>
    __device__ __forceinline__ void each(F &&f) const {   // f(number of the vector, the vector), in ascending order
        if (NV > 0) {
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int idx = tid + i * nt;
                if (idx < nvec) f(idx, a[i]);
            }
        } else {
            for (int idx = tid; idx < nvec; idx += nt) {
                const Vec v = row[idx];
                f(idx, v);
            }
        }
    }
    template <typename F>
    __device__ __forceinline__ void rewrite(F &&f) {   // f changes the vector in place, then it is stored over the row
        if (NV > 0) {
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int idx = tid + i * nt;
                if (idx < nvec) {
                    f(idx, a[i]);
                    row[idx] = a[i];
                }
            }
        } else {
            for (int idx = tid; idx < nvec; idx += nt) {
                Vec v = row[idx];
                f(idx, v);
                row[idx] = v;
            }
        }
    }
};

// The row pass of the V-wide cross-entropy heads: one workgroup per row of the chunk.  It loads the row's logits ONCE into registers
// (RowVecs), forms the norm factor c, the row's statistics and its loss term, and with GRAD writes G = dloss / dl in place over the
// logits from the same registers.  EVAL (never with GRAD) is the evaluation variant: the same sweep also carries the row's largest
// stored logit with its class and counts the stored logits above the target's, which every thread fetches for itself (one cached
// address); `ev` takes the results.
// Stat supplies what differs between the heads.  Types: Args (its kernel arguments) and Lds (one array per workgroup sum).  Static:
// keeps(in_range, y, args) and oor(in_range, y, args).  On an object that holds the thread's statistics: sweep(vecs, c, yvec, yel,
// lds, eval) runs the statistics over the thread's vectors and calls eval(idx, vec) once per vector; close(lds) sums them over the
// workgroup and returns the row's loss term; store_stats(args, r, c) is thread 0's; grad_prep(keep, c, args) then grad(stored
// logit, c, is the target) give one element of G.
template <typename T, typename Stat, int NV, bool GRAD, bool EVAL>
__global__ __launch_bounds__(kRowThreads) void wide_rows(T *S, int V, const T *__restrict__ x, int K, int norm_in, float eps,
                                                         const int64_t *__restrict__ tgt, int64_t rows, typename Stat::Args sa, float *__restrict__ term,
                                                         uint32_t *status, HeadEvalRows ev) {
    typedef LogitVec<T> Vec;
    __shared__ float sh_ss[kRowWavesMax];
    __shared__ typename Stat::Lds sh;
    __shared__ float sh_top[EVAL ? kRowWavesMax : 1], sh_above[EVAL ? kRowWavesMax : 1];
    __shared__ int sh_cls[EVAL ? kRowWavesMax : 1];
    const int64_t r = blockIdx.x;
    if (r >= rows) return;
    const int tid = threadIdx.x, nt = blockDim.x;
    RowVecs<T, NV> rv;
    rv.row = (Vec *)(S + r * (int64_t)V);
    rv.tid = tid;
    rv.nt = nt;
    rv.nvec = V / Vec::N;
    rv.load();
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
    const bool in_range = y >= 0 && y < V, keep = Stat::keeps(in_range, y, sa);
    const int yvec = in_range ? (int)(y / Vec::N) : -1, yel = in_range ? (int)(y % Vec::N) : -1;
    float sy = 0.f, best = -INFINITY;   // EVAL: the target's stored logit, the largest of this thread's
    int best_cls = 0x7fffffff, above = 0;
    if (EVAL && in_range) sy = (float)S[r * (int64_t)V + y];
    Stat st;
    st.sweep(rv, c, yvec, yel, sh, [&](int idx, const Vec &v) __attribute__((always_inline)) {
        if (EVAL) vec_top<T>(v, idx * Vec::N, sy, best, best_cls, above);
    });
    if (EVAL) {   // the waves' pairs, met in wave order behind the next sum's barrier
        wave_argmax(best, best_cls);
        if ((tid & 63) == 0) {
            sh_top[tid >> 6] = best;
            sh_cls[tid >> 6] = best_cls;
        }
    }
    const float row_term = st.close(sh);
    if (tid == 0) {
        term[r] = keep ? row_term : 0.f;
        st.store_stats(sa, r, c);
        if (Stat::oor(in_range, y, sa) && status) atomicOr(status, (uint32_t)MOT_STATUS_TARGET_OOR);
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
    st.grad_prep(keep, c, sa);
    rv.rewrite([&](int idx, Vec &v) __attribute__((always_inline)) {
        float g[Vec::N];
#pragma unroll
        for (int e = 0; e < Vec::N; ++e) g[e] = st.grad(v.get(e), c, idx == yvec && e == yel);
        v.put(g);
    });
}

// the row pass of one chunk of n rows: the workgroup size and the registers per thread follow the row's number of 16-byte vectors
template <typename T, typename Stat, bool GRAD, bool EVAL>
int launch_wide_rows(T *S, int V, const T *x, int K, int norm_in, float eps, const int64_t *tgt, int64_t n, const typename Stat::Args &sa, float *term,
                     uint32_t *status, HeadEvalRows ev, hipStream_t stream) {
    int nt, nv;
    rows_geometry<T>(V, nt, nv);
#define MOT_WIDE_ROWS(NV) \
    hipLaunchKernelGGL((wide_rows<T, Stat, NV, GRAD, EVAL>), dim3((unsigned)n), dim3(nt), 0, stream, S, V, x, K, norm_in, eps, tgt, n, sa, term, status, ev)
    // registers hold a row of up to kRegV classes (16 vectors a thread in fp32, 8 in bf16); a wider row is read twice
    if (nv <= 4) MOT_WIDE_ROWS(4);
    else if (nv <= 8) MOT_WIDE_ROWS(8);
    else if (V <= kRegV) MOT_WIDE_ROWS(kRegV / (kRowThreads * LogitVec<T>::N));   // 16 in fp32 (bf16 rows this wide took 8 above)
    else MOT_WIDE_ROWS(0);
#undef MOT_WIDE_ROWS
    return check_launch("wide_rows");
}

}  // namespace mot
