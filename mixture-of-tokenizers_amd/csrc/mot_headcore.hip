// mot_headcore.hip -- the kernels the output heads share (mot_headcore.hpp), each with its launcher: head_chain_rows, the
// wave-per-row chain that closes dx behind u = G W, head_loss_parts / head_loss_final, the loss as a sum of per-row terms, and
// head_count_parts / head_count_final, the counts of the evaluation calls, with the check of their out struct, and
// head_kept_parts / head_kept_final / head_loss_final_kept, the plain head's device count of kept rows and the loss divided by it.
#include "mot_headcore.hpp"

namespace mot {

// dx_r = u_r + (dc/dm0) (2 / K) (x_r . u_r / c_r) x_r; at L = 0 that is u_r - c_r^2 (x_r . u_r / K) x_r, the plain norm's.  Without
// norm_in the row is u_r itself (not u_r + 0 x_r: a non-finite x stays out of dx).
template <typename T>
__global__ __launch_bounds__(kThreads) void head_chain_rows(const T *__restrict__ x, const float *__restrict__ u, int K, int64_t rows, int L, int norm_in,
                                                            float eps, T *__restrict__ dx) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (r >= rows) return;
    const T *xr = x + r * K;
    const float *ur = u + r * K;
    if (!norm_in) {
        for (int k = lane; k < K; k += 64) dx[r * K + k] = (T)ur[k];
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
    // a row that is zero to fp32's sum of squares has dx_r = u_r: its x term is 0 x_r, whatever the factor (which no format holds at L > 44)
    const float m0 = ss / (float)K;
    const float coef = m0 > 0.f ? (float)(row_scale_dlog((double)m0, L, (double)eps) * (2.0 / (double)K) * (double)xu) : 0.f;
    for (int k = lane; k < K; k += 64) dx[r * K + k] = (T)(ur[k] + coef * (float)xr[k]);
}

template <typename T>
int launch_head_chain(const T *x, const float *u, int K, int64_t n, int L, int norm_in, float eps, T *dx, hipStream_t stream) {
    hipLaunchKernelGGL(head_chain_rows<T>, dim3((unsigned)((n + kWaves - 1) / kWaves)), dim3(kThreads), 0, stream, x, u, K, n, L, norm_in, eps, dx);
    return check_launch("head_chain_rows");
}
template int launch_head_chain<float>(const float *, const float *, int, int64_t, int, int, float, float *, hipStream_t);
template int launch_head_chain<__bf16>(const __bf16 *, const float *, int, int64_t, int, int, float, __bf16 *, hipStream_t);

// The loss: per-row terms summed in a fixed order in double, in two launches.  Workgroup p of a grid that depends on the row count
// only sums its fixed range of rows into part[p]; one workgroup then sums the parts in order and scales by 1 / M.
static int loss_parts(int64_t rows) {
    const int64_t p = (rows + 2047) / 2048;
    return (int)(p < 1 ? 1 : p > kLossParts ? kLossParts : p);
}

template <typename A>
static __device__ __forceinline__ A block_sum(A a, A *sh) {
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int o = kThreads / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    return sh[0];
}

__global__ __launch_bounds__(kThreads) void head_loss_parts(const float *__restrict__ term, int64_t rows, double *__restrict__ part) {
    __shared__ double sh[kThreads];
    const int64_t per = (rows + gridDim.x - 1) / gridDim.x, lo = (int64_t)blockIdx.x * per, hi = lo + per < rows ? lo + per : rows;
    double a = 0.0;
    int64_t i = lo + threadIdx.x;
    for (; i + 3 * kThreads < hi; i += 4 * kThreads) {   // four loads in flight, summed in index order
        const float t0 = term[i], t1 = term[i + kThreads], t2 = term[i + 2 * kThreads], t3 = term[i + 3 * kThreads];
        a += (double)t0;
        a += (double)t1;
        a += (double)t2;
        a += (double)t3;
    }
    for (; i < hi; i += kThreads) a += (double)term[i];
    const double s = block_sum(a, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(kThreads) void head_loss_final(const double *__restrict__ part, int parts, double inv_m, float *__restrict__ loss) {
    __shared__ double sh[kThreads];
    double a = 0.0;
    for (int i = threadIdx.x; i < parts; i += kThreads) a += part[i];
    const double s = block_sum(a, sh);
    if (threadIdx.x == 0) *loss = (float)(s * inv_m);
}

int launch_head_loss(const float *term, int64_t rows, double *part, double inv_m, float *loss, hipStream_t stream) {
    const int parts = loss_parts(rows);
    hipLaunchKernelGGL(head_loss_parts, dim3(parts), dim3(kThreads), 0, stream, term, rows, part);
    if (int rc = check_launch("head_loss_parts")) return rc;
    hipLaunchKernelGGL(head_loss_final, dim3(1), dim3(kThreads), 0, stream, part, parts, inv_m, loss);
    return check_launch("head_loss_final");
}

// The plain head's divisor: the number of kept rows (target in [0, vocab) and not `ignore`), counted on the device in front of the
// first chunk as integer sums laid out as the loss's, and its loss close, which divides by that count (0 / 0 = NaN at no kept row,
// as F.cross_entropy returns).
__global__ __launch_bounds__(kThreads) void head_kept_parts(const int64_t *__restrict__ tgt, int64_t rows, int vocab, int64_t ignore,
                                                            long long *__restrict__ part) {
    __shared__ long long sh[kThreads];
    const int64_t per = (rows + gridDim.x - 1) / gridDim.x, lo = (int64_t)blockIdx.x * per, hi = lo + per < rows ? lo + per : rows;
    long long n = 0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += kThreads) {
        const int64_t y = tgt[i];
        n += y >= 0 && y < vocab && y != ignore;
    }
    n = block_sum(n, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = n;
}

__global__ __launch_bounds__(64) void head_kept_final(const long long *__restrict__ part, int parts, long long *__restrict__ kept) {
    if (threadIdx.x) return;
    long long a = 0;
    for (int p = 0; p < parts; ++p) a += part[p];
    *kept = a;
}

int launch_head_kept(const int64_t *tgt, int64_t rows, int vocab, int64_t ignore, void *part, long long *kept, hipStream_t stream) {
    const int parts = loss_parts(rows);
    hipLaunchKernelGGL(head_kept_parts, dim3(parts), dim3(kThreads), 0, stream, tgt, rows, vocab, ignore, (long long *)part);
    if (int rc = check_launch("head_kept_parts")) return rc;
    hipLaunchKernelGGL(head_kept_final, dim3(1), dim3(64), 0, stream, (const long long *)part, parts, kept);
    return check_launch("head_kept_final");
}

__global__ __launch_bounds__(kThreads) void head_loss_final_kept(const double *__restrict__ part, int parts, const long long *__restrict__ kept,
                                                                 float *__restrict__ loss) {
    __shared__ double sh[kThreads];
    double a = 0.0;
    for (int i = threadIdx.x; i < parts; i += kThreads) a += part[i];
    const double s = block_sum(a, sh);
    if (threadIdx.x == 0) *loss = (float)(s / (double)*kept);
}

int launch_head_loss_kept(const float *term, int64_t rows, double *part, const long long *kept, float *loss, hipStream_t stream) {
    const int parts = loss_parts(rows);
    hipLaunchKernelGGL(head_loss_parts, dim3(parts), dim3(kThreads), 0, stream, term, rows, part);
    if (int rc = check_launch("head_loss_parts")) return rc;
    hipLaunchKernelGGL(head_loss_final_kept, dim3(1), dim3(kThreads), 0, stream, part, parts, kept, loss);
    return check_launch("head_loss_final_kept");
}

// The counts of an evaluation call, closed from what its row passes wrote: a row counts when its target lies in [0, vocab), it is a
// hit when pred equals that target, and a group (`per` consecutive rows: the byte positions of a token; 1 for the token-level head)
// is all-correct when every row of it is a hit.  Integer sums, laid out as the loss's: workgroup p sums its fixed range of groups
// into part[3 p ..], one workgroup then sums the parts in order.
// The plain head's form (skip_dropped, with its `ignore`; the other heads pass 0 and a value outside [0, vocab), which changes
// nothing for them): a row that does not count neither makes nor breaks its group, and a group with no counted row is not all-correct.
constexpr int kCountParts = kLossParts / 3;

__global__ __launch_bounds__(kThreads) void head_count_parts(const int32_t *__restrict__ pred, const int64_t *__restrict__ tgt, int64_t groups, int per,
                                                             int vocab, int skip_dropped, int64_t ignore, long long *__restrict__ part) {
    __shared__ long long sh[kThreads];
    const int64_t span = (groups + gridDim.x - 1) / gridDim.x, lo = (int64_t)blockIdx.x * span, hi = lo + span < groups ? lo + span : groups;
    long long n_in = 0, n_hit = 0, n_all = 0;
    for (int64_t g = lo + threadIdx.x; g < hi; g += kThreads) {
        bool all = true, any = false;
        for (int k = 0; k < per; ++k) {
            const int64_t y = tgt[g * (int64_t)per + k];
            const bool in = y >= 0 && y < vocab && y != ignore, hit = in && (int64_t)pred[g * (int64_t)per + k] == y;
            n_in += in;
            n_hit += hit;
            any = any || in;
            all = all && (hit || (skip_dropped && !in));
        }
        n_all += all && (any || !skip_dropped);
    }
    n_in = block_sum(n_in, sh);
    __syncthreads();   // sh is read by every thread before the next sum overwrites it
    n_hit = block_sum(n_hit, sh);
    __syncthreads();
    n_all = block_sum(n_all, sh);
    if (threadIdx.x == 0) {
        part[3 * blockIdx.x] = n_in;
        part[3 * blockIdx.x + 1] = n_hit;
        part[3 * blockIdx.x + 2] = n_all;
    }
}

__global__ __launch_bounds__(64) void head_count_final(const long long *__restrict__ part, int parts, int64_t *__restrict__ counts, int n_counts) {
    const int j = threadIdx.x;
    if (j >= n_counts) return;
    long long a = 0;
    for (int p = 0; p < parts; ++p) a += part[3 * p + j];
    counts[j] = a;
}

int launch_head_eval_counts(const int32_t *pred, const int64_t *tgt, int64_t groups, int per, int vocab, void *part, int64_t *counts, int n_counts,
                            hipStream_t stream, int skip_dropped, int64_t ignore) {
    const int parts = loss_parts(groups) < kCountParts ? loss_parts(groups) : kCountParts;
    hipLaunchKernelGGL(head_count_parts, dim3(parts), dim3(kThreads), 0, stream, pred, tgt, groups, per, vocab, skip_dropped, ignore, (long long *)part);
    if (int rc = check_launch("head_count_parts")) return rc;
    hipLaunchKernelGGL(head_count_final, dim3(1), dim3(64), 0, stream, (const long long *)part, parts, counts, n_counts);
    return check_launch("head_count_final");
}

int head_eval_check(const char *fn, const MotHeadEvalOut *o) {
    if (!o) return set_error(MOT_EINVAL, "%s: null out struct", fn);
    if (o->struct_size != sizeof(MotHeadEvalOut))
        return set_error(MOT_EINVAL, "%s: out struct_size %u != %zu (ABI mismatch)", fn, o->struct_size, sizeof(MotHeadEvalOut));
    if (o->reserved) return set_error(MOT_EINVAL, "%s: reserved %u must be 0", fn, o->reserved);
    if (((uintptr_t)o->row_loss & 3) || ((uintptr_t)o->pred & 3) || ((uintptr_t)o->rank & 3) || ((uintptr_t)o->counts & 7))
        return set_error(MOT_EINVAL, "%s: row_loss, pred and rank must be 4-byte aligned, counts 8-byte aligned", fn);
    if (o->counts && !o->pred) return set_error(MOT_EINVAL, "%s: counts are closed from pred and the targets: counts needs pred", fn);
    return MOT_OK;
}

}  // namespace mot
