// mot_rowloss.hpp -- what the two output heads (mot_head.hip: the 512-row byte head, mot_tokhead.hip: the token-level head) share:
// the factor of the row's closing rms-norm with its derivative, and the loss as a fixed-order double sum of per-row terms.
// Each translation unit gets its own copy of the two kernels (internal linkage); the code, and so the bits, are the same.
#pragma once
#include "mot_internal.hpp"
#include "mot_tile.hpp"

namespace mot {
namespace {

// norm(h_L) = c x_row and dc/dm0, for n_layer_out identity layers h <- h + norm(h) = h (1 + r), r = (mean(h^2) + eps)^-1/2:
// each layer scales the row by (1 + r) and its mean square by (1 + r)^2; the derivative is carried forward alongside.
// L = 0 is the plain norm: c = (m0 + eps)^-1/2, dc = -c^3 / 2.
__device__ __forceinline__ void row_scale(float m0, int L, float eps, float &c, float &dc) {
    float m = m0, dm = 1.f;
    c = 1.f;
    dc = 0.f;
    for (int i = 0; i < L; ++i) {
        const float r = rsqrtf(m + eps), dr = -0.5f * r * r * r * dm, a = 1.f + r;
        dc = dc * a + c * dr;
        c *= a;
        dm = dm * a * a + 2.f * m * a * dr;
        m *= a * a;
    }
    const float r = rsqrtf(m + eps);
    dc = dc * r - 0.5f * c * r * r * r * dm;
    c *= r;
}

// The loss: per-row terms summed in a fixed order in double, in two launches.  Workgroup p of a grid that depends on the row count
// only sums its fixed range of rows into part[p]; one workgroup then sums the parts in order and scales by 1 / M.
constexpr int kLossParts = 512;

__host__ __device__ inline int loss_parts(int64_t rows) {
    const int64_t p = (rows + 2047) / 2048;
    return (int)(p < 1 ? 1 : p > kLossParts ? kLossParts : p);
}

__device__ __forceinline__ double block_sum(double a, double *sh) {
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

}  // namespace
}  // namespace mot
