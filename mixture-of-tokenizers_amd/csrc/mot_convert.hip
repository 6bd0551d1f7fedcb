// mot_convert.hip -- element-type and layout conversions between the fp32 and bf16 sides of a pass: widen (bf16 -> fp32),
// narrow (fp32 -> bf16), transpose_bf16 and narrow_transpose (k-major copies of a weight for the bf16 products).
// Callers: the CONCAT_LINEAR backward (mot_bwd_linear.hip: widen, narrow, transpose_bf16), the MEAN backward (mot_bwd_mean.hip:
// widen), cross-attention (mot_attn.hip: narrow, narrow_transpose), the character mixer (mot_swa.hip: narrow), and for transpose_bf16
// the linear-on-bytes mixin (mot_bytefc.hip), the MoT value embeddings (mot_valuemix.hip) and the two output heads (mot_head.hip,
// mot_tokhead.hip).
#include "mot_mix.hpp"

namespace mot {

__global__ __launch_bounds__(kThreads) void widen_kernel(const __bf16 *__restrict__ src, int64_t n, float *__restrict__ dst) {
    for (int64_t i = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * 8; i < n; i += (int64_t)gridDim.x * kThreads * 8) {
        if (i + 8 <= n && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
            const float8v v = Elem<__bf16>::loadv(src + i);
            *(float4v *)(dst + i) = __builtin_shufflevector(v, v, 0, 1, 2, 3);
            *(float4v *)(dst + i + 4) = __builtin_shufflevector(v, v, 4, 5, 6, 7);
        } else {
            for (int64_t j = i; j < min(n, i + 8); ++j) dst[j] = (float)src[j];
        }
    }
}
int launch_widen(const void *src, size_t n, float *dst, hipStream_t stream) {
    if (!n) return MOT_OK;
    size_t blocks = (n / 8 + kThreads) / kThreads;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(widen_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, stream, (const __bf16 *)src, (int64_t)n, dst);
    return check_launch("widen_kernel");
}

__global__ __launch_bounds__(kThreads) void narrow_kernel(const float *__restrict__ src, int64_t n, __bf16 *__restrict__ dst) {
    for (int64_t i = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * 8; i < n; i += (int64_t)gridDim.x * kThreads * 8) {
        if (i + 8 <= n) {   // both buffers are 256-byte aligned workspace regions
            float8v v;
            const float4v a = *(const float4v *)(src + i), b = *(const float4v *)(src + i + 4);
            v = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
            Elem<__bf16>::storev_nt(dst + i, v);
        } else {
            for (int64_t j = i; j < n; ++j) dst[j] = (__bf16)src[j];
        }
    }
}
// dst[i] = bf16(src[i]); both 16-byte aligned
int launch_narrow(const float *src, int64_t n, void *dst, hipStream_t stream) {
    if (n <= 0) return MOT_OK;
    size_t nb = ((size_t)n / 8 + kThreads) / kThreads;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(narrow_kernel, dim3((unsigned)nb), dim3(kThreads), 0, stream, src, n, (__bf16 *)dst);
    return check_launch("narrow_kernel");
}

// dst[c][r] = src[r][c]   (rows x cols -> cols x rows), bf16, 32 x 32 tiles through LDS
__global__ __launch_bounds__(kThreads) void transpose_bf16_kernel(const __bf16 *__restrict__ src, int rows, int cols, __bf16 *__restrict__ dst) {
    __shared__ __bf16 tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    for (int r = ty; r < 32; r += 8)
        tile[r][tx] = (r0 + r < rows && c0 + tx < cols) ? src[(int64_t)(r0 + r) * cols + c0 + tx] : (__bf16)0.f;
    __syncthreads();
    for (int c = ty; c < 32; c += 8)
        if (c0 + c < cols && r0 + tx < rows) dst[(int64_t)(c0 + c) * rows + r0 + tx] = tile[tx][c];
}

// dst[c][r] = bf16(src[r][c])   (fp32 rows x cols -> bf16 cols x rows): the k-major copy of a weight for gemm_rows_bf16
__global__ __launch_bounds__(kThreads) void narrow_transpose_kernel(const float *__restrict__ src, int rows, int cols, __bf16 *__restrict__ dst) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    for (int r = ty; r < 32; r += 8)
        tile[r][tx] = (r0 + r < rows && c0 + tx < cols) ? src[(int64_t)(r0 + r) * cols + c0 + tx] : 0.f;
    __syncthreads();
    for (int c = ty; c < 32; c += 8)
        if (c0 + c < cols && r0 + tx < rows) dst[(int64_t)(c0 + c) * rows + r0 + tx] = (__bf16)tile[tx][c];
}
int launch_transpose_bf16(const void *src, int rows, int cols, void *dst, hipStream_t stream) {
    hipLaunchKernelGGL(transpose_bf16_kernel, dim3((unsigned)((cols + 31) / 32), (unsigned)((rows + 31) / 32)), dim3(kThreads), 0, stream, (const __bf16 *)src,
                       rows, cols, (__bf16 *)dst);
    return check_launch("transpose_bf16_kernel");
}
int launch_narrow_transpose(const float *src, int rows, int cols, void *dst, hipStream_t stream) {
    if (rows <= 0 || cols <= 0) return MOT_OK;
    hipLaunchKernelGGL(narrow_transpose_kernel, dim3((unsigned)((cols + 31) / 32), (unsigned)((rows + 31) / 32)), dim3(kThreads), 0, stream, src, rows, cols,
                       (__bf16 *)dst);
    return check_launch("narrow_transpose_kernel");
}

}  // namespace mot
